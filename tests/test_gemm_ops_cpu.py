"""CPU: the instruments of test_gemm_ops_gpu.py / test_attn_ops_gpu.py checked without a GPU.

1. The exact family really is exact: a float32 product of it summed in three different slab orders, and the split-pair emulation
   (hi = bf16(x), lo = bf16(x - hi), three passes), equal the float64 reference bit for bit at every (K, magnitude) pair the GPU
   file uses -- also with every operand at its largest magnitude and one sign, the worst partial sum.
2. Planted faults in an emulation of the tiled product.  The exact-family check (zero difference, every element written, nothing
   else touched) misses none of them; the random-family bounds catch the structural ones.  Caught by the exact family ONLY:
   the bf16 store that truncates instead of rounding (the random bound, 2^-8 max|ref| + 1e-3, is a full bf16 ulp of the largest
   output: a one-ulp error of any smaller element is inside it).
3. The float32 restatement of the kernels' tile-ordered online softmax stays within a quarter of each attention bound on the
   structured score cases.
"""
import math

import pytest

torch = pytest.importorskip("torch")

import _gemm_refs as R          # noqa: E402
from _gpu_guard import _bits, check_written          # noqa: E402

# every K the GPU file launches, per operand family
PLAIN_K = [32, 64, 128, 192, 256, 512, 1024, 1984, 2048, 2112, 4096]
SPLIT_K = [32, 64, 96, 128, 256, 768, 1024]
SENTINEL = 12345.0


def _ref(A, B):
    return A.double() @ B.double().t()


@pytest.mark.parametrize("K", PLAIN_K)
def test_exact_family_is_exact_in_fp32_in_any_slab_order(K):
    a, b = R.exact_mags(K)
    assert 1 <= a <= 127 and 1 <= b <= 127                       # bf16-exact integers
    for worst in (False, True):
        A, B = R.exact_operands(24, 40, K, seed=K)
        if worst:                                                # every product at its largest, all of one sign
            A, B = torch.full_like(A, a), torch.full_like(B, -b)
        assert torch.equal(A.to(torch.bfloat16).float(), A) and torch.equal(B.to(torch.bfloat16).float(), B)
        bias, resid = R.exact_vector(40, K + 1), R.exact_vector((24, 40), K + 2)
        if worst:
            bias, resid = -bias.abs(), -resid.abs()
        top = R.assert_exact_family(A, B, bias, resid)
        assert not worst or top > K * a * b                      # the bound is really approached
        ref = _ref(A, B) + bias.double() + resid.double()
        for order in ("fwd", "rev", "even_odd"):
            for slab in (32, 64):
                got = (R.tiled_product(A, B, slab=slab, order=order) + bias) + resid
                assert got.dtype == torch.float32 and torch.equal(got.double(), ref), (K, order, slab, worst)
        got = R.tiled_product(A, B, slab=32, sk_parts=3) + (bias + resid)          # partial tiles summed afterwards; another
        assert torch.equal(got.double(), ref), (K, "stream-K parts", worst)        # order of the epilogue's additions


@pytest.mark.parametrize("K", SPLIT_K)
@pytest.mark.parametrize("role", ["A", "B"])
def test_exact_split_family_is_exact_through_the_three_passes(K, role):
    a, b = R.exact_mags(K, split=True)
    assert a >= 512 and b >= 1                                   # more than 8 significant bits: hi and lo both carry some
    for worst in (False, True):
        A, B = R.exact_operands(24, 40, K, seed=K, split=role)
        if worst:
            big, small = (A, B) if role == "A" else (B, A)
            big.fill_(float(a) if a % 2 else float(a - 1))       # odd and > 256: lo != 0
            small.fill_(-float(b))
        wide = A if role == "A" else B
        hi, lo = R.split_pair(wide)
        assert torch.equal(hi.float() + lo.float(), wide)
        assert float(lo.float().abs().max()) > 0 and float(hi.float().abs().max()) > 0
        narrow_lo = R.split_pair(B if role == "A" else A)[1]
        assert float(narrow_lo.float().abs().max()) == 0.0       # the dropped lo.lo term is exactly 0
        bias, resid = R.exact_vector(40, K + 1), R.exact_vector((24, 40), K + 2)
        R.assert_exact_family(A, B, bias, resid, split=True)
        ref = _ref(A, B)
        assert torch.equal(R.split_product(A, B).double(), ref), (K, role, worst)
        # the pass that carries the low part of the wide operand is really needed: A_lo.B_hi for role A, A_hi.B_lo for role B
        if role == "A":
            assert not torch.equal(R.split_product(A, B, fault="drop_lo_hi").double(), ref)
        else:
            assert not torch.equal(R.split_product(B, A, fault="drop_lo_hi").double(), ref.t())


def test_split_output_identity():
    """A split output is split(ref); hi + lo == ref holds exactly when ref has at most 16 significant bits (|ref| < 2^16 here)."""
    ref = R.exact_vector(4096, 3, mag=2 ** 24 - 1)
    hi, lo = R.split_pair(ref)
    small = ref.abs() < 2 ** 16
    assert torch.equal((hi.float() + lo.float())[small], ref[small]) and int(small.sum()) > 0
    assert not torch.equal(hi.float() + lo.float(), ref)          # 24-bit values do not fit a pair: compare with split(ref)


# ------------------------------------------------------------------------------------------ planted faults
def _exact_catches(got, ref):
    """The exact-family check of the GPU file: every element written (no NaN left) and equal to the reference."""
    return bool(torch.isnan(got).any()) or not torch.equal(got.double(), ref)


def _bound_catches(got, ref, bound):
    return bool(torch.isnan(got).any()) or bool(((got.double() - ref).abs() > bound).any())


FAULTS = ["swap_tiles", "skip_last_slab", "sk_twice", "mask_off_by_one"]


@pytest.mark.parametrize("fault", FAULTS)
@pytest.mark.parametrize("K", [64, 1024])
def test_planted_tiling_faults_are_caught(fault, K):
    M, N = 20, 150                                               # three column tiles of 64, the last ragged
    sk = 4 if fault == "sk_twice" else 0
    A, B = R.exact_operands(M, N, K, seed=K)
    ref = _ref(A, B)
    assert not _exact_catches(R.tiled_product(A, B, sk_parts=sk), ref)
    assert _exact_catches(R.tiled_product(A, B, sk_parts=sk, fault=fault), ref), f"exact family misses {fault}"
    for bf16 in (False, True):
        A, B = R.random_operands(M, N, K, seed=K, bf16=bf16)
        ref, bound = _ref(A, B), R.accum_bound(A, B, bf16)
        assert not _bound_catches(R.tiled_product(A, B, sk_parts=sk), ref, bound)
        assert _bound_catches(R.tiled_product(A, B, sk_parts=sk, fault=fault), ref, bound), f"random family misses {fault}"
    print(f"[caught] {fault} K={K}: exact family yes, random family yes")


@pytest.mark.parametrize("K", [64, 1024])
def test_planted_dropped_cross_pass_is_caught(K):
    """A_lo.B_hi missing.  The exact family: any difference.  The random family's six-sigma budget also catches it (the missing
    pass is 2^-9 of the product against a 6 x 2^-16 budget), at K = 1024 as well."""
    A, B = R.exact_operands(20, 150, K, seed=K, split="A")
    assert _exact_catches(R.split_product(A, B, fault="drop_lo_hi"), _ref(A, B))
    A, B = R.random_operands(20, 150, K, seed=K, b_scale=0.25)
    ref, bound = _ref(A, B), R.x3_bound(A, B)
    good, bad = R.split_product(A, B), R.split_product(A, B, fault="drop_lo_hi")
    assert not _bound_catches(good, ref, bound)
    frac = float(((bad.double() - ref).abs() / bound).max())
    R.measure(f"cpu/gemm/fault/drop_lo_hi/K{K}/fraction_of_random_bound", frac)
    assert frac > 1.0


def _place_rows(val, row_div, fault):
    """What a row_div launch leaves in a Guarded2D: NaN where a write is expected, the sentinel elsewhere, then the rows written."""
    M, N = val.shape
    rows = (M // row_div) * (row_div + 1)
    mask = torch.zeros(rows, N, dtype=torch.bool)
    mask[[R.row_remap(m, row_div) for m in range(M)]] = True
    out = torch.full((rows, N), SENTINEL, dtype=val.dtype)
    out[mask] = float("nan")
    init_bits = _bits(out).clone()
    for m in range(M):
        out[R.row_remap(m, row_div, fault)] = val[m]
    return out, init_bits, mask


def test_planted_row_remap_fault_is_caught():
    """row_div remap without the + 1: token row 0 of every image is written and its last row is not.  Both families catch it
    through the GPU file's own written-region check (_gpu_guard.check_written, what Guarded2D.check applies): the sentinel of
    row 0 must survive and the last row must be written."""
    A, B = R.exact_operands(3 * 25, 40, 64, seed=1)
    val = _ref(A, B).float()
    check_written("row_div", *_place_rows(val, 25, False))
    with pytest.raises(AssertionError, match="outside the written region changed"):
        check_written("row_div without + 1", *_place_rows(val, 25, True))
    out, init_bits, mask = _place_rows(val, 25, True)
    out[torch.arange(3) * 26] = SENTINEL                         # even with the cls rows repaired, the unwritten last rows show
    with pytest.raises(AssertionError, match="not written"):
        check_written("row_div without + 1, last rows", out, init_bits, mask)


def test_planted_bf16_truncation_is_caught_by_the_exact_family_only():
    """Truncation is off by less than one bf16 ulp OF THE ELEMENT.  The exact family compares bits: caught.  The random bound is
    2^-8 max|ref| + 1e-3, a full ulp of the LARGEST output: no element below half the maximum can ever exceed it, although
    about half of them carry the fault."""
    A, B = R.exact_operands(20, 150, 256, seed=2)
    ref = _ref(A, B)
    want = ref.float().to(torch.bfloat16)
    bad = R.bf16_truncate(ref.float())
    assert not torch.equal(want.view(torch.int16), bad.view(torch.int16)), "exact family misses a truncating bf16 store"
    A, B = R.random_operands(20, 150, 256, seed=2, bf16=True)
    ref = _ref(A, B)
    want, bad = ref.float().to(torch.bfloat16), R.bf16_truncate(ref.float())
    small = ref.abs() < 0.5 * float(ref.abs().max())
    wrong = (want.view(torch.int16) != bad.view(torch.int16)) & small
    over = ((bad.double() - ref).abs() > R.bf16_out_bound(ref)) & small
    assert int(small.sum()) > 0.9 * ref.numel() and int(wrong.sum()) > 0.3 * int(small.sum())     # the fault is everywhere
    assert int(over.sum()) == 0                                                                   # and the bound sees none of it
    R.measure("cpu/gemm/fault/bf16_truncate/elements_wrong_below_half_max", int(wrong.sum()))
    print("[caught] bf16 truncation: exact family yes, random family no (below half the maximum: never)")


# ------------------------------------------------------------------------------------------ softmax restatement
@pytest.mark.parametrize("kind", ["f32", "bf16", "x3"])
@pytest.mark.parametrize("case", R.ATTN_CASES)
def test_softmax_restatement_uses_a_quarter_of_the_bound(case, kind):
    worst = 0.0
    for N, heads in ((33, 12), (257, 4), (442, 2)):
        q, k, v = R.make_attn_qkv(case, 1, N, heads, seed=N + heads)
        if kind == "bf16":
            q, k, v = (a.to(torch.bfloat16).float() for a in (q, k, v))
        elif kind == "x3":
            q, k, v = (sum(t.float() for t in R.split_pair(a)) for a in (q, k, v))
        ref, s = R.attn64(q, k, v, heads)
        got = R.attn_restated(q, k, v, heads, kind)
        assert bool(torch.isfinite(got).all())
        if case == "max_first" and N > 1:
            top2 = s.topk(2, dim=-1).values
            assert float((top2[..., 0] - top2[..., 1]).min()) >= 100.0
        if case == "outliers":
            assert float(s.abs().max()) >= 100.0
        worst = max(worst, float((got - ref).abs().max()) / R.attn_bound(kind, case, ref))
    R.measure(f"cpu/vit_attn/{kind}/{case}/restatement_fraction_of_bound", worst)
    assert worst <= 0.25, (kind, case, worst)


# ------------------------------------------------------------------------------------------ the library's launch plan
# pnp_op_gemm_plan is the function gemm_nt launches from; it needs no device.  The literals below are the independent statement of
# the dispatch (csrc/gemm.hip): they are written out, not computed from the library.
WIDE = dict(has=("bias", "out_t"))                  # + bias -> bf16: one of the wide kernel's epilogues
BOTH = dict(has=("bias", "out_f32", "out_t"))       # dual output: generic kernels only
X3 = dict(has=("bias", "out_f32"))                  # + bias -> fp32 of the split forms


def _plan(*a, **kw):
    from pnp_ovss import hip
    return hip.gemm_plan(*a, **kw)


def test_gemm_plan_matches_the_documented_thresholds():
    name = lambda *a, **kw: _plan(*a, **kw).name
    assert name("f32", 100, 191 * 128, 64, **BOTH) == "g64" and name("f32", 100, 191 * 128 + 1, 64, has=("out_f32",)) == "g128"
    assert name("bf16", 200, 127 * 256, 64, **WIDE) == "g128" and name("bf16", 200, 127 * 256 + 4, 64, **WIDE) == "wide"
    assert name("bf16", 257, 8192, 1984, **BOTH) == "g128" and name("bf16", 257, 8192, 2048, **BOTH) == "g256"
    assert name("bf16", 6144, 508, 2048, **BOTH) == "g128" and name("bf16", 6144, 512, 2048, **BOTH) == "g256"
    assert name("f32", 6144, 512, 2048, **BOTH) == "g128"
    assert name("bf16", 200, 127 * 256, 2048, **WIDE) == "g256" and name("bf16", 200, 127 * 256 + 4, 2048, **WIDE) == "wide"
    assert name("x3", 1, 4, 64, **X3) == "x3_wide" and name("x3a", 1, 4, 32, **X3) == "small_x3"
    assert math.isclose(R.GELU_SLOPE, 1.13)


def test_gemm_plan_tile_rounding_grid_and_lds_of_each_family():
    """N is rounded to the family's own tile; the generic and text-side kernels launch one workgroup per tile, the persistent
    ones min(tiles, CUs)."""
    f = lambda p: (p.name, p.variant, p.dtype_bf16, p.n_pad, p.grid, p.block, p.smem, p.keeps_stamps, p.profiled)
    assert f(_plan("f32", 100, 100, 64, **BOTH)) == ("g64", 0, 0, 128, 2 * 2, 256, 49152, 1, 0)
    assert f(_plan("bf16", 100, 191 * 128 + 1, 64, has=("out_f32", "out_t"))) == ("g128", 0, 1, 192 * 128, 192, 256, 65536, 1, 1)
    assert f(_plan("bf16", 257, 8196, 2048, **BOTH)) == ("g256", 0, 1, 8448, 2 * 33, 512, 131072, 1, 1)
    assert f(_plan("bf16", 200, 127 * 256 + 4, 64, n_cu=256, **WIDE)) == ("wide", 0, 1, 128 * 256, 128, 512, 135168, 1, 1)
    assert f(_plan("bf16", 200, 127 * 256 + 4, 64, n_cu=64, **WIDE)) == ("wide", 0, 1, 128 * 256, 64, 512, 135168, 1, 1)
    assert f(_plan("x3", 300, 300, 128, streamk=0, **X3)) == ("x3_wide", 4, 1, 512, 4, 512, 135168, 1, 1)
    assert f(_plan("x3", 4100, 2048, 256, streamk=0, n_cu=100, **X3)) == ("x3_wide", 4, 1, 2048, 100, 512, 135168, 1, 1)
    assert f(_plan("x3a", 641, 3900, 64, **X3)) == ("small_x3", 0, 0, 3904, 671, 512, 49152, 0, 0)
    # the wide epilogue kinds (the kernels' compile-time variants)
    assert _plan("bf16", 4096, 2048, 64, has=("bias", "out_t"), mode=1).variant == 1
    assert _plan("bf16", 4096, 2048, 64, has=("bias", "resid", "out_f32")).variant == 2
    assert _plan("bf16", 4096, 2048, 64, has=("bias", "bias_on_rows", "out_t"), col_div=442, col_pad=448).variant == 3
    assert _plan("x3", 64, 64, 64, has=("bias", "resid", "out_f32")).variant == 2
    assert _plan("x3", 64, 64, 64, has=("bias", "bias_on_rows", "out_f32"), col_div=442, col_pad=448).variant == 5
    assert _plan("x3", 64, 64, 64, has=("bias", "out_t", "out_lo"), mode=1).variant == 6
    assert _plan("x3", 64, 64, 64, has=("bias", "out_t", "out_lo")).variant == 7
    # more workgroups than stamp rows: a generic launch of 8193 tiles records no stamps
    assert _plan("bf16", 1, 8192 * 128, 64, has=("out_f32",)).keeps_stamps == 1
    assert _plan("bf16", 1, 8193 * 128, 64, has=("out_f32",)).keeps_stamps == 0


def test_gemm_plan_text_side_forms():
    """gemm_nt_small_x3_kernel: more than 600 workgroups and K <= 1024 -> 32-deep slabs on a three-slot 48 KB ring (variant 0);
    else 64-deep slabs when K % 64 == 0 (1, 128 KB), 32-deep otherwise (2, 64 KB)."""
    f = lambda M, N, K: (lambda p: (p.name, p.variant, p.grid, p.smem))(_plan("x3a", M, N, K, **X3))
    assert f(640, 3840, 1024) == ("small_x3", 1, 600, 131072)              # 600 workgroups: not more than 600
    assert f(640, 3844, 1024) == ("small_x3", 0, 610, 49152)
    assert f(640, 3844, 32) == ("small_x3", 0, 610, 49152)
    assert f(640, 3844, 1088) == ("small_x3", 1, 610, 131072)              # K > 1024
    assert f(640, 3844, 1056) == ("small_x3", 2, 610, 65536)
    assert f(64, 64, 64) == ("small_x3", 1, 1, 131072)
    assert f(64, 64, 96) == ("small_x3", 2, 1, 65536)
    assert _plan("x3a", 64, 64, 48, **X3).status == -22 and _plan("x3a", 64, 66, 64, **X3).status == -22


def test_gemm_plan_stream_k_split():
    """sk_full = rounds * CUs tiles are walked whole, the tail's K / 64 slab pairs are dealt sk_upw = ceil(tail * (K / 64) / CUs) per
    workgroup over a grid of all CUs.  5000 x 2304 is 20 x 9 = 180 tiles."""
    f = lambda p: (p.name, p.grid, p.sk_full, p.sk_upw)
    sk = lambda **kw: f(_plan("x3", 5000, 2304, 1024, **X3, **kw))
    assert sk(streamk=2, n_cu=64) == ("x3_wide", 64, 128, 13)             # 2 rounds, tail 52: ceil(52 * 16 / 64)
    assert sk(streamk=2, n_cu=256) == ("x3_wide", 256, 0, 12)             # no whole round, tail 180: ceil(180 * 16 / 256)
    assert sk(streamk=0, n_cu=64) == ("x3_wide", 64, 0, 0)
    assert sk(streamk=2, n_cu=64, sk_wgs=63) == ("x3_wide", 64, 0, 0)     # workspace smaller than the grid
    assert sk(streamk=2, n_cu=64, sk_wgs=0) == ("x3_wide", 64, 0, 0)
    assert sk(streamk=2, n_cu=60) == ("x3_wide", 60, 0, 0)                # 180 = 3 x 60: no tail
    assert sk(streamk=2, n_cu=256, sk_wgs=256) == sk(streamk=2, n_cu=256)
    # the cost model (mode 1) on the two launches csrc/gemm.hip names: a small tail of deep tiles pays (8 x 2305 rows, fc2: 292
    # tiles of K = 4096 -> tail 36, 9 pairs each), the bench batch's 732 tiles of K = 1024 do not
    assert f(_plan("x3", 8 * 2305, 1024, 4096, streamk=1, n_cu=256, **X3)) == ("x3_wide", 256, 256, 9)
    assert f(_plan("x3", 15470, 3072, 1024, streamk=1, n_cu=256, **X3)) == ("x3_wide", 256, 0, 0)
    # only the split-bf16 wide kernel has the tail: the bf16 wide kernel of the same shape keeps whole tiles
    assert f(_plan("bf16", 5000, 2304 * 4, 1024, streamk=2, n_cu=64, **WIDE)) == ("wide", 64, 0, 0)


def test_gemm_plan_refusals():
    """The checks of gemm_nt, in front of any launch: PNP_ERR_ARG = -22 and an empty plan."""
    bad = lambda *a, **kw: (lambda p: (p.status, p.name, p.grid))(_plan(*a, **kw)) == (-22, None, 0)
    assert bad("f32", 0, 64, 64, **BOTH) and bad("f32", 8, 0, 64, **BOTH) and bad("f32", 8, 64, 0, **BOTH)
    assert bad("f32", 8, 64, 48, **BOTH) and bad("bf16", 8, 64, 32, **BOTH) and bad("x3", 8, 64, 32, **X3)
    assert bad("f32", 8, 64, 64, lda=66, **BOTH) and bad("bf16", 8, 64, 64, ldb=68, **BOTH)
    for N in (65, 66, 67):                                               # four-column reads past column N
        assert bad("bf16", 8, N, 64, has=("bias", "out_f32")) and bad("f32", 8, N, 64, has=("resid", "out_f32"))
        assert bad("f32", 8, N, 64, has=("aux", "out_f32"), mode=1)
        assert _plan("f32", 8, N, 64, has=("bias", "bias_on_rows", "out_f32")).name == "g64"
    # a split launch whose epilogue is not one of the wide kinds: dual output, a GELU without the pair, token pairs with an odd N
    assert bad("x3", 64, 64, 64, has=("bias", "out_f32", "out_t")) and bad("x3", 64, 64, 64, has=("bias", "out_f32"), mode=1)
    assert bad("x3", 64, 63, 64, has=("bias", "bias_on_rows", "out_f32"), col_div=442, col_pad=448)
    assert bad("x3", 64, 63, 64, has=("bias", "bias_on_rows", "out_f32"))
    assert bad("x3", 64, 66, 64, **X3) and bad("x3", 64, 64, 64, has=("bias", "out_f32", "aux"))
    assert _plan("bf16", 255, 128 * 256 + 37, 64, has=("bias", "bias_on_rows", "out_t"), col_div=442, col_pad=448).name == "g128"
