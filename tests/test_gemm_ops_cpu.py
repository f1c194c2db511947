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


def test_dispatch_mirror_matches_the_documented_thresholds():
    assert R.gemm_branch("f32", 100, 191 * 128, 64, False) == "g64" and R.gemm_branch("f32", 100, 191 * 128 + 1, 64, False) == "g128"
    assert R.gemm_branch("bf16", 200, 127 * 256, 64, True) == "g128" and R.gemm_branch("bf16", 200, 127 * 256 + 4, 64, True) == "wide"
    assert R.gemm_branch("bf16", 257, 8192, 1984, False) == "g128" and R.gemm_branch("bf16", 257, 8192, 2048, False) == "g256"
    assert R.gemm_branch("bf16", 6144, 508, 2048, False) == "g128" and R.gemm_branch("bf16", 6144, 512, 2048, False) == "g256"
    assert R.gemm_branch("f32", 6144, 512, 2048, False) == "g128"
    assert math.isclose(R.GELU_SLOPE, 1.13)
