"""GPU: every dispatch branch of csrc/gemm.hip gemm_nt launched alone through a pnp_op_gemm* entry point and compared element
by element with float64 (tests/_gemm_refs.py), with both input families:

  exact : integer operands, every partial sum below 2^24 -- zero difference demanded on every linear epilogue (fp32 output ==
          ref, bf16 output == bf16(ref), split output == split(ref)); any indexing / slab / tile-ownership / stream-K error fails;
  random: N(0, 1) with outlier channels -- the GELU / GELU' epilogues and the rounding, against the project's bounds scaled
          by the row-norm product.

Common to every case: operands sit in buffers with leading dimensions larger than their width whose pad columns (and the
elements behind the last row, the bias and the residual) hold NaN; every output and stash is a NaN-filled Guarded2D whose pad
columns, skipped rows, columns past N and guard blocks must keep their sentinel bit for bit.  The branch a shape lands on is
part of the test id and is asserted against the library's own launch plan (pnp_op_gemm_plan, the function gemm_nt launches from).
Run on the MI355X box:  python -m pytest tests/test_gemm_ops_gpu.py -m gpu -x -q
"""
import pytest

torch = pytest.importorskip("torch")

import _gemm_refs as R          # noqa: E402
from _gpu_guard import Acc, Guarded2D, _bits, nan_after, padded          # noqa: E402

pytestmark = pytest.mark.gpu

ERR_ARG = -22
DEV = "cuda"


@pytest.fixture()
def lib():
    from pnp_ovss import hip
    lib = hip.load_library()
    yield lib
    assert lib.pnp_set_tuning(b"streamk", 1) == 0


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _ceil4(n):
    return (n + 3) // 4 * 4


def E(bias=None, resid=False, mode=0, aux=False, out="f32", row_div=0, col=None, role="A"):
    """An epilogue: bias None | "col" | "row"; resid (pos_embed when row_div); mode 0 linear | 1 GELU | 2 GELU'; aux: the stash of
    mode 1 (mode 2 always reads one); out "f32" | "t" (compute type) | "both" | "split" (split-bf16 pair); col = (col_div,
    col_pad); role: which operand carries the 11-bit values of the exact split family."""
    return dict(bias=bias, resid=resid, mode=mode, aux=aux, out=out, row_div=row_div, col=col, role=role)


def _plan(form, M, N, K, e, **kw):
    """The library's launch plan (pnp_ovss.hip.gemm_plan) of run_case's launch of epilogue `e`: the operands and outputs
    run_case hands the entry point, as presence bits."""
    from pnp_ovss import hip
    has = {"bias": bool(e["bias"]), "bias_on_rows": e["bias"] == "row", "resid": e["resid"],
           "out_f32": form == "x3a" or e["out"] in ("f32", "both"), "out_t": form != "x3a" and e["out"] in ("t", "both", "split"),
           "out_lo": e["out"] == "split", "aux": (e["mode"] == 1 and e["aux"]) or e["mode"] == 2}
    div, pad = e["col"] or (0, 0)
    return hip.gemm_plan(form, M, N, K, has=[h for h, on in has.items() if on], mode=e["mode"], row_div=e["row_div"], col_div=div,
                         col_pad=pad, lda=K + 16, ldb=K + 16, **kw)


def _accepts(form, e, N):
    """Does the form take this epilogue at this N (include/pnp_hip.h)."""
    needs4 = e["bias"] == "col" or e["resid"] or e["aux"] or e["mode"] == 2
    if form in ("f32", "bf16"):
        return not (N % 4 and needs4)
    if form == "x3a":
        return N % 4 == 0
    if e["col"] or e["bias"] == "row":
        div = e["col"][0] if e["col"] else 0
        return bool(div & 1) or N % 2 == 0
    return N % 4 == 0


def run_case(lib, acc, form, M, N, K, e, family, seed, branch=None):
    """One launch, every output element compared.  Returns the (M, N) fp32-facing result (CPU, float64) for callers that
    compare launches with each other."""
    case = f"{form} {family} M={M} N={N} K={K} " + " ".join(f"{k}={v}" for k, v in e.items() if v not in (None, False, 0))
    if branch is not None:
        assert _plan(form, M, N, K, e).name == branch, (case, "lands on another kernel than the id says")
    split = form in ("x3", "x3a")
    bf16 = form == "bf16"
    exact = family == "exact"
    # ---- operands
    if exact:
        A, B = R.exact_operands(M, N, K, seed, split=e["role"] if split else None, device=DEV)
    else:
        A, B = R.random_operands(M, N, K, seed, b_scale=0.25 if split else 1.0, device=DEV, bf16=bf16)
    gen = torch.Generator(device=DEV).manual_seed(seed + 1)
    nb = M if e["bias"] == "row" else N
    bias = None
    if e["bias"]:
        bias = R.exact_vector(nb, seed + 2, device=DEV) if exact else torch.randn(nb, generator=gen, device=DEV)
    rd = e["row_div"]
    res_rows = rd + 1 if rd else M
    resid = None
    if e["resid"]:
        resid = R.exact_vector((res_rows, N), seed + 3, device=DEV) if exact else torch.randn(res_rows, N, generator=gen, device=DEV)
    u = torch.randn(M, N, generator=gen, device=DEV) * 1.5 if e["mode"] == 2 else None
    if exact:
        assert e["mode"] == 0 or (e["mode"] == 1 and e["aux"]), "exact family: linear epilogues (and the linear stash) only"
        R.assert_exact_family(A, B, bias, resid, split=split)
    # ---- geometry: output row of m, output column of n
    m_idx = torch.arange(M, device=DEV)
    rmap = (m_idx // rd) * (rd + 1) + 1 + m_idx % rd if rd else m_idx
    out_rows = ((M + rd - 1) // rd) * (rd + 1) if rd else M
    n_idx = torch.arange(N, device=DEV)
    if e["col"]:
        div, pad = e["col"]
        cmap = (n_idx // div) * pad + n_idx % div
        out_cols = ((N + div - 1) // div) * pad
    else:
        div, pad, cmap, out_cols = 0, 0, n_idx, N
    written = torch.zeros(out_rows, out_cols, dtype=torch.bool, device=DEV)
    written[rmap[:, None], cmap[None, :]] = True
    ldo = _ceil4(out_cols) + 8
    # ---- reference
    lin = A.double() @ B.double().t()
    if bias is not None:
        lin = lin + (bias.double()[:, None] if e["bias"] == "row" else bias.double()[None, :])
    val = R.gelu64(lin) if e["mode"] == 1 else lin * R.gelu_grad64(u.double()) if e["mode"] == 2 else lin
    if resid is not None:
        val = val + (resid.double()[1 + m_idx % rd] if rd else resid.double())
    # ---- device buffers
    keep = []
    lda = K + 16
    tdt = torch.bfloat16 if (bf16 or split) else torch.float32

    def operand(x, dt):
        v, buf = padded(x, lda, dt)
        keep.append(buf)
        return v
    if form == "x3":
        (Ah, Al), (Bh, Bl) = R.split_pair(A), R.split_pair(B)
        dA, dAl, dB, dBl = (operand(x, torch.bfloat16) for x in (Ah, Al, Bh, Bl))
    elif form == "x3a":
        Bh, Bl = R.split_pair(B)
        dA, dB, dBl = operand(A, torch.float32), operand(Bh, torch.bfloat16), operand(Bl, torch.bfloat16)
    else:
        dA, dB = operand(A, tdt), operand(B, tdt)
    d_bias = d_res = None
    if bias is not None:
        d_bias, buf = nan_after(bias)
        keep.append(buf)
    ldr = _ceil4(N) + 4
    if resid is not None:
        d_res, buf = padded(resid, ldr)
        keep.append(buf)
    o32 = Guarded2D(out_rows, out_cols, ldo, torch.float32) if e["out"] in ("f32", "both") else None
    odt = torch.float32 if form in ("f32", "x3a") else torch.bfloat16
    ot = Guarded2D(out_rows, out_cols, ldo, odt) if e["out"] in ("t", "both", "split") else None
    olo = Guarded2D(out_rows, out_cols, ldo, torch.bfloat16) if e["out"] == "split" else None
    ld_aux = _ceil4(N) + 12
    aux = d_u = None
    if e["mode"] == 1 and e["aux"]:
        aux = Guarded2D(out_rows, N, ld_aux, torch.float32)
    if e["mode"] == 2:
        assert not rd
        d_u, buf = padded(u, ld_aux)
        keep.append(buf)
    aux_ptr = aux.ptr if aux is not None else _ptr(d_u)
    # ---- launch
    if form == "x3":
        rc = lib.pnp_op_gemm_x3(_ptr(dA), _ptr(dAl), lda, _ptr(dB), _ptr(dBl), lda, M, N, K, _ptr(d_bias), int(e["bias"] == "row"),
                                _ptr(d_res), ldr, o32.ptr if o32 else None, ldo, ot.ptr if ot else None, olo.ptr if olo else None,
                                ldo, e["mode"], div, pad, None)
    elif form == "x3a":
        rc = lib.pnp_op_gemm_x3a(_ptr(dA), lda, _ptr(dB), _ptr(dBl), lda, M, N, K, _ptr(d_bias), _ptr(d_res), ldr, o32.ptr, ldo,
                                 e["mode"], aux_ptr, ld_aux, None)
    else:
        rc = lib.pnp_op_gemm_args(int(bf16), _ptr(dA), lda, _ptr(dB), lda, M, N, K, _ptr(d_bias), int(e["bias"] == "row"),
                                  _ptr(d_res), ldr, o32.ptr if o32 else None, ldo, ot.ptr if ot else None, ldo, e["mode"],
                                  aux_ptr, ld_aux, rd, div, pad, None)
    assert rc == 0, (case, rc)
    torch.cuda.synchronize()
    # ---- compare
    val_c = val.cpu()
    rm, cm, wr = rmap.cpu(), cmap.cpu(), written.cpu()

    def mn(buf, tag, cols_map=cm, wmask=wr):
        got = buf.check(f"{case} {tag}", written=wmask)
        return got[rm][:, cols_map]

    def bounded(name, got, want, bound):
        err = (got.double() - want).abs()
        assert bool(torch.isfinite(got.float()).all()), (case, name, "NaN / inf in the output")
        b = bound if torch.is_tensor(bound) else torch.full_like(err, float(bound))
        i = int((err / b).argmax())
        acc.add(name, float(err.reshape(-1)[i]), float(b.reshape(-1)[i]), case)

    # exact family: the accumulator is the float64 value, so a linear epilogue leaves no error at all and GELU only its own
    # evaluation error (the stash in front of it stays exact)
    exact_out = exact and e["mode"] == 0
    lin_b = torch.zeros(M, N, dtype=torch.float64) if exact else (R.x3_bound(A, B) if split else R.accum_bound(A, B, bf16)).cpu()
    val_b = lin_b
    if e["mode"] == 1:
        val_b = R.gelu_bound(lin_b, lin.cpu())
    elif e["mode"] == 2:
        val_b = R.gelu_grad_bound(lin_b, lin.cpu())
    res = None
    if o32 is not None:
        res = mn(o32, "out_f32")
        if exact_out:
            assert torch.equal(res.double(), val_c), (case, "out_f32 != float64 reference", float((res.double() - val_c).abs().max()))
        else:
            bounded(f"{form}/out_f32/mode{e['mode']}", res, val_c, val_b)
    if ot is not None and e["out"] != "split":
        got = mn(ot, "out_t")
        want = val_c.float().to(odt)
        if exact_out:
            assert torch.equal(_bits(got.contiguous()), _bits(want.contiguous())), \
                (case, "out_t != one rounding of the reference", float((got.double() - val_c).abs().max()))
        elif odt == torch.float32:
            bounded(f"{form}/out_t_f32/mode{e['mode']}", got, val_c, val_b)
        else:
            bounded(f"{form}/out_t_bf16/mode{e['mode']}", got, val_c, R.bf16_out_bound(val_c))
        if res is not None:                                   # dual store: the compute-type copy is the fp32 one, rounded once
            assert torch.equal(_bits(got.contiguous()), _bits(res.to(odt).contiguous())), (case, "out_t != rounded out_f32")
        res = got if res is None else res
    if e["out"] == "split":
        hi, lo = mn(ot, "out_hi"), mn(olo, "out_lo")
        if exact_out:
            whi, wlo = R.split_pair(val_c.float())
            assert torch.equal(_bits(hi.contiguous()), _bits(whi)) and torch.equal(_bits(lo.contiguous()), _bits(wlo)), \
                (case, "pair != split(reference)")
            fits = val_c.abs() < 2 ** 16                      # 16 significant bits: the pair then IS the value
            assert torch.equal((hi.double() + lo.double())[fits], val_c[fits]), (case, "hi + lo != reference")
        else:
            bounded(f"{form}/out_pair/mode{e['mode']}", hi.double() + lo.double(), val_c, lin_b + 2.0 ** -16 * float(val_c.abs().max()))
            assert bool((lo.float().abs() <= 2.0 ** -8 * hi.float().abs() + 1e-30).all()), (case, "lo is not the remainder of hi")
        res = hi.double() + lo.double()
    if aux is not None:
        rows_w = torch.zeros(out_rows, N, dtype=torch.bool)
        rows_w[rm] = True
        got = aux.check(f"{case} aux", written=rows_w)[rm]
        if exact:
            assert torch.equal(got.double(), lin.cpu()), (case, "stash != pre-activation")
        else:
            bounded(f"{form}/aux_stash", got, lin.cpu(), lin_b)
    return res.double()


# ------------------------------------------------------------------------------------------ shapes of a branch
def _n0(M, tile, tiles):
    """Smallest N (a multiple of 128) at which an M-row problem has `tiles` tiles of `tile`."""
    per = (M + tile - 1) // tile
    return (tiles + per - 1) // per * tile


def _shapes(Ms, n_of_m, Ks):
    """Every (M, N) with K cycling through Ks, plus every K at the first ragged (M, N)."""
    out, seen = [], set()
    for i, M in enumerate(Ms):
        for j, N in enumerate(n_of_m(M)):
            out.append((M, N, Ks[(i + j) % len(Ks)]))
    M, N = Ms[2], n_of_m(Ms[2])[-1]
    out += [(M, N, K) for K in Ks]
    return [s for s in out if not (s in seen or seen.add(s))]


LINEAR = [E(), E(bias="row", out="t"), E(bias="col", resid=True), E(bias="col", out="both"), E(bias="col", mode=1, aux=True)]
NONLIN = [E(bias="col", mode=1, aux=True, resid=True), E(bias="col", mode=1, out="t"), E(bias="col", mode=2, resid=True),
          E(bias="row", out="both")]


def _sweep(lib, acc, form, branch, shapes, linear, nonlin, random_every=2):
    """Every epilogue the form accepts at each shape -- and that lands on `branch` there (an N % 4 != 0 launch of a row-major
    wide epilogue, say, belongs to the generic kernels' sweep) -- with the exact family; the random family on every linear
    epilogue and the non-linear ones at every `random_every`-th shape (a deliberate subsample: on a linear epilogue the exact
    family is the stronger check, the random one adds the rounding of non-integer data)."""
    n = 0
    lands = lambda e, M, N, K: _accepts(form, e, N) and _plan(form, M, N, K, e).name == branch
    for i, (M, N, K) in enumerate(shapes):
        for e in linear:
            if lands(e, M, N, K):
                run_case(lib, acc, form, M, N, K, e, "exact", seed=1000 * i + M + N + K, branch=branch)
                n += 1
        if i % random_every == 0:
            for e in linear + nonlin:
                if lands(e, M, N, K):
                    run_case(lib, acc, form, M, N, K, e, "random", seed=7000 * i + M + N + K, branch=branch)
                    n += 1
    R.measure(f"{acc.tag}/launches", n)
    assert n >= len(shapes)


@pytest.mark.parametrize("form", ["f32", "bf16"])
def test_branch_generic_64x64(lib, form):
    """gemm_nt_big_kernel<T, 64, 64, 32, 32, 3> (fewer than 192 tiles of 128): M in {63, 64, 65, 1}, N on and off the 64-column tile with
    N % 4 in {0, 1, 2, 3}, K = one slab (the smallest the type accepts), two and sixteen."""
    bk = 64 if form == "bf16" else 32
    acc = Acc(f"gpu/gemm/g64/{form}")
    try:
        _sweep(lib, acc, form, "g64", _shapes((63, 64, 65, 1), lambda M: (64, 65, 66, 67, 100, 132), (bk, 2 * bk, 16 * bk)),
               LINEAR, NONLIN)
    finally:
        acc.flush()


@pytest.mark.parametrize("form", ["f32", "bf16"])
def test_branch_generic_128x128(lib, form):
    """gemm_nt_big_kernel<T, 128, 128, 64, 64, 2> (192 tiles of 128 or more, bf16: K < 2048): ragged row tile, ragged column tile and
    the partial-fragment store (n + 3 >= N) against the reference."""
    bk = 64 if form == "bf16" else 32
    acc = Acc(f"gpu/gemm/g128/{form}")
    try:
        ns = lambda M: tuple(_n0(M, 128, 192) + d for d in (0, 1, 2, 3, 36))
        _sweep(lib, acc, form, "g128", _shapes((127, 128, 129, 1), ns, (bk, 2 * bk, 8 * bk)), LINEAR, NONLIN, random_every=3)
    finally:
        acc.flush()


def test_branch_generic_256x256_bf16(lib):
    """gemm_nt_big_kernel<bf16, 256, 256, 128, 64, 2, false> (K >= 2048, N >= 512, 192 tiles of 128 or more and fewer than 128 tiles of
    256, or an epilogue the wide kernel does not have): ViT-L fc2 in bf16 mode at 7..17 images.  Also on a large problem (136
    tiles of 256) through the dual output and the GELU stash."""
    acc = Acc("gpu/gemm/g256/bf16")
    try:
        ns = lambda M: tuple(_n0(M, 128, 192) + d for d in ((0, 3, 36) if M > 1 else (0, 1, 2)))
        shapes = [(M, N, 2048 if M != 257 else K) for M in (255, 256, 257, 1) for N in ns(M) for K in ((2048, 2112, 4096) if M == 257 else (2048,))]
        shapes = sorted(set(shapes))
        for M, N, K in shapes:
            assert ((M + 255) // 256) * ((N + 255) // 256) < 128
        _sweep(lib, acc, "bf16", "g256", shapes, LINEAR[:4], NONLIN[:3], random_every=4)
        for i, e in enumerate((E(bias="col", out="both"), E(bias="col", mode=1, aux=True, out="t"))):
            run_case(lib, acc, "bf16", 4100, 2048, 2048, e, "exact", seed=40 + i, branch="g256")
        run_case(lib, acc, "bf16", 4100, 2048, 2048, E(bias="col", mode=1, aux=True, out="t"), "random", seed=43, branch="g256")
    finally:
        acc.flush()


WIDE_LINEAR = [E(bias="col", out="t"), E(bias="col", resid=True), E(bias="row", out="t", col=(442, 448)), E(bias="row", out="t", col=(577, 640)),
               E(out="t")]
WIDE_NONLIN = [E(bias="col", mode=1, out="t")]


def test_branch_wide_bf16(lib):
    """gemm_nt_wide_kernel<EPI> (a wide epilogue and 128 tiles of 256 or more), its four epilogues: + bias -> bf16, + bias GELU ->
    bf16, + bias + residual -> fp32, + row bias with token columns -> bf16 (even col_div: token pairs; odd: single tokens)."""
    acc = Acc("gpu/gemm/wide/bf16")
    try:
        ns = lambda M: tuple(_n0(M, 256, 128) + d for d in (0, 4, 36, 37, 38, 39))
        _sweep(lib, acc, "bf16", "wide", _shapes((255, 256, 257, 1), ns, (64, 128, 1024)), WIDE_LINEAR, WIDE_NONLIN, random_every=3)
    finally:
        acc.flush()


X3_LINEAR = [E(bias="col"), E(bias="col", resid=True), E(bias="col", out="split"), E(bias="row", col=(442, 448)), E(bias="row", col=(577, 640)),
             E(bias="col", role="B"), E(bias="col", out="split", role="B"), E(bias="row", col=(577, 640), role="B")]
X3_NONLIN = [E(bias="col", mode=1, out="split")]


@pytest.mark.parametrize("streamk", [0, 1, 2])
def test_branch_split_wide(lib, streamk):
    """gemm_nt_x3_kernel<EPI, SK>, five epilogues (+ bias -> fp32, + bias + residual -> fp32, + bias -> pair, + bias GELU -> pair,
    token columns -> fp32) with the stream-K tail off, chosen by the cost model, and forced: a forced tail cuts even a one-tile
    problem along K, so every fix-up path (partial tiles summed by the owner) is held to zero difference.  Both cross terms:
    the 11-bit operand is A (A_lo.B_hi carries the result) and then B (A_hi.B_lo)."""
    assert lib.pnp_set_tuning(b"streamk", streamk) == 0
    acc = Acc(f"gpu/gemm/x3_wide/streamk{streamk}")
    try:
        ns = lambda M: (256, 260, 300, 516, 577 + 66, 1154 + 31, 442 * 3, 442 + 100)
        _sweep(lib, acc, "x3", "x3_wide", _shapes((255, 256, 257, 1), ns, (64, 128, 1024)), X3_LINEAR, X3_NONLIN, random_every=3)
        # many tiles and a tail round: 4100 x 2048 is 136 tiles (no whole round on 256 CUs), 5000 x 2304 x 1024 is 180
        for i, (M, N, K) in enumerate(((4100, 2048, 256), (5000, 2304, 1024))):
            for e in (E(bias="col", resid=True), E(bias="col", out="split", role="B"), E(bias="row", col=(442, 448))):
                run_case(lib, acc, "x3", M, N, K, e, "exact", seed=90 + i, branch="x3_wide")
        from pnp_ovss import hip
        launches, gave_up = hip.streamk_status_ops()
        assert gave_up == 0, gave_up
        R.measure(f"{acc.tag}/streamk_launches_so_far", launches)
    finally:
        acc.flush()


X3A_LINEAR = [E(), E(bias="col", resid=True), E(bias="col", mode=1, aux=True), E(bias="col", resid=True, role="B")]
X3A_NONLIN = [E(bias="col", mode=1, aux=True, resid=True), E(bias="col", mode=1), E(bias="col", mode=2, resid=True)]


def test_branch_split_small(lib):
    """gemm_nt_small_x3_kernel (fp32 activations split by the kernel, weight pair): 64-deep slabs (K % 64 == 0), 32-deep slabs
    (K = 32, 96) and, past 600 tiles at K <= 1024, the three-slot 32-deep variant; modes 0, 1 (+ stash), 2."""
    acc = Acc("gpu/gemm/small_x3")
    try:
        _sweep(lib, acc, "x3a", "small_x3", _shapes((63, 64, 65, 1), lambda M: (64, 68, 100, 132), (32, 64, 96, 768)), X3A_LINEAR, X3A_NONLIN)
        for K in (32, 64, 1024):                               # 11 x 61 = 671 tiles
            run_case(lib, acc, "x3a", 641, 3900, K, E(bias="col", resid=True), "exact", seed=K, branch="small_x3")
        run_case(lib, acc, "x3a", 641, 3900, 96, E(bias="col", mode=1, aux=True), "random", seed=5, branch="small_x3")
    finally:
        acc.flush()


# ------------------------------------------------------------------------------------------ dispatch boundaries
BOUNDARIES = [
    # id, form, epilogue, (M, N, K, branch) just below the threshold, the same just at / above it
    ("tiles128_191_192-f32", "f32", E(bias="row"), (100, 191 * 128, 64, "g64"), (100, 191 * 128 + 1, 64, "g128")),
    ("tiles128_191_192-bf16", "bf16", E(bias="row", out="both"), (100, 191 * 128, 128, "g64"), (100, 191 * 128 + 1, 128, "g128")),
    ("tiles256_127_128", "bf16", E(bias="col", out="t"), (200, 127 * 256, 64, "g128"), (200, 127 * 256 + 4, 64, "wide")),
    ("K_1984_2048", "bf16", E(bias="col", out="both"), (257, 8192, 1984, "g128"), (257, 8192, 2048, "g256")),
    ("N_508_512", "bf16", E(bias="col", out="both"), (6144, 508, 2048, "g128"), (6144, 512, 2048, "g256")),
    ("tiles256_127_128-K2048", "bf16", E(bias="col", resid=True), (200, 127 * 256, 2048, "g256"), (200, 127 * 256 + 4, 2048, "wide")),
]


@pytest.mark.parametrize("name,form,e,below,above", BOUNDARIES, ids=[b[0] for b in BOUNDARIES])
def test_dispatch_boundary(lib, name, form, e, below, above):
    """One step either side of each threshold of gemm_nt (tiles of 128 < 192, tiles of 256 >= 128, K >= 2048, N >= 512): both
    sides, exact family, zero difference."""
    acc = Acc(f"gpu/gemm/boundary/{name}")
    try:
        for M, N, K, branch in (below, above):
            run_case(lib, acc, form, M, N, K, e, "exact", seed=M + N + K, branch=branch)
            run_case(lib, acc, form, M, N, K, e, "random", seed=M + N + K + 1, branch=branch)
    finally:
        acc.flush()


# ------------------------------------------------------------------------------------------ hidden epilogues (pnp_op_gemm_args)
HIDDEN_SHAPES = {          # branch -> (M, N, K) with M a whole number of row_div-row images where row_div is used
    "g64": dict(row=(25, 3, 132), tok_m=65, k=(64, 192)),
    "g128": dict(row=(441, 13, 640), tok_m=1536, k=(64, 192)),
}


@pytest.mark.parametrize("form", ["f32", "bf16"])
@pytest.mark.parametrize("branch", ["g64", "g128"])
def test_hidden_epilogues_generic(lib, branch, form):
    """The epilogues the engine uses that no other entry point reaches: the patch-embed row remap with pos_embed as residual
    (token row 0 of every image keeps its sentinel), the GELU stash (aux compared as well as the output), GELU' reading aux, the
    dual fp32 + compute-type store; and the token-column geometry (bias_on_rows + col_div even 442/448, odd 577/640, and
    col_div = 3 < 4: every fragment straddles an image) with a partial last image -- pad columns and columns past N keep the
    sentinel."""
    acc = Acc(f"gpu/gemm/hidden/{branch}/{form}")
    sh = HIDDEN_SHAPES[branch]
    try:
        rd, nimg, N = sh["row"]
        for K in sh["k"]:
            for fam in ("exact", "random"):
                run_case(lib, acc, form, rd * nimg, N, K, E(bias="col", resid=True, row_div=rd), fam, seed=K + 1, branch=branch)
                run_case(lib, acc, form, rd * nimg, N, K, E(bias="col", resid=True, row_div=rd, out="both"), fam, seed=K + 2, branch=branch)
                run_case(lib, acc, form, rd * nimg, N, K, E(bias="col", mode=1, aux=True, out="t"), fam, seed=K + 3, branch=branch)
                run_case(lib, acc, form, rd * nimg, N, K, E(bias="col", out="both"), fam, seed=K + 4, branch=branch)
            run_case(lib, acc, form, rd * nimg, N, K, E(bias="col", mode=2, out="t"), "random", seed=K + 5, branch=branch)
            run_case(lib, acc, form, rd * nimg, N, K, E(bias="col", mode=2, resid=True, out="both"), "random", seed=K + 6, branch=branch)
        M = sh["tok_m"]
        big = branch == "g128"
        for div, pad, N in ((442, 448, 4 * 442 + 200 if big else 2 * 442 + 100), (577, 640, 3 * 577 + 300 if big else 577 + 301),
                            (3, 4, 2031 if big else 302), (442, 448, 4 * 442 + 201 if big else 2 * 442 + 101)):
            for out in ("t", "f32", "both"):
                for fam in ("exact", "random"):
                    run_case(lib, acc, form, M, N, 128, E(bias="row", col=(div, pad), out=out), fam, seed=div + N, branch=branch)
    finally:
        acc.flush()


def test_token_pairs_need_an_even_n(lib):
    """The wide token-column epilogues store token PAIRS when col_div is even.  With an odd N the last pair would write column N:
    the bf16 form then runs on the generic kernel (column N keeps its sentinel), the split form is refused."""
    acc = Acc("gpu/gemm/wide/odd_n_even_col_div")
    try:
        N = 128 * 256 + 37                                     # 129 tiles of 256; 74 images of 442 and a partial one, odd
        for M in (255, 257):
            run_case(lib, acc, "bf16", M, N, 64, E(bias="row", out="t", col=(442, 448)), "exact", seed=M, branch="g128")
            run_case(lib, acc, "bf16", M, N - 1, 64, E(bias="row", out="t", col=(442, 448)), "exact", seed=M, branch="wide")
    finally:
        acc.flush()
    t = torch.zeros(64 * 80, dtype=torch.bfloat16, device=DEV)
    o = Guarded2D(64, 448, 456, torch.float32)
    p = t.data_ptr()
    assert lib.pnp_op_gemm_x3(p, p, 80, p, p, 80, 64, 63, 64, None, 1, None, 0, o.ptr, 456, None, None, 0, 0, 442, 448, None) == ERR_ARG
    assert lib.pnp_op_gemm_x3(p, p, 80, p, p, 80, 64, 63, 64, None, 1, None, 0, o.ptr, 456, None, None, 0, 0, 0, 0, None) == ERR_ARG
    torch.cuda.synchronize()
    o.untouched("refused split token-column launch")


# ------------------------------------------------------------------------------------------ N % 4 != 0 with four-column reads
@pytest.mark.parametrize("form", ["f32", "bf16"])
def test_odd_n_with_column_operands_is_refused(lib, form):
    """store_frag reads a per-column bias, the residual row and the GELU stash four columns at a time (and writes the stash so):
    with N % 4 != 0 the last group reaches up to three elements past bias[N - 1], past the last residual row and -- the stash --
    WRITES past column N.  gemm_nt refuses the combination (include/pnp_hip.h); nothing is written.  The same N with a per-row
    bias and no residual runs, exactly (the sweeps above); here the refusals, on the 64- and the 128-tile shapes."""
    bf = int(form == "bf16")
    tdt = torch.bfloat16 if bf else torch.float32
    K, lda = 64, 80
    for M, N in ((65, 67), (129, 192 * 128 + 1), (129, 192 * 128 + 2)):
        A, ka = padded(torch.ones(M, K), lda, tdt)
        B, kb = padded(torch.ones(N, K), lda, tdt)
        bias, kc = nan_after(torch.ones(N))
        ldr = _ceil4(N) + 4
        resid, kr = padded(torch.ones(M, N), ldr)
        ldo = _ceil4(N) + 8
        out = Guarded2D(M, N, ldo, torch.float32)
        aux = Guarded2D(M, N, ldo, torch.float32)
        a = lambda **kw: lib.pnp_op_gemm_args(bf, A.data_ptr(), lda, B.data_ptr(), lda, M, N, K, kw.get("bias"), kw.get("rows", 0),
                                              kw.get("resid"), ldr, out.ptr, ldo, None, 0, kw.get("mode", 0), kw.get("aux"), ldo, 0, 0, 0,
                                              None)
        assert a(bias=bias.data_ptr()) == ERR_ARG
        assert a(resid=resid.data_ptr()) == ERR_ARG
        assert a(mode=1, aux=aux.ptr) == ERR_ARG
        assert a(mode=2, aux=aux.ptr) == ERR_ARG
        assert lib.pnp_op_gemm(bf, A.data_ptr(), lda, B.data_ptr(), lda, M, N, K, bias.data_ptr(), None, 0, out.ptr, ldo, 0, None) == ERR_ARG
        assert lib.pnp_op_gemm_ex(bf, A.data_ptr(), lda, B.data_ptr(), lda, M, N, K, None, resid.data_ptr(), ldr, out.ptr, ldo, None, 0,
                                  0, None) == ERR_ARG
        torch.cuda.synchronize()
        out.untouched(f"{form} M={M} N={N} out")
        aux.untouched(f"{form} M={M} N={N} aux")
        rowb, kd = nan_after(torch.full((M,), 3.0))           # the accepted form of the same shape
        assert a(bias=rowb.data_ptr(), rows=1) == 0
        torch.cuda.synchronize()
        got = out.check(f"{form} M={M} N={N} row bias")
        assert torch.equal(got, torch.full((M, N), float(K + 3))), (form, M, N)


def test_gemm_args_refuses_bad_arguments(lib):
    t = torch.zeros(4096, device=DEV)
    p = t.data_ptr()
    ok = dict(A=p, lda=64, B=p, ldb=64, M=8, N=16, K=32, bias=None, rows=0, resid=None, ldr=16, o32=p, ldo=16, ot=None, ldo_t=16,
              mode=0, aux=None, ld_aux=16, row_div=0, col_div=0, col_pad=0)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.pnp_op_gemm_args(0, a["A"], a["lda"], a["B"], a["ldb"], a["M"], a["N"], a["K"], a["bias"], a["rows"], a["resid"],
                                    a["ldr"], a["o32"], a["ldo"], a["ot"], a["ldo_t"], a["mode"], a["aux"], a["ld_aux"], a["row_div"],
                                    a["col_div"], a["col_pad"], None)
    assert call() == 0
    for bad in (dict(A=None), dict(B=None), dict(o32=None), dict(M=0), dict(N=-1), dict(K=0), dict(lda=16), dict(mode=3), dict(mode=-1),
                dict(mode=2), dict(col_div=8, col_pad=4), dict(col_div=-1), dict(row_div=-1), dict(K=48), dict(lda=66)):
        assert call(**bad) == ERR_ARG, bad
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ in-kernel clock stamps
def test_gemm_stamps_time_the_shipped_kernels(lib):
    """pnp_set_tuning("gemm_stamps", 1) / pnp_dbg_gemm_stamps on the three stamped kernel families at their smallest launches:
    fp32 generic (four 64 x 64 workgroups), split-bf16 wide with the stream-K tail off (four tiles, one ragged row tile) and
    bf16 wide at the dispatcher's threshold of 128 tiles.  Stamps change no output bit; every launched workgroup (grid =
    min(tiles, CUs)) leaves a start (slot 0) and an end (slot 3) on the shader clock and on the wall clock (slots 4, 7), written
    by THIS launch (its row differs from what the buffer held before); with the switch off again a launch leaves the rows alone."""
    import numpy as np
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    gen = torch.Generator(device=DEV).manual_seed(11)
    rnd = lambda *s: torch.randn(*s, generator=gen, device=DEV)

    def fp32_generic():
        M, N, K = 96, 128, 64
        A, B, bias = rnd(M, K), rnd(N, K), rnd(N)
        run = lambda out: lib.pnp_op_gemm(0, _ptr(A), K, _ptr(B), K, M, N, K, _ptr(bias), None, 0, _ptr(out), N, 0, None)
        return run, (M, N, torch.float32), 4, ("g64", _plan("f32", M, N, K, E(bias="col"), n_cu=cus, streamk=0))

    def split_wide():
        M, N, K = 300, 512, 128
        (Ah, Al), (Bh, Bl), bias = R.split_pair(rnd(M, K)), R.split_pair(rnd(N, K) * 0.25), rnd(N)
        run = lambda out: lib.pnp_op_gemm_x3(_ptr(Ah), _ptr(Al), K, _ptr(Bh), _ptr(Bl), K, M, N, K, _ptr(bias), 0, None, 0, _ptr(out), N,
                                             None, None, 0, 0, 0, 0, None)
        return run, (M, N, torch.float32), 4, ("x3_wide", _plan("x3", M, N, K, E(bias="col"), n_cu=cus, streamk=0))

    def bf16_wide():
        M, N, K = 4096, 2048, 64
        A, B, bias = rnd(M, K).bfloat16(), rnd(N, K).bfloat16(), rnd(N)
        run = lambda out: lib.pnp_op_gemm_ex(1, _ptr(A), K, _ptr(B), K, M, N, K, _ptr(bias), None, 0, None, 0, _ptr(out), N, 0, None)
        return run, (M, N, torch.bfloat16), 128, ("wide", _plan("bf16", M, N, K, E(bias="col", out="t"), n_cu=cus, streamk=0))

    def launch(run, shape):
        out = torch.zeros(shape[0], shape[1], dtype=shape[2], device=DEV)
        assert run(out) == 0
        torch.cuda.synchronize()
        return _bits(out).cpu()

    def stamps(rows):
        st = np.zeros((rows, 8), dtype=np.uint64)
        assert lib.pnp_dbg_gemm_stamps(st.ctypes.data, rows) == 0
        return st

    try:
        assert lib.pnp_set_tuning(b"streamk", 0) == 0
        for case in (fp32_generic, split_wide, bf16_wide):
            name = case.__name__
            run, shape, tiles, (branch, plan) = case()
            assert plan.name == branch, (name, "lands on another kernel")
            grid = min(tiles, cus)
            assert plan.grid == grid and plan.keeps_stamps == 1, (name, plan.grid, grid)
            off = launch(run, shape)
            assert bool(off.ne(0).any()), name
            assert lib.pnp_set_tuning(b"gemm_stamps", 1) == 0
            before = stamps(grid + 8)
            on = launch(run, shape)
            assert torch.equal(off, on), (name, "stamps changed the output")
            st = stamps(grid + 8)
            print(f"{name}: grid {grid}, shader clocks start..end min {int((st[:grid, 3] - st[:grid, 0]).min())} "
                  f"max {int((st[:grid, 3] - st[:grid, 0]).max())}, wall ticks max {int((st[:grid, 7] - st[:grid, 4]).max())}")
            for a, b in ((0, 3), (4, 7)):
                assert (st[:grid, a] != 0).all() and (st[:grid, b] != 0).all(), (name, a, b)
                assert (st[:grid, a] <= st[:grid, b]).all(), (name, a, b)
            assert (st[:grid] != before[:grid]).any(axis=1).all(), (name, "a launched workgroup left no stamps")
            assert (st[grid:] == before[grid:]).all(), (name, "rows past the grid were written")
            assert int((st != before).any(axis=1).sum()) == plan.grid, (name, "stamp rows written != the plan's grid")
            assert lib.pnp_set_tuning(b"gemm_stamps", 0) == 0
            assert torch.equal(off, launch(run, shape)), name
            assert (stamps(grid + 8) == st).all(), (name, "a launch with stamps off wrote stamps")
    finally:
        assert lib.pnp_set_tuning(b"gemm_stamps", 0) == 0
        assert lib.pnp_set_tuning(b"streamk", 1) == 0


def test_gemm_stamps_skip_launches_with_more_workgroups_than_rows(lib):
    """The stamp buffer has 8192 rows and the generic kernels launch one workgroup per tile: a launch of 8192 tiles of 128 stamps
    every row up to the last, a launch of 8193 records nothing (it is handed no buffer: no write behind row 8191) and computes
    the same output as with stamps off."""
    import numpy as np
    rows, K = 8192, 64
    gen = torch.Generator(device=DEV).manual_seed(12)
    A = torch.randn(1, K, generator=gen, device=DEV).bfloat16()
    B = torch.randn((rows + 1) * 128, K, generator=gen, device=DEV).bfloat16()

    def launch(tiles):
        N = tiles * 128
        plan = _plan("bf16", 1, N, K, E())
        assert plan.name == "g128" and plan.grid == tiles and plan.keeps_stamps == int(tiles <= rows)
        out = torch.zeros(1, N, device=DEV)
        assert lib.pnp_op_gemm(1, _ptr(A), K, _ptr(B), K, 1, N, K, None, None, 0, _ptr(out), N, 0, None) == 0
        torch.cuda.synchronize()
        return _bits(out).cpu()

    def stamps():
        st = np.zeros((rows, 8), dtype=np.uint64)
        assert lib.pnp_dbg_gemm_stamps(st.ctypes.data, rows) == 0
        return st

    try:
        off = launch(rows + 1)
        assert lib.pnp_set_tuning(b"gemm_stamps", 1) == 0
        before = stamps()
        assert torch.equal(launch(rows), off[:, :rows * 128])
        full = stamps()
        assert (full != before).any(axis=1).all(), "a launch of exactly 8192 workgroups stamps every row"
        assert (full[:, 0] != 0).all() and (full[:, 0] <= full[:, 3]).all()
        assert torch.equal(launch(rows + 1), off), "stamps changed the output"
        assert (stamps() == full).all(), "a launch of 8193 workgroups wrote stamps"
    finally:
        assert lib.pnp_set_tuning(b"gemm_stamps", 0) == 0
