"""GPU: every text-stack kernel (and the two ViT input kernels) launched alone through its pnp_op_* entry point and compared
element by element with the float64 references of tests/_text_refs.py, at the launch forms the model runs never reach under a
reference-compared test: every workgroups-per-(head, image) split of the self-attention (forced with the "text_rows" tuning
key), the one- and two-launch fp32 backward, the long form through the stash and through the scratch.

Common to every case: each output (and the scratch the kernel writes) is NaN before the launch and sits between two guard
blocks of a sentinel value; afterwards the live region holds no NaN and the guards are untouched bit for bit.  Inputs the
kernel must not read hold NaN / out-of-range values.  Measured figures are printed and appended to PNP_TEST_MEASURE_LOG.
Run on the MI355X box:  python -m pytest tests/test_text_ops_gpu.py -m gpu -x -q
"""
import itertools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import _text_refs as R          # noqa: E402
from _gpu_guard import SENTINEL, Acc, Guarded, _bits          # noqa: E402,F401

pytestmark = pytest.mark.gpu

ERR_ARG = -22
POISON_I64 = 1 << 62             # in mask / id columns the kernels must not read


@pytest.fixture()
def lib():
    from pnp_ovss import hip
    lib = hip.load_library()
    yield lib
    assert lib.pnp_set_tuning(b"text_rows", 0) == 0


def _tdt(bf16):
    return torch.bfloat16 if bf16 else torch.float32


def _err(got, ref):
    return float((got.double() - ref.double()).abs().max()) if got.numel() else 0.0


def _mask_sets(B):
    if B == 1:
        return [(k,) for k in R.MASK_KINDS]
    return [("ones", "prefix", "token0"), ("hole", "zeros", "prefix")]


def _padded_i64(a, extra=3):
    """(B, L) int64 -> device (B, L + extra) whose extra columns hold a value no kernel may read."""
    B, L = a.shape
    p = torch.full((B, L + extra), POISON_I64, dtype=torch.int64)
    p[:, :L] = a
    return p.cuda(), L + extra


# ------------------------------------------------------------------------------------------ self-attention forward
def _run_fwd(lib, bf16, qkv, mask, heads, route, rows):
    """route: "stash" (d_probs given), "scratch" (d_probs NULL, d_scratch given), "none" (both NULL: L <= 192 only)."""
    B, L, _ = qkv.shape
    H = heads * R.HEAD
    tdt = _tdt(bf16)
    d_qkv = qkv.reshape(B * L, 3 * H).to(tdt).contiguous().cuda()
    d_mask, ld = _padded_i64(mask)
    ctx = Guarded((B, L, H), tdt, 4 * H)
    pb = Guarded((B, heads, L, L), torch.float32, L * L) if route != "none" else None
    assert lib.pnp_set_tuning(b"text_rows", rows) == 0
    rc = lib.pnp_op_text_self_attn(int(bf16), d_qkv.data_ptr(), d_mask.data_ptr(), ld, ctx.ptr,
                                   pb.ptr if route == "stash" else None, pb.ptr if route == "scratch" else None,
                                   B, L, H, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    tag = f"fwd L={L} B={B} heads={heads} bf16={bf16} route={route} rows={rows}"
    return ctx.check(tag + " ctx"), (pb.check(tag + " probs") if pb is not None else None)


def _check_fwd(acc, case, bf16, qkv, mask, heads, ctx, probs, p64, c64):
    B, L, _ = qkv.shape
    H = heads * R.HEAD
    pbound = R.attn_bound(p64)                                 # fp32 probs: 2e-5 * max(1, max|ref|)
    cbound = R.attn_bound_bf16(c64) if bf16 else R.attn_bound(c64)
    for b in range(B):
        pe, ce, sfx = 0.0, 0.0, ""
        if int(mask[b].sum()) == 0:                            # every key at -10000: the derived 2^-10 terms, this image only
            pe, ce = R.zero_mask_terms(p64[b], qkv[b, :, 2 * H:])
            sfx = "_zero_mask"
            if probs is not None:
                rowsum = _err(probs[b].double().sum(-1), torch.ones(heads, L))
                acc.add("zero_mask_rowsum", rowsum, 1e-6, case)       # measured 4.0e-7
        elif probs is not None:
            dead = mask[b] == 0
            assert float(probs[b][:, :, dead].abs().max()) == 0.0 if bool(dead.any()) else True, \
                (case, b, "masked key with non-zero probability")
        if probs is not None:
            acc.add("probs" + sfx, _err(probs[b], p64[b]), pbound + pe, case)
        acc.add("ctx" + sfx, _err(ctx[b], c64[b]), cbound + ce, case)


FWD_SHORT = [1, 2, 5, 63, 64, 65, 85, 127, 129, 155, 191, 192]
FWD_LONG = [193, 256, 300, 511, 512]


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("L", FWD_SHORT + FWD_LONG)
def test_self_attention_forward(lib, L, bf16):
    """probs and ctx against float64 for heads in {1, 12}, B in {1, 3}, five masks, q ~ N(0, 1) and 4 N(0, 1).
    64 < L <= 192: text_rows 1, 2, 3, 4 bit-identical (L = 65 with 4: workgroups that own one row or none of a wave's turn).
    d_probs NULL gives the same ctx bits; for L > 192 NULL is the scratch route, whose scratch then equals the stash bit for
    bit (B = 3: a wrong per-(image, head) offset shows)."""
    acc = Acc(f"gpu/self_attn_fwd/{'bf16' if bf16 else 'f32'}/L{L}")
    rows_list = (1, 2, 3, 4) if 64 < L <= 192 else (0,)
    try:
        for heads, B, scale in itertools.product((1, 12), (1, 3), (1.0, 4.0)):
            for kinds in _mask_sets(B):
                case = f"heads={heads} B={B} scale={scale:g} masks={'+'.join(kinds)}"
                qkv = R.make_qkv(B, L, heads, scale, seed=L * 7 + heads + B, bf16=bf16)
                mask = R.make_masks(kinds, L)
                p64, c64 = R.attn_fwd(qkv, mask, heads)
                base = None
                for rows in rows_list:
                    ctx, probs = _run_fwd(lib, bf16, qkv, mask, heads, "stash", rows)
                    if base is None:
                        _check_fwd(acc, case, bf16, qkv, mask, heads, ctx, probs, p64, c64)
                        base = (ctx, probs)
                    else:
                        assert torch.equal(ctx, base[0]) and torch.equal(probs, base[1]), (case, f"text_rows={rows} differs from 1")
                route = "scratch" if L > 192 else "none"
                ctx, scr = _run_fwd(lib, bf16, qkv, mask, heads, route, rows_list[-1])
                assert torch.equal(ctx, base[0]), (case, f"ctx without d_probs ({route}) differs")
                if scr is not None:
                    assert torch.equal(scr, base[1]), (case, "scratch route: probabilities differ from the stash route")
    finally:
        acc.flush()


def test_self_attention_refuses_out_of_range_shapes(lib):
    t = torch.zeros(1024, device="cuda")
    m = torch.ones(1024, dtype=torch.int64, device="cuda")
    p = t.data_ptr()
    assert lib.pnp_op_text_self_attn(0, p, m.data_ptr(), 513, p, p, p, 1, 513, 64, None) == ERR_ARG
    assert lib.pnp_op_text_self_attn(0, p, m.data_ptr(), 8, p, p, p, 1, 8, 96, None) == ERR_ARG
    assert lib.pnp_op_text_self_attn_bwd(0, p, p, p, p, p, 1, 513, 64, None) == ERR_ARG
    assert lib.pnp_op_text_self_attn_bwd(0, p, p, p, p, p, 1, 8, 96, None) == ERR_ARG
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ self-attention backward
def _run_bwd(lib, bf16, qkv, dctx, pst, heads, rows, scratch=None):
    B, L, _ = qkv.shape
    H = heads * R.HEAD
    tdt = _tdt(bf16)
    d_qkv = qkv.reshape(B * L, 3 * H).to(tdt).contiguous().cuda()
    d_dctx = dctx.reshape(B * L, H).contiguous().cuda()
    d_p = pst.contiguous().cuda()
    ds = scratch if scratch is not None else Guarded((B, heads, L, L), torch.float32, L * L)
    dqkv = Guarded((B, L, 3 * H), tdt, 4 * 3 * H)
    assert lib.pnp_set_tuning(b"text_rows", rows) == 0
    rc = lib.pnp_op_text_self_attn_bwd(int(bf16), d_qkv.data_ptr(), d_dctx.data_ptr(), d_p.data_ptr(), ds.ptr, dqkv.ptr,
                                       B, L, H, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    tag = f"bwd L={L} B={B} heads={heads} bf16={bf16} rows={rows}"
    n = B * heads * L * L
    return dqkv.check(tag + " dqkv"), ds.check(tag + " dS", written=n).reshape(-1)[:n].view(B, heads, L, L)


def _check_bwd(acc, case, bf16, qkv, mask, dctx, pst, heads, dqkv, ds):
    B, L, _ = qkv.shape
    H = heads * R.HEAD
    bound = R.attn_bound_bf16 if bf16 else R.attn_bound
    refs = R.attn_bwd_autograd(qkv, mask, dctx, heads)                       # float64 autograd: dq | dk | dv
    for i, (name, ref) in enumerate(zip(("dq", "dk", "dv"), refs)):
        acc.add(name, _err(dqkv[..., i * H:(i + 1) * H], ref), bound(ref), case)
    ds64 = R.attn_bwd(qkv, dctx, pst, heads)[3]                              # P (dP - rowsum(dP P)) from the fp32 stash
    acc.add("dS", _err(ds, ds64), R.attn_bound(ds64), case)
    g = dqkv.float()
    for b, l in ((0, 0), (B - 1, L // 2)):                                   # rows whose dctx is zero: dq exactly 0
        assert float(g[b, l, :H].abs().max()) == 0.0, (case, "dq of a zero-dctx row", b, l)
    for b in range(B):
        dead = mask[b] == 0
        if int(mask[b].sum()) == 0 or not bool(dead.any()):
            continue
        assert float(pst[b][:, :, dead].abs().max()) == 0.0                  # probability exactly 0 in the fp32 stash ...
        assert float(g[b, dead, H:].abs().max()) == 0.0, (case, "dk / dv of a key every row masks", b)   # ... so dk = dv = 0


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("L", FWD_SHORT + FWD_LONG)
def test_self_attention_backward(lib, L, bf16):
    """dq | dk | dv against float64 autograd and the dS scratch against P (dP - rowsum(dP P)), the probabilities being the
    float64 forward rounded to fp32 (the backward is judged alone).  fp32, 64 < L <= 192: text_rows 1 (one launch) and
    2, 3, 4 (two launches, rows over grid.z) bit-identical.  bf16: the one form it has."""
    acc = Acc(f"gpu/self_attn_bwd/{'bf16' if bf16 else 'f32'}/L{L}")
    rows_list = (1, 2, 3, 4) if (not bf16 and 64 < L <= 192) else (0,)
    try:
        for heads, B, scale in itertools.product((1, 12), (1, 3), (1.0, 4.0)):
            for kinds in _mask_sets(B):
                case = f"heads={heads} B={B} scale={scale:g} masks={'+'.join(kinds)}"
                qkv = R.make_qkv(B, L, heads, scale, seed=L * 11 + heads + B, bf16=bf16)
                mask = R.make_masks(kinds, L)
                dctx = R.make_dctx(B, L, heads, seed=L)
                pst = R.attn_fwd(qkv, mask, heads)[0].float()
                base = None
                for rows in rows_list:
                    dqkv, ds = _run_bwd(lib, bf16, qkv, dctx, pst, heads, rows)
                    if base is None:
                        _check_bwd(acc, case, bf16, qkv, mask, dctx, pst, heads, dqkv, ds)
                        base = (dqkv, ds)
                    else:
                        assert torch.equal(dqkv, base[0]) and torch.equal(ds, base[1]), (case, f"text_rows={rows} differs from 1")
    finally:
        acc.flush()


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("rows", [1, 3])
def test_self_attention_backward_reuses_a_dirty_scratch(lib, bf16, rows):
    """The dS scratch left full of a previous, larger launch's data (as the engine's is): same bits as with a fresh one, and
    nothing behind the smaller launch's B * heads * L * L elements is written."""
    heads, B = 2, 3
    big, small = 192, 85
    scratch = Guarded((B, heads, big, big), torch.float32, big * big)
    args = []
    for L in (big, small):
        qkv = R.make_qkv(B, L, heads, 1.0, seed=L, bf16=bf16)
        mask = R.make_masks(("ones", "prefix", "hole"), L)
        args.append((qkv, R.make_dctx(B, L, heads, seed=L), R.attn_fwd(qkv, mask, heads)[0].float()))
    _run_bwd(lib, bf16, *args[0], heads, rows, scratch=scratch)
    before = scratch.live.cpu().reshape(-1).clone()
    dqkv, ds = _run_bwd(lib, bf16, *args[1], heads, rows, scratch=scratch)
    fresh_dqkv, fresh_ds = _run_bwd(lib, bf16, *args[1], heads, rows)
    assert torch.equal(dqkv, fresh_dqkv) and torch.equal(ds, fresh_ds)
    n = B * heads * small * small
    assert torch.equal(_bits(scratch.live.cpu().reshape(-1)[n:]), _bits(before[n:]))


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,L", [(35, 25), (35, 64), (35, 85), (8, 155)])
def test_self_attention_at_the_benchmarked_launches(lib, B, L, bf16):
    """text_rows = 0: the forms the cost model picks for the benchmark's own batches (12 heads; on a 256-CU device one
    workgroup of 8 waves, then 3 and 2 workgroups per (head, image), the latter with the two-launch fp32 backward)."""
    heads = 12
    acc = Acc(f"gpu/self_attn_bench/{'bf16' if bf16 else 'f32'}/B{B}_L{L}")
    try:
        kinds = tuple(R.MASK_KINDS[i % len(R.MASK_KINDS)] for i in range(B))
        qkv = R.make_qkv(B, L, heads, 1.0, seed=B * L, bf16=bf16)
        mask = R.make_masks(kinds, L)
        dctx = R.make_dctx(B, L, heads, seed=B)
        p64, c64 = R.attn_fwd(qkv, mask, heads)
        ctx, probs = _run_fwd(lib, bf16, qkv, mask, heads, "stash", 0)
        _check_fwd(acc, "fwd", bf16, qkv, mask, heads, ctx, probs, p64, c64)
        pst = p64.float()
        dqkv, ds = _run_bwd(lib, bf16, qkv, dctx, pst, heads, 0)
        _check_bwd(acc, "bwd", bf16, qkv, mask, dctx, pst, heads, dqkv, ds)
    finally:
        acc.flush()


# ------------------------------------------------------------------------------------------ LayerNorm
LN_ROWS = [1, 3, 4, 5, 130, 1025]
LN_DIMS = [4, 64, 252, 256, 260, 768, 1020, 1024]
LN_OUTS = ("y", "yt", "yt_lo", "xhat", "rstd")


def _run_ln(lib, bf16, x, w, b, eps, want):
    rows, D = x.shape
    tdt = _tdt(bf16)
    dx, dw, db = x.contiguous().cuda(), w.cuda(), b.cuda()
    bufs = {"y": Guarded((rows, D), torch.float32, 4 * D), "yt": Guarded((rows, D), tdt, 4 * D),
            "yt_lo": Guarded((rows, D), torch.bfloat16, 4 * D), "xhat": Guarded((rows, D), torch.float32, 4 * D),
            "rstd": Guarded((rows,), torch.float32, 64)}
    ptr = {k: (bufs[k].ptr if k in want else None) for k in LN_OUTS}
    rc = lib.pnp_op_layernorm_ex(int(bf16), dx.data_ptr(), dw.data_ptr(), db.data_ptr(), eps, rows, D, ptr["y"], ptr["yt"],
                                 ptr["yt_lo"], ptr["xhat"], ptr["rstd"], None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    tag = f"layernorm rows={rows} D={D} bf16={bf16} want={want}"
    out = {k: bufs[k].check(f"{tag} {k}") for k in want}
    for k in LN_OUTS:                                       # an output that was not asked for is not written at all
        if k not in want:
            assert bool(torch.isnan(bufs[k].live.float()).all()), (tag, k, "written though its pointer was NULL")
    return out


def _ln_wants(bf16):
    for r in range(1, 6):
        for sub in itertools.combinations(LN_OUTS, r):
            if "yt_lo" in sub and (not bf16 or "yt" not in sub):
                continue
            yield sub


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("D", LN_DIMS)
def test_layernorm_all_outputs(lib, D, bf16):
    """pnp_op_layernorm_ex: xhat, rstd and y against float64 within the derived bounds of tests/_text_refs.py; the compute-type
    copy and the split-bf16 low half bit-equal to the roundings of the y the same launch wrote; a constant row exact."""
    acc = Acc(f"gpu/layernorm/{'bf16' if bf16 else 'f32'}/D{D}")
    all_outs = tuple(k for k in LN_OUTS if bf16 or k != "yt_lo")
    w, b = R.make_ln_weights(D, seed=D)
    try:
        for rows, kind, eps in itertools.product(LN_ROWS, R.LN_KINDS, (1e-6, 1e-12)):
            case = f"rows={rows} kind={kind} eps={eps:g}"
            x = R.make_ln_rows(kind, rows, D, seed=rows * 3 + D)
            o = _run_ln(lib, bf16, x, w, b, eps, all_outs)
            y64, xhat64, rstd64 = R.ln_fwd(x, w, b, eps)
            if kind == "constant":                          # variance 0: xhat = 0, y = b exactly, rstd = 1 / sqrt(eps)
                assert float(o["xhat"].abs().max()) == 0.0, case
                assert torch.equal(o["y"], b.expand(rows, D)), case
                # eps rounded to fp32 (2^-25 after the root), sqrtf <= 1 ulp, the division <= 2.5 ulp: < 4 ulp = 2^-21
                acc.add("rstd_constant_rel", float((o["rstd"].double() * eps ** 0.5 - 1).abs().max()), 2.0 ** -21, case)   # measured 6.1e-8
            else:
                acc.add("xhat", _err(o["xhat"], xhat64), R.ln_xhat_bound(x, xhat64, rstd64), case)
                acc.add("rstd_rel", float(((o["rstd"].double() - rstd64) / rstd64).abs().max()), R.ln_rstd_bound(x, rstd64), case)
                acc.add("y", _err(o["y"], y64), R.ln_y_bound(x, xhat64, rstd64, w, y64), case)
            if bf16:
                assert torch.equal(_bits(o["yt"]), _bits(o["y"].to(torch.bfloat16))), (case, "yt != bf16(y)")
                assert torch.equal(_bits(o["yt_lo"]), _bits((o["y"] - o["yt"].float()).to(torch.bfloat16))), (case, "yt_lo")
            else:
                assert torch.equal(_bits(o["yt"]), _bits(o["y"])), (case, "fp32 yt != y")
        # every subset of the optional outputs gives the same bits as all of them together
        x = torch.cat([R.make_ln_rows(k, 5, D, seed=D + i) for i, k in enumerate(("normal", "offset"))])
        full = _run_ln(lib, bf16, x, w, b, 1e-12, all_outs)
        for want in _ln_wants(bf16):
            part = _run_ln(lib, bf16, x, w, b, 1e-12, want)
            for k in want:
                assert torch.equal(_bits(part[k]), _bits(full[k])), (want, k)
    finally:
        acc.flush()


def test_layernorm_refuses_out_of_range_shapes(lib):
    t = torch.zeros(8 * 1028, device="cuda")
    p = t.data_ptr()
    assert lib.pnp_op_layernorm_ex(0, p, p, p, 1e-6, 4, 1028, p, None, None, None, None, None) == ERR_ARG
    assert lib.pnp_op_layernorm_ex(0, p, p, p, 1e-6, 4, 770, p, None, None, None, None, None) == ERR_ARG
    assert lib.pnp_op_layernorm_ex(0, p, p, p, 1e-6, 4, 64, p, p, p, None, None, None) == ERR_ARG
    torch.cuda.synchronize()


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("D", LN_DIMS)
def test_layernorm_backward(lib, D, bf16):
    """dx against float64 rstd (g - mean(g) - xhat mean(g xhat)) with xhat / rstd from the float64 forward rounded to fp32; the
    compute-type copy bit-equal to the rounded dx; rows beyond `rows` of the last 4-row workgroup untouched (guards)."""
    acc = Acc(f"gpu/layernorm_bwd/{'bf16' if bf16 else 'f32'}/D{D}")
    tdt = _tdt(bf16)
    w, b = R.make_ln_weights(D, seed=D)
    try:
        for rows, kind, eps in itertools.product(LN_ROWS, R.LN_KINDS, (1e-6, 1e-12)):
            case = f"rows={rows} kind={kind} eps={eps:g}"
            x = R.make_ln_rows(kind, rows, D, seed=rows * 5 + D)
            _, xhat64, rstd64 = R.ln_fwd(x, w, b, eps)
            xh, rs = xhat64.float(), rstd64.float()
            dy = torch.randn(rows, D, generator=torch.Generator().manual_seed(rows + D))
            ref = R.ln_bwd(dy, w, xh, rs)
            got = {}
            for want in (("dx", "dxt"), ("dx",), ("dxt",)) if rows in (5, 130) else (("dx", "dxt"),):
                bufs = {"dx": Guarded((rows, D), torch.float32, 4 * D), "dxt": Guarded((rows, D), tdt, 4 * D)}
                dev = [t.contiguous().cuda() for t in (dy, w, xh, rs)]
                rc = lib.pnp_op_layernorm_bwd(int(bf16), *[t.data_ptr() for t in dev], rows, D,
                                              bufs["dx"].ptr if "dx" in want else None, bufs["dxt"].ptr if "dxt" in want else None, None)
                assert rc == 0, rc
                torch.cuda.synchronize()
                got[want] = {k: bufs[k].check(f"layernorm_bwd {case} {k}") for k in want}
            o = got[("dx", "dxt")]
            acc.add("dx", _err(o["dx"], ref), R.ln_bwd_bound(dy, w, xh, rs), case)
            assert torch.equal(_bits(o["dxt"]), _bits(o["dx"].to(tdt))), (case, "dxt != rounded dx")
            for want, g in got.items():
                for k in want:
                    assert torch.equal(_bits(g[k]), _bits(o[k])), (case, want, k)
    finally:
        acc.flush()


# ------------------------------------------------------------------------------------------ exact kernels
@pytest.mark.parametrize("H", [64, 768])
@pytest.mark.parametrize("enc_id", [-1, 7])
def test_text_embed_is_exact(lib, H, enc_id):
    """One fp32 add per element: bit-equal to numpy.  enc_id >= 0 replaces column 0, enc_id < 0 keeps it; ids below 0 and at
    or above `vocab` clamp to 0 and vocab - 1 (the ABI's documented behaviour); id columns beyond L are never read."""
    vocab = 50
    for B, L in itertools.product((1, 3, 35), (1, 5, 40)):
        rng = np.random.default_rng(B * 100 + L + H)
        ids = rng.integers(-3, vocab + 3, size=(B, L)).astype(np.int64)
        ids.flat[0] = -(1 << 40)
        ids.flat[-1] = 1 << 40
        word = rng.standard_normal((vocab, H)).astype(np.float32)
        pos = rng.standard_normal((L + 2, H)).astype(np.float32)
        d_ids, ld = _padded_i64(torch.from_numpy(ids), extra=2)
        out = Guarded((B, L, H), torch.float32, 4 * H)
        dw, dp = torch.from_numpy(word).cuda(), torch.from_numpy(pos).cuda()
        assert lib.pnp_op_text_embed(d_ids.data_ptr(), ld, dw.data_ptr(), dp.data_ptr(), out.ptr, B, L, H, enc_id, vocab, None) == 0
        torch.cuda.synchronize()
        eff = ids.copy()
        if enc_id >= 0:
            eff[:, 0] = enc_id
        ref = word[np.clip(eff, 0, vocab - 1)] + pos[None, :L]
        got = out.check(f"text_embed B={B} L={L} H={H}").numpy()
        np.testing.assert_array_equal(got.view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize("H", [64, 768])
def test_itm_head_and_grad_seed(lib, H):
    """itm_head: token 0 only (the others hold NaN) against float64 within 2^-22 sum|h_d w_d| + 2^-23 |logit|.
    itm_grad_seed: weight row 1 at token 0, zeros elsewhere, bit-equal."""
    acc = Acc(f"gpu/itm_head/H{H}")
    try:
        for B, L in itertools.product((1, 3, 35), (1, 5, 40)):
            g = torch.Generator().manual_seed(B * 10 + L)
            h = torch.randn(B, L, H, generator=g)
            w, bias = 0.05 * torch.randn(2, H, generator=g), torch.randn(2, generator=g)
            ref = R.itm_head(h, w, bias)
            bound = R.itm_bound(h, w, ref)
            h[:, 1:] = float("nan")
            logits = Guarded((B, 2), torch.float32, 64)
            dev = [t.contiguous().cuda() for t in (h, w, bias)]
            assert lib.pnp_op_itm_head(*[t.data_ptr() for t in dev], logits.ptr, B, L, H, None) == 0
            seed = Guarded((B, L, H), torch.float32, 4 * H)
            assert lib.pnp_op_itm_grad_seed(dev[1].data_ptr(), seed.ptr, B, L, H, None) == 0
            torch.cuda.synchronize()
            got = logits.check(f"itm_head B={B} L={L}")
            acc.add("logits_fraction", float(((got.double() - ref).abs() / bound).max()), 1.0, f"B={B} L={L}")
            want = torch.zeros(B, L, H)
            want[:, 0] = w[1]
            assert torch.equal(_bits(seed.check(f"itm_grad_seed B={B} L={L}")), _bits(want))
    finally:
        acc.flush()


@pytest.mark.parametrize("B", [1, 3, 35])
def test_cls_rows_is_exact(lib, B):
    """x[b, 0, :] = cls + pos[0] bit-equal to numpy; every other row keeps its bits."""
    for N, D in itertools.product((1, 17), (64, 1024)):
        rng = np.random.default_rng(B + N + D)
        cls = rng.standard_normal(D).astype(np.float32)
        pos = rng.standard_normal((N, D)).astype(np.float32)
        x = Guarded((B, N, D), torch.float32, 4 * D)
        x.live.fill_(7.0)
        dc, dp = torch.from_numpy(cls).cuda(), torch.from_numpy(pos).cuda()
        assert lib.pnp_op_cls_rows(dc.data_ptr(), dp.data_ptr(), x.ptr, B, N, D, None) == 0
        torch.cuda.synchronize()
        ref = np.full((B, N, D), 7.0, dtype=np.float32)
        ref[:, 0] = cls + pos[0]
        np.testing.assert_array_equal(x.check(f"cls_rows B={B} N={N} D={D}").numpy().view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("B", [1, 3, 35])
@pytest.mark.parametrize("P", [4, 21, 48])
def test_patchify_is_exact(lib, P, B, bf16):
    """The im2col of the 16 x 16 patch convolution: fp32 bit-equal, bf16 bit-equal to the round-to-nearest-even rounding, with
    and without a `dropped` mask; dropped patches exactly zero."""
    S = 16 * P
    g = torch.Generator().manual_seed(P * 10 + B)
    img = torch.randn(B, 3, S, S, generator=g)
    ref = img.view(B, 3, P, 16, P, 16).permute(0, 2, 4, 1, 3, 5).reshape(B * P * P, 768)
    d_img = img.cuda()
    for with_drop in (False, True):
        dropped = (torch.rand(B * P * P, generator=g) < 0.3).to(torch.uint8) if with_drop else None
        want = ref.clone()
        if with_drop:
            dropped[0], dropped[-1] = 1, 0
            want[dropped.bool()] = 0.0
        want = want.to(_tdt(bf16))
        out = Guarded((B * P * P, 768), _tdt(bf16), 4 * 768)
        d_drop = dropped.cuda() if with_drop else None
        assert lib.pnp_op_patchify(int(bf16), d_img.data_ptr(), d_drop.data_ptr() if with_drop else None, out.ptr, B, S, P, None) == 0
        torch.cuda.synchronize()
        got = out.check(f"patchify P={P} B={B} bf16={bf16} drop={with_drop}")
        assert torch.equal(_bits(got), _bits(want)), f"P={P} B={B} drop={with_drop}"
        if with_drop:
            assert float(got[dropped.bool()].float().abs().max()) == 0.0


@pytest.mark.parametrize("n", [1, 255, 256, 257, 2 ** 20 + 1])
def test_split_and_cast_round_to_nearest_even(lib, n):
    """pnp_op_split / pnp_op_cast bit-equal to torch's round-to-nearest-even on normal values, signed zeros and +-inf (the lo
    half of an infinity is NaN in both: compared as NaN == NaN)."""
    g = torch.Generator().manual_seed(n)
    v = torch.randn(n, generator=g) * torch.exp2(torch.randint(-30, 31, (n,), generator=g).float())
    special = torch.tensor([0.0, -0.0, float("inf"), -float("inf"), 1.00390625, -3.0e38])   # incl. a tie to even and a near-max
    k = min(n, special.numel())
    v[:k] = special[(torch.arange(k) + n) % special.numel()]
    d_v = v.cuda()
    hi, lo, cb, cf = (Guarded((n,), dt, 64) for dt in (torch.bfloat16, torch.bfloat16, torch.bfloat16, torch.float32))
    assert lib.pnp_op_split(d_v.data_ptr(), hi.ptr, lo.ptr, n, None) == 0
    assert lib.pnp_op_cast(1, d_v.data_ptr(), cb.ptr, n, None) == 0
    assert lib.pnp_op_cast(0, d_v.data_ptr(), cf.ptr, n, None) == 0
    torch.cuda.synchronize()
    ref_hi = v.to(torch.bfloat16)
    ref_lo = (v - ref_hi.float()).to(torch.bfloat16)
    fin = torch.isfinite(v)
    got_hi, got_cb, got_cf = hi.check("split hi"), cb.check("cast bf16"), cf.check("cast f32")
    got_lo = lo.live.cpu()
    raw = _bits(lo.buf).cpu()
    assert torch.equal(raw[:lo.g], lo.guard_bits) and torch.equal(raw[lo.g + n:], lo.guard_bits)
    assert torch.equal(_bits(got_hi), _bits(ref_hi)) and torch.equal(_bits(got_cb), _bits(ref_hi))
    assert torch.equal(_bits(got_cf), _bits(v))
    assert torch.equal(_bits(got_lo[fin]), _bits(ref_lo[fin]))
    assert bool(torch.isnan(got_lo[~fin].float()).all()) and bool(torch.isnan(ref_lo[~fin].float()).all())
