"""GPU: the three ViT self-attention kernels (vit_attn_kernel<float>, vit_attn32_kernel, vit_attn32_x3_kernel) and xattn_kernel
launched alone through pnp_op_vit_attention / pnp_op_vit_attention_x3 / pnp_op_xattn and compared with float64
(tests/_gemm_refs.py), at every token count where the workgroup partition changes (N = 32 | 33: one or two 32-query waves; 64 |
65: key tiles; 256 | 257: one or two workgroups of 8 waves; 768 | 769: 8 or 12 waves per workgroup in the split form) and on
structured scores: the running maximum rising in the last key tile only, sitting in the first tile with everything behind it
underflowing, a constant row, and outlier channels that push the scaled scores into the hundreds.

Common to every case: fused q | k | v rows with a leading dimension larger than 3 D whose pad columns hold NaN, V read in place
(bf16 / split forms) or from a V^T buffer whose pad columns are zero as documented and whose columns beyond the last image hold
NaN (fp32); every output is a NaN-filled guarded buffer whose pad columns and guards must keep their sentinel.
Run on the MI355X box:  python -m pytest tests/test_attn_ops_gpu.py -m gpu -x -q
"""
import pytest

torch = pytest.importorskip("torch")

import _gemm_refs as R          # noqa: E402
from _gpu_guard import Acc, Guarded2D, padded          # noqa: E402

pytestmark = pytest.mark.gpu

ERR_ARG = -22
DEV = "cuda"
PARTITION_N = [1, 31, 32, 33, 64, 65, 256, 257, 768, 769]
GEOMETRY_N = [17, 197, 442, 577, 2305]


@pytest.fixture()
def lib():
    from pnp_ovss import hip
    return hip.load_library()


def _geometry(N, i):
    """(B, heads): B in {1, 3} and heads in {12, 16} alternate over the cases; the 768-pixel geometry stays at one image."""
    if N > 1024:
        return 1, 12
    return ((1, 12), (3, 16), (3, 12), (1, 16))[i % 4]


def _run_vit(lib, kind, q, k, v, heads):
    """q, k, v (B, N, D) fp32, already exact in the kernel's operand type.  Returns the context (B, N, D) float64 on the CPU."""
    B, N, D = q.shape
    ld = 3 * D + 16
    fused = torch.cat([q, k, v], dim=-1).reshape(B * N, 3 * D)
    tag = f"vit_attention {kind} B={B} N={N} heads={heads}"
    if kind == "x3":
        hi, lo = R.split_pair(fused)
        assert torch.equal(hi.float() + lo.float(), fused), "x3 operands must be exact (hi, lo) pairs"
        (dh, kh), (dl, kl) = padded(hi, ld, torch.bfloat16), padded(lo, ld, torch.bfloat16)
        ch, cl = Guarded2D(B * N, D, D, torch.bfloat16), Guarded2D(B * N, D, D, torch.bfloat16)
        rc = lib.pnp_op_vit_attention_x3(dh.data_ptr(), dl.data_ptr(), ld, D, ch.ptr, cl.ptr, B, heads, N, 0.125, None)
        assert rc == 0, (tag, rc)
        torch.cuda.synchronize()
        got = ch.check(tag + " ctx_hi").double() + cl.check(tag + " ctx_lo").double()
        return got.view(B, N, D)
    Npad = (N + 63) // 64 * 64
    if kind == "bf16":
        d, keep = padded(fused, ld, torch.bfloat16)
        ctx = Guarded2D(B * N, D, D, torch.bfloat16)
        rc = lib.pnp_op_vit_attention(1, d.data_ptr(), ld, D, d.data_ptr() + 2 * D * 2, ld, Npad, ctx.ptr, B, heads, N, 0.125, None)
    else:
        d, keep = padded(fused, ld, torch.float32)
        ld_vt = (B + 2) * Npad                                 # two more image slots than the launch has: NaN
        vt = torch.full((D, ld_vt), float("nan"), device=DEV)
        vt[:, :B * Npad] = 0.0                                 # pad columns of the live images: zero, as documented
        vt[:, :B * Npad].view(D, B, Npad)[:, :, :N] = v.permute(2, 0, 1)
        ctx = Guarded2D(B * N, D, D, torch.float32)
        rc = lib.pnp_op_vit_attention(0, d.data_ptr(), ld, D, vt.data_ptr(), ld_vt, Npad, ctx.ptr, B, heads, N, 0.125, None)
    assert rc == 0, (tag, rc)
    torch.cuda.synchronize()
    return ctx.check(tag + " ctx").double().view(B, N, D)


def _operands(kind, case, B, N, heads, seed):
    q, k, v = R.make_attn_qkv(case, B, N, heads, seed, device=DEV)
    if kind == "bf16":
        return tuple(a.to(torch.bfloat16).float() for a in (q, k, v))
    if kind == "x3":                                           # exact pairs: what the kernel is given IS what the reference sees
        return tuple(sum(t.float() for t in R.split_pair(a)) for a in (q, k, v))
    return q, k, v


@pytest.mark.parametrize("kind", ["f32", "bf16", "x3"])
@pytest.mark.parametrize("N", PARTITION_N + GEOMETRY_N)
def test_vit_attention_partitions_and_score_structure(lib, N, kind):
    """Every score structure at every token count, against float64 of the operands the kernel is given.  Bounds: the project's
    (2e-5 fp32, 2e-2 bf16, 5e-5 split) times max(1, max|ref|); the outlier case of the fp32 and split kernels uses four times the
    float32 restatement's measured error (_gemm_refs.ATTN_TOL_CASE).  No output may be NaN or inf."""
    acc = Acc(f"gpu/vit_attn/{kind}/N{N}")
    try:
        for i, case in enumerate(R.ATTN_CASES):
            B, heads = _geometry(N, i + N)
            q, k, v = _operands(kind, case, B, N, heads, seed=N * 10 + i)
            ref, s = R.attn64(q, k, v, heads)
            got = _run_vit(lib, kind, q, k, v, heads)
            assert bool(torch.isfinite(got).all()), (kind, case, N, "NaN / inf in the context")
            err = float((got - ref.cpu()).abs().max())
            acc.add(case, err, R.attn_bound(kind, case, ref), f"case={case} B={B} heads={heads} max|score|={float(s.abs().max()):.0f}")
            if case == "max_first":                            # the margin the case promises
                top2 = s.topk(min(2, N), dim=-1).values
                assert N == 1 or float((top2[..., 0] - top2[..., 1]).min()) >= 100.0
            if case == "constant":                             # uniform softmax: the context is the mean of v, for every query
                mean = v.double().mean(dim=1, keepdim=True).expand(B, N, heads * 64)
                acc.add("constant_vs_mean", float((got - mean.cpu()).abs().max()), R.attn_bound(kind, case, ref), f"B={B} heads={heads}")
    finally:
        acc.flush()


def test_vit_attention_refuses_bad_shapes(lib):
    t = torch.zeros(64 * 256, device=DEV)
    p = t.data_ptr()
    assert lib.pnp_op_vit_attention(0, p, 128, 64, p, 64, 64, p, 1, 1, 0, 0.125, None) == ERR_ARG           # N = 0
    assert lib.pnp_op_vit_attention(0, p, 128, 96, p, 64, 64, p, 1, 1, 8, 0.125, None) == ERR_ARG           # D != 64 heads
    assert lib.pnp_op_vit_attention(0, p, 128, 64, p, 64, 32, p, 1, 1, 8, 0.125, None) == ERR_ARG           # n_pad % 64
    assert lib.pnp_op_vit_attention(0, None, 128, 64, p, 64, 64, p, 1, 1, 8, 0.125, None) == ERR_ARG
    assert lib.pnp_op_vit_attention_x3(p, p, 128, 64, p, p, 1, 1, 8, 0.125, None) == ERR_ARG                 # ld_qkv < 3 D
    assert lib.pnp_op_vit_attention_x3(p, None, 192, 64, p, p, 1, 1, 8, 0.125, None) == ERR_ARG
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ cross attention
XATTN_SHAPES = [(26, 1), (197, 64), (512, 65), (512, 7), (513, 64), (513, 1), (577, 65), (2305, 65), (2560, 1)]


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("N,L", XATTN_SHAPES)
def test_cross_attention_launch_shapes(lib, N, L, bf16):
    """pnp_op_xattn modes 0, 1, 2 at L in {1, 64, 65} and at N = 512 | 513, the switch between its two launch shapes, against
    the float64 forward and autograd backward of B/med.py:229-283.  Rows whose upstream gradient is exactly zero give an
    exactly zero dq.  f32: 2e-5, bf16 operands: 3e-2, times max(1, max|ref|)."""
    heads, B = 12, 2
    H = heads * 64
    Npad = (N + 63) // 64 * 64
    kind = "bf16" if bf16 else "f32"
    tdt = torch.bfloat16 if bf16 else torch.float32
    g = torch.Generator(device=DEV).manual_seed(N * 100 + L)
    rnd = lambda *s: torch.randn(*s, generator=g, device=DEV)
    K, V, q, dctx = rnd(B, N, H) * 0.5, rnd(B, N, H) * 0.5, rnd(B, L, H), rnd(B, L, H)
    dctx[0, 0] = 0
    dctx[:, 1:3] = 0
    K, V, q, dctx = (a.to(tdt).float() for a in (K, V, q, dctx))
    ld = H + 16

    def tr(a):                                                 # [H, B * Npad], pad columns zero
        t = torch.zeros(H, B, Npad, device=DEV)
        t[:, :, :N] = a.permute(2, 0, 1)
        return t.reshape(H, B * Npad).to(tdt).contiguous()
    (Kn, k1), (Vn, k2) = padded(K.reshape(B * N, H), ld, tdt), padded(V.reshape(B * N, H), ld, tdt)
    (qd, k3), (dcd, k4) = padded(q.reshape(B * L, H), ld, tdt), padded(dctx.reshape(B * L, H), ld, tdt)
    Kt, Vt = tr(K), tr(V)
    # the kernel writes whole 16-key tiles: columns [0, ceil16(N)) of a row; the rest of the Npad stride keeps its sentinel
    N16 = (N + 15) // 16 * 16
    P = Guarded2D(B * heads * L, N16, Npad, torch.float32)
    dP = Guarded2D(B * heads * L, N16, Npad, torch.float32)
    ctx, dq = Guarded2D(B * L, H, H + 8, tdt), Guarded2D(B * L, H, H + 8, tdt)
    p = lambda t: t.data_ptr()
    bf = int(bf16)
    tag = f"xattn {kind} N={N} L={L}"
    assert lib.pnp_op_xattn(bf, 0, p(Kn), ld, p(Vt), B * Npad, Npad, p(qd), ld, ctx.ptr, H + 8, P.ptr, Npad, B, L, N, heads, None) == 0
    assert lib.pnp_op_xattn(bf, 2, p(Vn), ld, None, 0, Npad, p(dcd), ld, None, 0, dP.ptr, Npad, B, L, N, heads, None) == 0
    torch.cuda.synchronize()
    Pg = P.check(tag + " probs").reshape(B, heads, L, N16)
    assert lib.pnp_op_xattn(bf, 1, p(Vn), ld, p(Kt), B * Npad, Npad, p(dcd), ld, dq.ptr, H + 8, P.ptr, Npad, B, L, N, heads, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(P.check(tag + " probs after mode 1").reshape(B, heads, L, N16), Pg), "mode 1 must only read d_probs"
    f = lambda a: a.double().view(B, -1, heads, 64).permute(0, 2, 1, 3)
    Kh, Vh, qh, dch = f(K), f(V), f(q), f(dctx)
    Pr = (qh @ Kh.transpose(-1, -2) / 8).softmax(-1)
    ctxr = (Pr @ Vh).permute(0, 2, 1, 3).reshape(B * L, H)
    dPr = dch @ Vh.transpose(-1, -2)
    dS = Pr * (dPr - (dPr * Pr).sum(-1, keepdim=True))
    dqr = (dS @ Kh / 8).permute(0, 2, 1, 3).reshape(B * L, H)
    dPg, ctxg, dqg = dP.check(tag + " dP").reshape(B, heads, L, N16), ctx.check(tag + " ctx"), dq.check(tag + " dq")
    acc = Acc(f"gpu/xattn/{kind}/N{N}_L{L}")
    try:
        for name, got, ref in (("probs", Pg[..., :N], Pr), ("ctx", ctxg, ctxr), ("dP", dPg[..., :N], dPr), ("dq", dqg, dqr)):
            err = float((got.double() - ref.cpu()).abs().max())
            acc.add(name, err, R.XATTN_TOL[kind] * max(1.0, float(ref.abs().max())), tag)
    finally:
        acc.flush()
    if N16 > N:
        assert float(Pg[..., N:].abs().max()) == 0.0                            # keys past N: probability exactly 0
    dq3 = dqg.float().view(B, L, H)
    assert float(dq3[0, 0].abs().max()) == 0.0                                  # zero upstream rows stay exactly zero
    assert L < 2 or float(dq3[:, 1:3].abs().max()) == 0.0
