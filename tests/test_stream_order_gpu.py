"""GPU: every entry point of include/pnp_hip.h that takes a `stream` stays on it -- no launch, memset or copy of the call runs on
another stream (tests/_stream_gate.py has the method: the call sits behind a ~100 ms blocker on a stream S of its own, its real
inputs arrive on S behind the blocker, and its outputs are probed from a third stream while the blocker still runs).

One gated call per case, at the smallest shape that still takes every launch of the entry point.  No float64 reference is
needed here: the default-stream result of every one of these calls is pinned by the operator and parity tests, and the gated
result must equal it bit for bit.  The stream-K tail is switched off for the whole module (two runs of a launch with a tail
may differ in summation order only between modes, but the tail's cross-stream event chain is test_streamk_chain_gpu.py's).

CASES maps a case id to the entry points it gates (tests/test_stream_order_cpu.py holds that table against the header) and to
the function that builds the case.  The engine cases run blip_itm_small(128) in the benchmarked split-bf16 mode at B = 2; the
post-processing stages share one prepared batch of sizes (24, 40) and (33, 45); the stand-alone CRF cases run case 2 of
_crf_terms_ref.CASES.

Measured on MI355X (PNP_TEST_MEASURE_LOG): blockers of 100 ms (200 ms for drop_loop), the calls alone 0.02 .. 4.5 ms, the
smallest blocker / alone ratio 44; 2 .. 5 stream candidates tried.  The host was held by pnp_post_prepare, pnp_crf_set_batch*,
pnp_crf_kl, pnp_op_sort_pairs, pnp_op_scan_i32 and pnp_jpeg_decode_scans with h_group_ms, and by nothing else.  The calls
that upload a small host table with hipMemcpyAsync from pageable memory returned with the blocker pending: pnp_png_encode and
pnp_jpeg_encode (descriptors and code tables), pnp_crf_step with a matrix term (crf_matrices: the scalar term as w I) and
pnp_crf_backward_terms (tile table).
Run on the MI355X box:  python -m pytest tests/test_stream_order_gpu.py -m gpu -x -q
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import _gemm_refs as R          # noqa: E402
from _stream_gate import MAY_BLOCK, Case, Gate, blocker_cycles, early_of, sptr          # noqa: E402, F401

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, F32, U8, I32, I64 = torch.bfloat16, torch.float32, torch.uint8, torch.int32, torch.int64
TAG = "gpu/stream_order"

# Entry points with a stream parameter that no case names: pure aliases of a covered sibling (the same launcher behind them).
EXCLUDED = {
    "pnp_op_gemm": "pnp_op_gemm_ex with the compute-type output left out: the same launcher",
    "pnp_op_layernorm": "pnp_op_layernorm_ex with d_y alone",
    "pnp_compute_gradcam": "pnp_compute_gradcam_layer at layer = stash_layer",
    "pnp_drop_loop": "pnp_drop_loop_layer at layer = stash_layer",
    "pnp_xattn_grad": "pnp_xattn_grad_layer at layer = stash_layer",
}

CASES = {}


def case(name, *covers, may_block=False):
    def reg(fn):
        CASES[name] = (covers, fn, may_block)
        return fn
    return reg


def rnd(seed, *shape, dtype=F32, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(*shape, generator=g, device=DEV) * scale).to(dtype)


def split(x):
    hi = x.to(BF)
    return hi, (x - hi.float()).to(BF)


def p(t):
    return None if t is None else t.data_ptr()


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def up(buf):
    return torch.frombuffer(bytearray(bytes(buf)), dtype=U8).to(DEV)


# ================================================================================================ operators
def _gemm_ex(ctx, bf16):
    M, N, K = 70, 68, 64
    from pnp_ovss import hip
    assert hip.gemm_plan("bf16" if bf16 else "f32", M, N, K, has=("bias", "resid", "out_f32", "out_t"), mode=1).name == "g64"
    tdt = BF if bf16 else F32
    c = Case(f"gemm_ex_{'bf16' if bf16 else 'f32'}")
    A, B = c.late(rnd(1, M, K, dtype=tdt)), c.late(rnd(2, N, K, dtype=tdt))
    bias, resid = c.late(rnd(3, N)), c.late(rnd(4, M, N))
    out, out_t = c.out("out_f32", (M, N)), c.out("out_t", (M, N), tdt)
    c.call = lambda s: ctx.lib.pnp_op_gemm_ex(int(bf16), p(A), K, p(B), K, M, N, K, p(bias), p(resid), N, p(out), N, p(out_t), N, 1, sptr(s))
    return c


@case("gemm_ex_f32", "pnp_op_gemm_ex")
def _(ctx):
    return _gemm_ex(ctx, False)


@case("gemm_ex_bf16", "pnp_op_gemm_ex")
def _(ctx):
    return _gemm_ex(ctx, True)


@case("gemm_args_gelu_stash", "pnp_op_gemm_args")
def _(ctx):
    """The generic 64 x 64 branch with bias + residual + the GELU stash (d_aux), which pnp_op_gemm_ex does not expose."""
    M, N, K = 70, 68, 64
    c = Case("gemm_args_gelu_stash")
    A, B, bias, resid = c.late(rnd(1, M, K)), c.late(rnd(2, N, K)), c.late(rnd(3, N)), c.late(rnd(4, M, N))
    out, aux = c.out("out_f32", (M, N)), c.out("aux", (M, N))
    c.call = lambda s: ctx.lib.pnp_op_gemm_args(0, p(A), K, p(B), K, M, N, K, p(bias), 0, p(resid), N, p(out), N, None, 0, 1, p(aux), N,
                                                0, 0, 0, sptr(s))
    return c


X3_SHAPE = (300, 512, 256)          # test_streamk_chain_gpu.py's: 2 x 2 wide tiles, M ragged


@case("gemm_x3", "pnp_op_gemm_x3")
def _(ctx):
    M, N, K = X3_SHAPE
    c = Case("gemm_x3")
    (Ah, Al), (Bh, Bl) = split(rnd(1, M, K)), split(rnd(2, N, K, scale=0.25))
    Ah, Al, Bh, Bl = c.late(Ah), c.late(Al), c.late(Bh), c.late(Bl)
    bias, resid = c.late(rnd(3, N)), c.late(rnd(4, M, N))
    out = c.out("out_f32", (M, N))
    c.call = lambda s: ctx.lib.pnp_op_gemm_x3(p(Ah), p(Al), K, p(Bh), p(Bl), K, M, N, K, p(bias), 0, p(resid), N, p(out), N, None, None,
                                              0, 0, 0, 0, sptr(s))
    return c


@case("gemm_x3_gelu_pair", "pnp_op_gemm_x3")
def _(ctx):
    M, N, K = X3_SHAPE
    c = Case("gemm_x3_gelu_pair")
    (Ah, Al), (Bh, Bl) = split(rnd(1, M, K)), split(rnd(2, N, K, scale=0.25))
    Ah, Al, Bh, Bl, bias = c.late(Ah), c.late(Al), c.late(Bh), c.late(Bl), c.late(rnd(3, N))
    hi, lo = c.out("out_hi", (M, N), BF), c.out("out_lo", (M, N), BF)
    c.call = lambda s: ctx.lib.pnp_op_gemm_x3(p(Ah), p(Al), K, p(Bh), p(Bl), K, M, N, K, p(bias), 0, None, 0, None, 0, p(hi), p(lo),
                                              N, 1, 0, 0, sptr(s))
    return c


@case("gemm_x3a", "pnp_op_gemm_x3a")
def _(ctx):
    M, N, K = X3_SHAPE
    c = Case("gemm_x3a")
    Bh, Bl = split(rnd(2, N, K, scale=0.25))
    A, Bh, Bl, bias, resid = c.late(rnd(1, M, K)), c.late(Bh), c.late(Bl), c.late(rnd(3, N)), c.late(rnd(4, M, N))
    out, aux = c.out("out_f32", (M, N)), c.out("aux", (M, N))
    c.call = lambda s: ctx.lib.pnp_op_gemm_x3a(p(A), K, p(Bh), p(Bl), K, M, N, K, p(bias), p(resid), N, p(out), N, 1, p(aux), N, sptr(s))
    return c


@case("gemm_tokcols", "pnp_op_gemm_tokcols")
def _(ctx):
    M, N, K = X3_SHAPE
    div, pad = 256, 264
    c = Case("gemm_tokcols")
    A, B, bias = c.late(rnd(1, M, K, dtype=BF)), c.late(rnd(2, N, K, dtype=BF)), c.late(rnd(3, M))
    out = c.out("out_t", (M, 2 * pad), BF)
    c.call = lambda s: ctx.lib.pnp_op_gemm_tokcols(1, p(A), K, p(B), K, M, N, K, p(bias), p(out), 2 * pad, div, pad, sptr(s))
    return c


ATT = dict(B=2, heads=2, N=65, D=128, n_pad=128)


@case("vit_attention_f32", "pnp_op_vit_attention")
def _(ctx):
    B, heads, N, D, n_pad = (ATT[k] for k in ("B", "heads", "N", "D", "n_pad"))
    c = Case("vit_attention_f32")
    qk = c.late(rnd(1, B * N, 2 * D))
    v = torch.zeros(D, B, n_pad, device=DEV)
    v[:, :, :N] = rnd(2, D, B, N)
    vt = c.late(v.reshape(D, B * n_pad))
    out = c.out("ctx", (B * N, D))
    c.call = lambda s: ctx.lib.pnp_op_vit_attention(0, p(qk), 2 * D, D, p(vt), B * n_pad, n_pad, p(out), B, heads, N, 0.125, sptr(s))
    return c


@case("vit_attention_bf16", "pnp_op_vit_attention")
def _(ctx):
    B, heads, N, D = (ATT[k] for k in ("B", "heads", "N", "D"))
    c = Case("vit_attention_bf16")
    qkv = c.late(rnd(1, B * N, 3 * D, dtype=BF))
    out = c.out("ctx", (B * N, D), BF)
    c.call = lambda s: ctx.lib.pnp_op_vit_attention(1, p(qkv), 3 * D, D, p(qkv) + 2 * D * 2, 3 * D, 128, p(out), B, heads, N, 0.125, sptr(s))
    return c


@case("vit_attention_x3", "pnp_op_vit_attention_x3")
def _(ctx):
    B, heads, N, D = (ATT[k] for k in ("B", "heads", "N", "D"))
    c = Case("vit_attention_x3")
    hi, lo = split(rnd(1, B * N, 3 * D))
    hi, lo = c.late(hi), c.late(lo)
    ch, cl = c.out("ctx_hi", (B * N, D), BF), c.out("ctx_lo", (B * N, D), BF)
    c.call = lambda s: ctx.lib.pnp_op_vit_attention_x3(p(hi), p(lo), 3 * D, D, p(ch), p(cl), B, heads, N, 0.125, sptr(s))
    return c


@case("layernorm_ex", "pnp_op_layernorm_ex")
def _(ctx):
    rows, D = 5, 260
    c = Case("layernorm_ex")
    x, w, b = c.late(rnd(1, rows, D)), c.late(rnd(2, D)), c.late(rnd(3, D))
    y, yt, lo = c.out("y", (rows, D)), c.out("yt", (rows, D), BF), c.out("yt_lo", (rows, D), BF)
    xhat, rstd = c.out("xhat", (rows, D)), c.out("rstd", (rows,))
    c.call = lambda s: ctx.lib.pnp_op_layernorm_ex(1, p(x), p(w), p(b), 1e-6, rows, D, p(y), p(yt), p(lo), p(xhat), p(rstd), sptr(s))
    return c


@case("layernorm_bwd", "pnp_op_layernorm_bwd")
def _(ctx):
    rows, D = 5, 260
    c = Case("layernorm_bwd")
    dy, w, xhat = c.late(rnd(1, rows, D)), c.late(rnd(2, D)), c.late(rnd(3, D))
    rstd = c.late(rnd(4, rows).abs() + 0.5)
    dx, dxt = c.out("dx", (rows, D)), c.out("dxt", (rows, D), BF)
    c.call = lambda s: ctx.lib.pnp_op_layernorm_bwd(1, p(dy), p(w), p(xhat), p(rstd), rows, D, p(dx), p(dxt), sptr(s))
    return c


def _xattn(ctx, mode, N, L):
    B, heads = 2, 2
    H = heads * 64
    npad = (N + 63) // 64 * 64
    c = Case(f"xattn_mode{mode}_N{N}_L{L}")

    def tr(a):                                                 # [H, B * npad], pad columns zero
        t = torch.zeros(H, B, npad, device=DEV)
        t[:, :, :N] = a.permute(2, 0, 1)
        return t.reshape(H, B * npad).contiguous()
    K, V = rnd(1, B, N, H, scale=0.5), rnd(2, B, N, H, scale=0.5)
    x = c.late(rnd(3, B * L, H))                               # q (mode 0) or dctx (modes 1, 2)
    if mode == 0:
        nat, trn = c.late(K.reshape(B * N, H)), c.late(tr(V))
        out, probs = c.out("ctx", (B * L, H)), c.out("probs", (B * heads * L, npad))
    elif mode == 1:
        nat, trn = c.late(V.reshape(B * N, H)), c.late(tr(K))
        out = c.out("dq", (B * L, H))
        probs = c.late(torch.softmax(rnd(4, B * heads * L, npad), dim=-1))
    else:
        nat, trn, out = c.late(V.reshape(B * N, H)), None, None
        probs = c.out("dP", (B * heads * L, npad))
    c.call = lambda s: ctx.lib.pnp_op_xattn(0, mode, p(nat), H, p(trn), B * npad, npad, p(x), H, p(out), H, p(probs), npad, B, L, N,
                                            heads, sptr(s))
    return c


for _mode in (0, 2, 1):
    for _N, _L in ((26, 1), (513, 7)):
        case(f"xattn_mode{_mode}_N{_N}_L{_L}", "pnp_op_xattn")(lambda ctx, m=_mode, n=_N, l=_L: _xattn(ctx, m, n, l))


def _mask(B, L):
    m = torch.ones(B, L, dtype=I64, device=DEV)
    m[1, L - max(1, L // 3):] = 0
    return m


def _text_attn(ctx, L, text_rows=0, probs=True):
    B, heads = 2, 2
    H = heads * 64
    c = Case(f"text_self_attn_L{L}")
    qkv, mask = c.late(rnd(1, B * L, 3 * H)), _mask(B, L)
    out = c.out("ctx", (B * L, H))
    pr = c.out("probs", (B, heads, L, L)) if probs else None
    scratch = None if probs else c.out("scratch", (B, heads, L, L))

    def call(s):
        ctx.tune("text_rows", text_rows)
        try:
            return ctx.lib.pnp_op_text_self_attn(0, p(qkv), p(mask), L, p(out), p(pr), p(scratch), B, L, H, sptr(s))
        finally:
            ctx.tune("text_rows", 0)
    c.call = call
    return c


@case("text_self_attn_L5", "pnp_op_text_self_attn")
def _(ctx):
    return _text_attn(ctx, 5)


@case("text_self_attn_L85_rows3", "pnp_op_text_self_attn")
def _(ctx):
    return _text_attn(ctx, 85, text_rows=3)


@case("text_self_attn_L193_scratch", "pnp_op_text_self_attn")
def _(ctx):
    return _text_attn(ctx, 193, probs=False)


def _text_attn_bwd(ctx, L, text_rows=0):
    B, heads = 2, 2
    H = heads * 64
    c = Case(f"text_self_attn_bwd_L{L}")
    qkv, dctx = c.late(rnd(1, B * L, 3 * H)), c.late(rnd(2, B * L, H))
    probs = c.late(torch.softmax(rnd(3, B, heads, L, L), dim=-1))
    ds, dqkv = c.out("ds_scratch", (B, heads, L, L)), c.out("dqkv", (B * L, 3 * H))

    def call(s):
        ctx.tune("text_rows", text_rows)
        try:
            return ctx.lib.pnp_op_text_self_attn_bwd(0, p(qkv), p(dctx), p(probs), p(ds), p(dqkv), B, L, H, sptr(s))
        finally:
            ctx.tune("text_rows", 0)
    c.call = call
    return c


@case("text_self_attn_bwd_L85_rows2", "pnp_op_text_self_attn_bwd")
def _(ctx):
    return _text_attn_bwd(ctx, 85, text_rows=2)


@case("text_self_attn_bwd_L193", "pnp_op_text_self_attn_bwd")
def _(ctx):
    return _text_attn_bwd(ctx, 193)


@case("text_embed", "pnp_op_text_embed")
def _(ctx):
    B, L, H, vocab, ld = 2, 7, 128, 50, 9
    c = Case("text_embed")
    ids = torch.randint(0, vocab, (B, ld), device=DEV, dtype=I64, generator=torch.Generator(device=DEV).manual_seed(1))
    word, pos = c.late(rnd(2, vocab, H)), c.late(rnd(3, L, H))
    out = c.out("out", (B, L, H))
    c.call = lambda s: ctx.lib.pnp_op_text_embed(p(ids), ld, p(word), p(pos), p(out), B, L, H, vocab - 1, vocab, sptr(s))
    return c


@case("itm_head", "pnp_op_itm_head")
def _(ctx):
    B, L, H = 3, 5, 128
    c = Case("itm_head")
    h, w, b = c.late(rnd(1, B, L, H)), c.late(rnd(2, 2, H)), c.late(rnd(3, 2))
    out = c.out("logits", (B, 2))
    c.call = lambda s: ctx.lib.pnp_op_itm_head(p(h), p(w), p(b), p(out), B, L, H, sptr(s))
    return c


@case("itm_grad_seed", "pnp_op_itm_grad_seed")
def _(ctx):
    B, L, H = 3, 5, 128
    c = Case("itm_grad_seed")
    w = c.late(rnd(2, 2, H))
    out = c.out("dh", (B, L, H))
    c.call = lambda s: ctx.lib.pnp_op_itm_grad_seed(p(w), p(out), B, L, H, sptr(s))
    return c


@case("patchify_dropped", "pnp_op_patchify")
def _(ctx):
    B, P = 2, 2
    S = 16 * P
    c = Case("patchify_dropped")
    img = c.late(rnd(1, B, 3, S, S))
    dropped = torch.tensor([[0, 1, 0, 0], [1, 0, 0, 1]], dtype=U8, device=DEV)
    out = c.out("out", (B * P * P, 768))
    c.call = lambda s: ctx.lib.pnp_op_patchify(0, p(img), p(dropped), p(out), B, S, P, sptr(s))
    return c


@case("cls_rows", "pnp_op_cls_rows")
def _(ctx):
    B, N, D = 3, 5, 128
    c = Case("cls_rows")
    cls, pos = c.late(rnd(1, D)), c.late(rnd(2, N, D))
    x = c.out("x", (B, N, D))
    c.call = lambda s: ctx.lib.pnp_op_cls_rows(p(cls), p(pos), p(x), B, N, D, sptr(s))
    return c


@case("split", "pnp_op_split")
def _(ctx):
    c = Case("split")
    x = c.late(rnd(1, 257))
    hi, lo = c.out("hi", (257,), BF), c.out("lo", (257,), BF)
    c.call = lambda s: ctx.lib.pnp_op_split(p(x), p(hi), p(lo), 257, sptr(s))
    return c


@case("cast", "pnp_op_cast")
def _(ctx):
    c = Case("cast")
    x = c.late(rnd(1, 257))
    out = c.out("out", (257,), BF)
    c.call = lambda s: ctx.lib.pnp_op_cast(1, p(x), p(out), 257, sptr(s))
    return c


@case("sort_pairs", "pnp_op_sort_pairs", may_block=True)
def _(ctx):
    n = 4097
    c = Case("sort_pairs")
    g = torch.Generator(device=DEV).manual_seed(1)
    keys = torch.randint(0, 1 << 40, (n,), device=DEV, dtype=I64, generator=g)
    vals = torch.arange(n, device=DEV, dtype=I32)
    # every 64-bit pattern is a valid key and every value is carried, not used: both may arrive late
    kin, vin = c.late(keys, early=keys.flip(0) ^ 0x5555), c.late(vals, early=vals.flip(0))
    kout, vout = c.out("keys_out", (n,), I64), c.out("vals_out", (n,), I32)
    seg = (C.c_size_t * 3)(0, 2000, n)
    c.call = lambda s: ctx.lib.pnp_op_sort_pairs(p(kin), p(kout), p(vin), p(vout), n, 0, 40, C.cast(seg, C.c_void_p), 2, sptr(s))
    return c


@case("scan_i32", "pnp_op_scan_i32", may_block=True)
def _(ctx):
    n = 8193
    c = Case("scan_i32")
    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randint(0, 9, (n,), device=DEV, dtype=I32, generator=g)
    xin = c.late(x, early=x.flip(0) + 1)
    out = c.out("out", (n,), I32)
    c.call = lambda s: ctx.lib.pnp_op_scan_i32(p(xin), p(out), n, 1, sptr(s))
    return c


@case("itc_similarity", "pnp_itc_similarity")
def _(ctx):
    B, T, E = 3, 5, 256
    c = Case("itc_similarity")
    a, b = c.late(rnd(1, B, E)), c.late(rnd(2, T, E))
    out = c.out("sim", (B, T))
    c.call = lambda s: ctx.lib.pnp_itc_similarity(p(a), p(b), B, T, E, p(out), sptr(s))
    return c


# ================================================================================================ input and output side
@case("preprocess_images", "pnp_preprocess_images")
def _(ctx):
    from pnp_ovss import hip
    import _post_refs as PR
    S = 32
    images = [PR.photo_like(24, 40, 1), PR.photo_like(33, 45, 2)]
    B = len(images)
    desc = (hip.PnpPreImage * B)()
    parts, coef_off, src_off, tmp_off, seen = [], 0, 0, 0, {}
    for i, im in enumerate(images):
        H, W = im.shape[:2]
        for n in (W, H):
            if n not in seen:
                tab, ks = hip.resample_table(n, S)
                seen[n] = (coef_off, ks)
                parts.append(tab.reshape(-1))
                coef_off += tab.size
        desc[i] = hip.PnpPreImage(src_off, tmp_off, H, W, seen[W][0], seen[W][1], seen[H][0], seen[H][1])
        src_off += H * W * 3
        tmp_off += H * S * 3
    c = Case("preprocess_images")
    rgb = c.late(dev(np.concatenate([im.reshape(-1) for im in images])))
    coef, d_desc = dev(np.concatenate(parts)), up(desc)
    tmp, out = c.out("tmp", (tmp_off,), U8), c.out("out", (B, 3, S, S))
    m3, s3 = (C.c_float * 3)(0.48, 0.45, 0.40), (C.c_float * 3)(0.26, 0.26, 0.27)
    c.keep = (coef, d_desc, desc)
    c.call = lambda s: ctx.lib.pnp_preprocess_images(p(rgb), p(d_desc), B, S, 33, p(coef), p(tmp), m3, s3, p(out), sptr(s))
    return c


@case("jpeg_decode", "pnp_jpeg_decode")
def _(ctx):
    """One 4:2:0 file with restart intervals.  The entropy-coded bytes and every table are valid from the start."""
    from pnp_ovss import jpeg as J
    import _jpeg_streams as JS
    data, imgs, tabs, segs, sizes, tot = J.pack_batch([JS.recode(JS.source(24, 40, "420", 90, seed=3), dri=2)])
    c = Case("jpeg_decode")
    d_data, d_imgs, d_tabs, d_segs = dev(data), up(imgs), up(tabs), up(segs)
    clean, bits = c.out("d_clean", (tot["clean_bytes"],), U8), c.out("d_seg_bits", (len(segs),), I32)
    coef, planes = c.out("d_coef", (tot["coef_elems"],), torch.int16), c.out("d_planes", (tot["plane_bytes"],), U8)
    rgb = c.out("d_rgb", (tot["rgb_bytes"],), U8)
    err = c.out("d_err", (1,), I32, init=torch.zeros(1, dtype=I32), may_stay=True)
    c.call = lambda s: ctx.lib.pnp_jpeg_decode(p(d_data), p(d_imgs), p(d_tabs), p(d_segs), 1, len(segs), p(clean), p(bits), p(coef),
                                               tot["coef_elems"], p(planes), p(rgb), tot["max_blocks"], tot["max_pixels"], p(err), sptr(s))
    c.after = lambda: int(err.item()) == 0
    return c


def _jpeg_scans(ctx, timed):
    """One progressive 24 x 40 file.  Without h_group_ms the call is not documented to hold the host; with it, it is."""
    from pnp_ovss import jpeg as J
    import _jpeg_progressive as JP
    src = JP.small_source("420", 24, 40)
    data, imgs, tabs, scans, segs, groups, sizes, tot = J.pack_scans([JP.recode_progressive(src, JP.pillow_script(3))])
    groups = np.ascontiguousarray(groups, dtype=np.int32)
    c = Case("jpeg_decode_scans_timed" if timed else "jpeg_decode_scans")
    group_ms = np.zeros(len(groups), dtype=np.float32)
    d_data, d_imgs, d_tabs, d_scans, d_segs = dev(data), up(imgs), up(tabs), up(scans), up(segs)
    clean, bits = c.out("d_clean", (tot["clean_bytes"],), U8), c.out("d_seg_bits", (len(segs),), I32)
    coef, hist = c.out("d_coef", (tot["coef_elems"],), torch.int16), c.out("d_hist", (tot["coef_elems"] // 64,), I64)
    planes, rgb = c.out("d_planes", (tot["plane_bytes"],), U8), c.out("d_rgb", (tot["rgb_bytes"],), U8)
    err = c.out("d_err", (1,), I32, init=torch.zeros(1, dtype=I32), may_stay=True)
    c.keep = (groups, group_ms)
    c.call = lambda s: ctx.lib.pnp_jpeg_decode_scans(
        p(d_data), p(d_imgs), p(d_tabs), p(d_scans), p(d_segs), 1, len(scans), len(segs), tot["base_segments"], groups.ctypes.data,
        len(groups), p(clean), p(bits), p(coef), tot["coef_elems"], p(hist), p(planes), p(rgb), tot["max_blocks"], tot["max_pixels"],
        None, group_ms.ctypes.data if timed else None, p(err), sptr(s))
    c.after = lambda: int(err.item()) == 0
    return c


@case("jpeg_decode_scans", "pnp_jpeg_decode_scans")
def _(ctx):
    return _jpeg_scans(ctx, False)


@case("jpeg_decode_scans_timed", "pnp_jpeg_decode_scans", may_block=True)
def _(ctx):
    return _jpeg_scans(ctx, True)


OUT_SIZES = ((17, 33), (24, 40))


@case("jpeg_encode", "pnp_jpeg_encode")
def _(ctx):
    from pnp_ovss import hip, jpeg as J
    import _post_refs as PR
    images = [PR.photo_like(h, w, 3 + i) for i, (h, w) in enumerate(OUT_SIZES)]
    B = len(images)
    quant = np.ascontiguousarray(J.quality_tables(75))
    desc = (hip.PnpJpegEncImage * B)()
    ro = oo = 0
    for i, (h, w) in enumerate(OUT_SIZES):
        cap = J.scan_capacity(h, w)
        desc[i] = hip.PnpJpegEncImage(ro, oo, h, w, cap, 0)
        ro, oo = ro + h * w * 3, oo + cap
    need = C.c_int64()
    assert ctx.lib.pnp_jpeg_encode(None, desc, B, quant.ctypes.data, None, None, None, None, 0, C.byref(need), None) == 0
    c = Case("jpeg_encode")
    rgb = c.late(dev(np.concatenate([im.reshape(-1) for im in images])))
    ws, out = c.out("d_ws", (need.value,), U8), c.out("d_out", (oo,), U8)
    lens, err = c.out("d_out_len", (B,), I32), c.out("d_err", (1,), I32)
    c.keep = (desc, quant)
    c.call = lambda s: ctx.lib.pnp_jpeg_encode(p(rgb), desc, B, quant.ctypes.data, p(out), p(lens), p(err), p(ws), need.value, None, sptr(s))
    c.after = lambda: int(err.item()) == 0 and int(lens.min()) > 0
    return c


@case("png_encode", "pnp_png_encode")
def _(ctx):
    from pnp_ovss import hip, png as PN
    rng = np.random.default_rng(5)
    maps = [np.repeat(rng.integers(0, 21, size=(h, (w + 3) // 4)), 4, axis=1)[:, :w].astype(np.uint8) for h, w in OUT_SIZES]
    B = len(maps)
    desc = (hip.PnpPngImage * B)()
    lo = oo = 0
    for i, (h, w) in enumerate(OUT_SIZES):
        cap = PN.stream_capacity(h, w)
        desc[i] = hip.PnpPngImage(lo, oo, h, w, cap, 0)
        lo, oo = lo + h * w, oo + cap
    need = C.c_int64()
    assert ctx.lib.pnp_png_encode(None, desc, B, None, None, None, None, 0, C.byref(need), None) == 0
    c = Case("png_encode")
    flat = dev(np.concatenate([m.reshape(-1) for m in maps]))
    labels = c.late(flat, early=(flat + 7) % 21)
    ws, out = c.out("d_ws", (need.value,), U8), c.out("d_out", (oo,), U8)
    lens, err = c.out("d_out_len", (B,), I32), c.out("d_err", (1,), I32)
    c.keep = desc
    c.call = lambda s: ctx.lib.pnp_png_encode(p(labels), desc, B, p(out), p(lens), p(err), p(ws), need.value, None, sptr(s))
    c.after = lambda: int(err.item()) == 0 and int(lens.min()) > 0
    return c


@case("overlay_labels", "pnp_overlay_labels")
def _(ctx):
    import _post_refs as PR
    rng = np.random.default_rng(6)
    c = Case("overlay_labels")
    lab = dev(np.concatenate([rng.integers(0, 21, size=h * w) for h, w in OUT_SIZES]).astype(np.uint8))
    labels = c.late(lab, early=(lab + 7) % 21)
    rgb = c.late(dev(np.concatenate([PR.photo_like(h, w, 8 + i).reshape(-1) for i, (h, w) in enumerate(OUT_SIZES)])))
    off = torch.tensor([0, 17 * 33, 17 * 33 + 24 * 40], dtype=I64, device=DEV)
    pal = dev(rng.integers(0, 256, size=768).astype(np.uint8))
    out = c.out("out", (rgb.numel(),), U8)
    c.call = lambda s: ctx.lib.pnp_overlay_labels(p(labels), p(rgb), p(off), 2, p(pal), 0.3, p(out), sptr(s))
    return c


# ================================================================================================ engine
ENG_B, ENG_HEAD = 2, 1


class _Engine:
    """blip_itm_small(128) in the benchmarked mode with synthetic weights, B = 2 captions of 4 and 2 classes, and one prepared
    post-processing batch of sizes (24, 40) and (33, 45)."""

    def __init__(self):
        from pnp_ovss import config, synth
        from pnp_ovss.hip import Engine
        import _post_refs as PR
        cfg = config.blip_itm_small(128)
        W = synth.synth_state_dict(cfg, 3)
        W.update(synth.itc_state_dict(cfg, 3))
        self.cfg = cfg
        self.e = Engine(cfg, max_batch=ENG_B, max_text_len=16, stash_layer=7, mode="bf16x3")
        self.e.load_state_dict(W)
        _, imgs = synth.synth_images(ENG_B, cfg.img_size, seed=5)
        ids, mask = synth.synth_tokens(cfg, [4, 2], seed=1)
        self.images = dev(imgs, F32)
        self.ids, self.mask = dev(ids), dev(mask)
        self.ld, self.L = int(ids.shape[1]), int(mask.sum(1).max())
        self.G = cfg.grid
        self.post = PR.Case([(24, 40), (33, 45)], [3, 2], [True, True], seed=11)
        pix = [h * w for h, w in self.post.sizes]
        self.e.post_reserve(ENG_B, sum(pix), max(pix), max(self.post.K), 0)
        self.rgb = dev(np.concatenate([r.reshape(-1) for r in self.post.rgb]))
        self.gt = dev(np.concatenate([g.reshape(-1) for g in self.post.gts]))
        self.total = sum(pix)
        self.prepare(self.rgb, self.gt)
        torch.cuda.synchronize()

    def prepare(self, rgb, gt):
        c = self.post
        self.e.post_prepare(c.sizes, c.plans, c.luts, c.has_bg, rgb=rgb, gt=gt, want_crf=True)

    def own(self, c, *names, fill=0xA5, dtype=F32):
        """Engine.buffer(name) of every name as a probe; a name pnp_get_buffer does not know is an error of the case."""
        for n in names:
            c.own(n, self.e.buffer(n, dtype), fill)


def _h(E):
    return E.e.lib, E.e.h


@case("vit_forward", "pnp_vit_forward")
def _(ctx):
    E = ctx.engine
    lib, h = _h(E)
    c = Case("vit_forward")
    images = c.late(E.images)
    drop = torch.zeros(ENG_B, E.G * E.G, dtype=U8, device=DEV)
    drop[0, 3] = drop[1, 10] = drop[1, 11] = 1
    dropped = c.late(drop, early=1 - drop)
    E.own(c, "image_embeds", "x")
    E.own(c, "Kt", "Vt", fill=0, dtype=U8)                                  # (their pad columns are zero from pnp_create on)
    c.call = lambda s: lib.pnp_vit_forward(h, p(images), p(dropped), ENG_B, sptr(s))
    return c


@case("cross_kv", "pnp_cross_kv")
def _(ctx):
    E = ctx.engine
    lib, h = _h(E)
    c = Case("cross_kv")
    E.own(c, "Kt", "Vt", fill=0, dtype=U8)
    c.setup = lambda: E.e.vit_forward(E.images)
    c.call = lambda s: lib.pnp_cross_kv(h, ENG_B, sptr(s))
    return c


@case("text_forward_grad_gather", "pnp_text_forward_xattn", "pnp_xattn_grad_layer", "pnp_gradcam_gather")
def _(ctx):
    E = ctx.engine
    lib, h = _h(E)
    c = Case("text_forward_grad_gather")
    logits, cam = c.out("logits", (ENG_B, 2)), c.out("gradcam", (ENG_B, E.L - 1, E.G, E.G))
    E.own(c, "P", "dP", "text_hidden", "dq_xattn", "dctx_xattn", dtype=U8)
    c.setup = lambda: E.e.vit_forward(E.images)

    def call(s):
        return (lib.pnp_text_forward_xattn(h, p(E.ids), p(E.mask), E.ld, ENG_B, E.L, p(logits), sptr(s)) or
                lib.pnp_xattn_grad_layer(h, ENG_B, E.L, 7, sptr(s)) or
                lib.pnp_gradcam_gather(h, p(E.mask), E.ld, ENG_B, E.L, ENG_HEAD, p(cam), sptr(s)))
    c.call = call
    return c


@case("compute_gradcam", "pnp_compute_gradcam_layer")
def _(ctx):
    E = ctx.engine
    lib, h = _h(E)
    c = Case("compute_gradcam")
    images = c.late(E.images)
    cam, logits = c.out("gradcam", (ENG_B, E.L - 1, E.G, E.G)), c.out("logits", (ENG_B, 2))
    E.own(c, "image_embeds", "P", "dP", dtype=U8)
    c.call = lambda s: lib.pnp_compute_gradcam_layer(h, p(images), None, p(E.ids), p(E.mask), E.ld, ENG_B, E.L, 7, ENG_HEAD, p(cam),
                                                     p(logits), sptr(s))
    return c


@case("drop_step", "pnp_drop_step")
def _(ctx):
    """Two bookkeeping steps (iter 0 sets g0, iter 1 adds to the running sum) on gathered maps that arrive late."""
    E = ctx.engine
    lib, h = _h(E)
    T, PP, npick = E.L - 1, E.G * E.G, 10
    c = Case("drop_step")
    g_a, g_b = c.late(rnd(1, ENG_B, T, E.G, E.G).abs()), c.late(rnd(2, ENG_B, T, E.G, E.G).abs())
    g0, agg = c.out("g0", (ENG_B, T, E.G, E.G)), c.out("agg", (ENG_B, T, E.G, E.G), init=torch.zeros(ENG_B, T, E.G, E.G))
    dropped = c.out("dropped", (ENG_B, PP), U8, init=torch.zeros(ENG_B, PP, dtype=U8))
    picks = c.out("picks", (ENG_B, 2 * npick), I32, init=torch.full((ENG_B, 2 * npick), -1, dtype=I32))
    c.call = lambda s: (lib.pnp_drop_step(h, p(g_a), p(g0), p(agg), p(dropped), p(picks), 0, ENG_B, T, npick, 2 * npick, sptr(s)) or
                        lib.pnp_drop_step(h, p(g_b), p(g0), p(agg), p(dropped), p(picks), 1, ENG_B, T, npick, 2 * npick, sptr(s)))
    return c


@case("drop_loop", "pnp_drop_loop_layer")
def _(ctx):
    E = ctx.engine
    lib, h = _h(E)
    npick, iters = 10, 2
    shape = (ENG_B, E.L - 1, E.G, E.G)
    c = Case("drop_loop")
    images = c.late(E.images)
    g0, agg, logits = c.out("g0", shape), c.out("agg", shape), c.out("logits", (ENG_B, 2))
    picks = c.out("picks", (ENG_B, iters * npick), I32, init=torch.full((ENG_B, iters * npick), -1, dtype=I32))
    E.own(c, "image_embeds", dtype=U8)
    c.call = lambda s: lib.pnp_drop_loop_layer(h, p(images), p(E.ids), p(E.mask), E.ld, ENG_B, E.L, 7, ENG_HEAD, iters, npick, p(g0),
                                               p(agg), p(picks), p(logits), sptr(s))
    return c


@case("text_only_and_project", "pnp_text_forward_text", "pnp_project_normalize")
def _(ctx):
    E = ctx.engine
    lib, h = _h(E)
    Hd, D, N = E.cfg.txt_hidden, E.cfg.vit_dim, E.G * E.G + 1
    c = Case("text_only_and_project")
    hid, tf, vf = c.out("hidden", (ENG_B, E.L, Hd)), c.out("text_feat", (ENG_B, 256)), c.out("image_feat", (ENG_B, 256))
    emb = E.e.buffer("image_embeds")
    c.setup = lambda: E.e.vit_forward(E.images)
    c.call = lambda s: (lib.pnp_text_forward_text(h, p(E.ids), p(E.mask), E.ld, ENG_B, E.L, p(hid), sptr(s)) or
                        lib.pnp_project_normalize(h, 1, p(hid), E.L * Hd, ENG_B, p(tf), sptr(s)) or
                        lib.pnp_project_normalize(h, 0, p(emb), N * D, ENG_B, p(vf), sptr(s)))
    return c


@case("post_prepare", "pnp_post_prepare", may_block=True)
def _(ctx):
    """rgb and gt late.  Only the bilateral normaliser is probed with a sentinel: that lattice is built on every call, the
    Gaussian one is kept between batches of the same sizes.  The index tables of both lattices are compared as the build left
    them (never armed: the mean-field addresses through them).  The labels of a blur + CRF run behind the call (the read-out)
    show which pixels the build saw."""
    E = ctx.engine
    lib, h = _h(E)
    c = Case("post_prepare")
    rgb, gt = c.late(E.rgb), c.late(E.gt)
    cam = dev(E.post.maps)
    labels = c.out("labels", (E.total,), U8)
    hist = c.out("hist", (21 * 21,), I64, init=torch.zeros(21 * 21, dtype=I64))
    E.own(c, "crf_norm_bilateral")
    E.own(c, "crf_norm_gauss", fill=None)
    E.own(c, "crf_offset_bilateral", "crf_offset_gauss", "crf_idbase_bilateral", "crf_idbase_gauss", fill=None, dtype=I32)
    E.own(c, "crf_nbr8_bilateral", "crf_nbr8_gauss", fill=None, dtype=U8)

    def call(s):
        with torch.cuda.stream(s):                                          # (None: the current stream stays, the default one)
            E.prepare(rgb, gt)
        return 0
    c.call = call
    c.readout = lambda s: lib.pnp_postprocess(h, p(cam), cam.shape[1], 0.15, 1, 3, p(labels), p(hist), 21, sptr(s))
    c.restore = lambda: E.prepare(E.rgb, E.gt)                              # the later cases read the module's own rgb / gt
    return c


def _post_stage(ctx, name, upto):
    """One stage of the prepared batch; the stages in front of it run in setup(), on the default stream."""
    E = ctx.engine
    lib, h = _h(E)
    c = Case(name)
    cam_real = dev(E.post.maps)
    T = cam_real.shape[1]
    stages = [lambda s, g: lib.pnp_merge_tokens(h, p(g), T, sptr(s)),
              lambda s, g: lib.pnp_threshold_upsample(h, 0.15, 1, sptr(s)),
              lambda s, g: lib.pnp_blur_minmax(h, sptr(s)),
              lambda s, g: lib.pnp_densecrf(h, 3, 7.0, 3.0, 10.0, 50.0, 5.0, sptr(s))]

    def setup():
        for st in stages[:upto]:
            assert st(None, cam_real) == 0
    c.setup = setup
    return c, cam_real, stages


@case("merge_tokens", "pnp_merge_tokens")
def _(ctx):
    c, cam_real, stages = _post_stage(ctx, "merge_tokens", 0)
    cam = c.late(cam_real)
    ctx.engine.own(c, "merged")
    c.call = lambda s: stages[0](s, cam)
    return c


@case("threshold_upsample", "pnp_threshold_upsample")
def _(ctx):
    c, cam_real, stages = _post_stage(ctx, "threshold_upsample", 1)
    ctx.engine.own(c, "maps", "maps_pre_blur")
    c.call = lambda s: stages[1](s, None)
    return c


@case("blur_minmax", "pnp_blur_minmax")
def _(ctx):
    c, cam_real, stages = _post_stage(ctx, "blur_minmax", 2)
    c.setup()
    assert stages[2](None, None) == 0                                       # "maps" names the blurred maps from here on
    torch.cuda.synchronize()
    ctx.engine.own(c, "maps")
    c.call = lambda s: stages[2](s, None)
    return c


@case("densecrf", "pnp_densecrf")
def _(ctx):
    c, cam_real, stages = _post_stage(ctx, "densecrf", 3)
    ctx.engine.own(c, "unary", "crf_q")
    c.call = lambda s: stages[3](s, None)
    return c


@case("remap_hist", "pnp_remap_hist")
def _(ctx):
    E = ctx.engine
    lib, h = _h(E)
    c, cam_real, stages = _post_stage(ctx, "remap_hist", 4)
    labels = c.out("labels", (E.total,), U8)
    hist = c.out("hist", (21 * 21,), I64, init=torch.zeros(21 * 21, dtype=I64))
    c.call = lambda s: lib.pnp_remap_hist(h, 1, p(labels), p(hist), 21, sptr(s))
    return c


@case("postprocess_blur_crf", "pnp_postprocess")
def _(ctx):
    E = ctx.engine
    lib, h = _h(E)
    c = Case("postprocess_blur_crf")
    cam = c.late(dev(E.post.maps))
    labels = c.out("labels", (E.total,), U8)
    hist = c.out("hist", (21 * 21,), I64, init=torch.zeros(21 * 21, dtype=I64))
    E.own(c, "merged", "maps", "maps_pre_blur", "unary", "crf_q")
    c.call = lambda s: lib.pnp_postprocess(h, p(cam), cam.shape[1], 0.15, 1, 3, p(labels), p(hist), 21, sptr(s))
    return c


@case("postprocess_pair", "pnp_postprocess_pair")
def _(ctx):
    E = ctx.engine
    lib, h = _h(E)
    c = Case("postprocess_pair")
    cam1, camn = c.late(dev(E.post.maps)), c.late(dev(E.post.maps_n))
    l1, ln = c.out("labels_1drop", (E.total,), U8), c.out("labels_ndrop", (E.total,), U8)
    h1 = c.out("hist_1drop", (21 * 21,), I64, init=torch.zeros(21 * 21, dtype=I64))
    hn = c.out("hist_ndrop", (21 * 21,), I64, init=torch.zeros(21 * 21, dtype=I64))
    E.own(c, "merged", "unary", "crf_q")
    c.call = lambda s: lib.pnp_postprocess_pair(h, p(cam1), p(camn), cam1.shape[1], 0.15, 1, p(l1), p(h1), p(ln), p(hn), 21, sptr(s))
    return c


# ================================================================================================ stand-alone CRF
class _Crf:
    """Case 2 of _crf_terms_ref.CASES: K = 3 labels on 13 x 17 pixels, a 2-axis and a 4-axis term; one two-term solver and one
    feature-term solver with the gradient workspace.  Term 1 of the feature solver has a (K, K) compatibility."""

    def __init__(self):
        from pnp_ovss import crf, hip
        import _crf_terms_ref as T3
        (K, H, W), names, weights = T3.CASES[2]
        U, feats = T3.case_inputs((K, H, W), names)
        rgb, _ = T3.T.inputs(K, H, W)
        self.K, self.H, self.W, self.n = K, H, W, H * W
        self.U, self.rgb = dev(U.copy()), dev(rgb.copy())
        self.feats = [dev(f.copy()).reshape(-1) for f in feats]
        self.dims = [int(f.shape[0]) for f in feats]
        self.weights = (C.c_float * 2)(*[float(w) for w in weights])
        self.two = crf.DenseCRF(1, self.n, self.n, K)
        self.terms = crf.FeatureCRF(1, self.n, self.n, K, max_terms=2, max_dims=4)
        assert self.terms.lib.pnp_crf_reserve_grad(self.terms.h) == 0
        M = (np.eye(K, dtype=np.float32) * 6 + np.float32(0.5)).astype(np.float32)
        self.terms.set_compat([None, M])
        self.lib = hip.load_library()
        self.hw = [np.array([v], dtype=np.int32) for v in (H, W, K)]
        self.q_floats = self.n * ((K + 3) // 4 * 4)

    def batch(self, unary, rgb=None):
        from pnp_ovss import hip
        return hip.PnpCrfBatch(1, hip._i32p(self.hw[0]), hip._i32p(self.hw[1]), hip._i32p(self.hw[2]), p(rgb), p(unary))

    def set_two(self, unary, rgb, s=None):
        return self.lib.pnp_crf_set_batch(self.two.h, C.byref(self.batch(unary, rgb)), 3.0, 50.0, 5.0, sptr(s))

    def set_terms(self, unary, feats, s=None):
        from pnp_ovss import hip
        arr = (hip.PnpCrfTerm * 2)(*[hip.PnpCrfTerm(d, p(f)) for d, f in zip(self.dims, feats)])
        return self.lib.pnp_crf_set_batch_terms(self.terms.h, C.byref(self.batch(unary)), 2, arr, sptr(s))

    def outs(self, c):
        return c.out("q", (self.K, self.n)), c.out("labels", (self.n,), U8)


@case("crf_set_batch", "pnp_crf_set_batch", may_block=True)
def _(ctx):
    """set_batch alone is under test; the infer behind it is the read-out of the lattices and of the unary copy it made."""
    X = ctx.crf
    c = Case("crf_set_batch")
    U, rgb = c.late(X.U), c.late(X.rgb)
    q, lab = X.outs(c)
    c.call = lambda s: X.set_two(U, rgb, s)
    c.readout = lambda s: X.lib.pnp_crf_infer(X.two.h, 3, 7.0, 10.0, p(q), p(lab), sptr(s))
    return c


@case("crf_set_batch_aniso", "pnp_crf_set_batch_aniso", may_block=True)
def _(ctx):
    X = ctx.crf
    c = Case("crf_set_batch_aniso")
    U, rgb = c.late(X.U), c.late(X.rgb)
    q, lab = X.outs(c)
    f2, f3 = (C.c_float * 2), (C.c_float * 3)
    c.call = lambda s: X.lib.pnp_crf_set_batch_aniso(X.two.h, C.byref(X.batch(U, rgb)), f2(3.0, 4.0), f2(50.0, 40.0), f3(5.0, 6.0, 7.0),
                                                     sptr(s))
    c.readout = lambda s: X.lib.pnp_crf_infer(X.two.h, 3, 7.0, 10.0, p(q), p(lab), sptr(s))
    return c


def _two_ready(X):
    def setup():
        assert X.set_two(X.U, X.rgb) == 0
    return setup


@case("crf_infer", "pnp_crf_infer")
def _(ctx):
    """The batch is set on the default stream beforehand: the start, the Potts updates, the label output fused into the last
    one and the marginals out are all issued behind the blocker."""
    X = ctx.crf
    c = Case("crf_infer")
    q, lab = X.outs(c)
    c.setup = _two_ready(X)
    c.call = lambda s: X.lib.pnp_crf_infer(X.two.h, 3, 7.0, 10.0, p(q), p(lab), sptr(s))
    return c


@case("crf_start_step_read", "pnp_crf_start", "pnp_crf_step", "pnp_crf_read")
def _(ctx):
    X = ctx.crf
    c = Case("crf_start_step_read")
    q, lab = X.outs(c)
    c.setup = _two_ready(X)
    c.call = lambda s: (X.lib.pnp_crf_start(X.two.h, sptr(s)) or X.lib.pnp_crf_step(X.two.h, 2, 7.0, 10.0, sptr(s)) or
                        X.lib.pnp_crf_read(X.two.h, p(q), p(lab), sptr(s)))
    return c


@case("crf_step_matrix", "pnp_crf_start", "pnp_crf_step", "pnp_crf_read")
def _(ctx):
    """The bilateral term as a (K, K) matrix, the Gaussian one left scalar: pnp_crf_step then runs the compatibility kernel and
    uploads the scalar term as w I from pageable host memory (crf_matrices) -- once per weight, so setup() steps with another
    weight first and the call under test has to upload again.  The solver goes back to Potts afterwards."""
    X = ctx.crf
    c = Case("crf_step_matrix")
    q, lab = X.outs(c)
    M = (np.eye(X.K, dtype=np.float32) * 9 + np.float32(0.5)).astype(np.float32)

    def setup():
        assert X.lib.pnp_crf_set_compat(X.two.h, 1, 2, M.ctypes.data_as(C.POINTER(C.c_float)), X.K) == 0
        assert X.set_two(X.U, X.rgb) == 0 and X.lib.pnp_crf_start(X.two.h, None) == 0
        assert X.lib.pnp_crf_step(X.two.h, 1, 5.0, 10.0, None) == 0
    c.setup = setup
    c.call = lambda s: (X.lib.pnp_crf_start(X.two.h, sptr(s)) or X.lib.pnp_crf_step(X.two.h, 2, 7.0, 10.0, sptr(s)) or
                        X.lib.pnp_crf_read(X.two.h, p(q), p(lab), sptr(s)))

    def restore():
        assert X.lib.pnp_crf_set_compat(X.two.h, 1, 0, None, 0) == 0
    c.restore = restore
    return c


@case("crf_kl", "pnp_crf_kl", may_block=True)
def _(ctx):
    """The result is host memory: it is copied into a probed device word behind the call, which has synchronised by then."""
    X = ctx.crf
    c = Case("crf_kl")
    out = c.out("kl", (1,), torch.float64)
    host = (C.c_double * 1)()

    def setup():
        assert X.set_two(X.U, X.rgb) == 0 and X.lib.pnp_crf_start(X.two.h, None) == 0
        assert X.lib.pnp_crf_step(X.two.h, 2, 7.0, 10.0, None) == 0
    c.setup = setup

    def call(s):
        r = X.lib.pnp_crf_kl(X.two.h, 7.0, 10.0, host, sptr(s))
        out.copy_(torch.tensor([host[0]], dtype=torch.float64))
        return r
    c.call = call
    return c


@case("crf_probe_filter", "pnp_crf_probe_filter")
def _(ctx):
    X = ctx.crf
    c = Case("crf_probe_filter")
    planes = c.late(torch.softmax(-X.U, dim=0))
    out = c.out("message", (X.K, X.n))

    def setup():
        assert X.set_two(X.U, X.rgb) == 0
    c.setup = setup
    c.call = lambda s: X.lib.pnp_crf_probe_filter(X.two.h, 1, 3, p(planes), p(out), sptr(s))
    return c


@case("crf_set_batch_terms", "pnp_crf_set_batch_terms", may_block=True)
def _(ctx):
    """set_batch_terms alone is under test; the infer_terms behind it is the read-out of the lattices it built."""
    X = ctx.crf
    c = Case("crf_set_batch_terms")
    U = c.late(X.U)
    feats = [c.late(f, early=f * 0.5 + 0.125) for f in X.feats]              # other finite features well inside the key range
    q, lab = X.outs(c)
    c.call = lambda s: X.set_terms(U, feats, s)
    c.readout = lambda s: X.lib.pnp_crf_infer_terms(X.terms.h, 3, X.weights, p(q), p(lab), sptr(s))
    return c


@case("crf_infer_terms", "pnp_crf_infer_terms")
def _(ctx):
    X = ctx.crf
    c = Case("crf_infer_terms")
    q, lab = X.outs(c)

    def setup():
        assert X.set_terms(X.U, X.feats) == 0
    c.setup = setup
    c.call = lambda s: X.lib.pnp_crf_infer_terms(X.terms.h, 3, X.weights, p(q), p(lab), sptr(s))
    return c


@case("crf_step_terms", "pnp_crf_step_terms")
def _(ctx):
    X = ctx.crf
    c = Case("crf_step_terms")
    q, lab = X.outs(c)

    def setup():
        assert X.set_terms(X.U, X.feats) == 0
    c.setup = setup
    c.call = lambda s: (X.lib.pnp_crf_start(X.terms.h, sptr(s)) or X.lib.pnp_crf_step_terms(X.terms.h, 2, X.weights, sptr(s)) or
                        X.lib.pnp_crf_read(X.terms.h, p(q), p(lab), sptr(s)))
    return c


@case("crf_marginals_forward_backward", "pnp_crf_infer_terms_saved", "pnp_crf_backward_terms")
def _(ctx):
    """What FeatureCRF.marginals and its backward issue: the saved forward, then the gradients of the unary energies, of term
    0's weight and of term 1's (K, K) compatibility from a cotangent that arrives late."""
    X = ctx.crf
    iters = 2
    c = Case("crf_marginals_forward_backward")
    gq = c.late(rnd(1, X.K, X.n))
    hist, q = c.out("history", ((iters + 1) * X.q_floats,)), c.out("q", (X.K, X.n))
    gu, g0, g1 = c.out("grad_unary", (X.K, X.n)), c.out("grad_w0", (1,)), c.out("grad_M1", (X.K * X.K,))
    ptrs = (C.c_void_p * 2)(p(g0), p(g1))

    def setup():
        assert X.set_terms(X.U, X.feats) == 0
    c.setup = setup
    c.call = lambda s: (X.lib.pnp_crf_infer_terms_saved(X.terms.h, iters, X.weights, p(hist), p(q), None, sptr(s)) or
                        X.lib.pnp_crf_backward_terms(X.terms.h, iters, X.weights, p(hist), p(gq), p(gu), ptrs, sptr(s)))
    return c


# ================================================================================================ the run
class _Ctx:
    def __init__(self):
        from pnp_ovss import hip
        self.lib = hip.load_library()
        self._engine = self._crf = None

    def tune(self, key, value):
        assert self.lib.pnp_set_tuning(key.encode(), value) == 0

    @property
    def engine(self):
        if self._engine is None:
            self._engine = _Engine()
        return self._engine

    @property
    def crf(self):
        if self._crf is None:
            self._crf = _Crf()
        return self._crf


@pytest.fixture(scope="module")
def ctx():
    c = _Ctx()
    c.tune("streamk", 0)
    yield c
    c.tune("streamk", 1)
    c.tune("text_rows", 0)
    torch.cuda.synchronize()
    if c._engine is not None:
        c._engine.e.close()
    if c._crf is not None:
        c._crf.two.close()
        c._crf.terms.close()


@pytest.fixture(scope="module")
def gate(blocker_cycles):
    return Gate(blocker_cycles, TAG)


@pytest.mark.parametrize("name", list(CASES))
def test_entry_point_stays_on_the_callers_stream(ctx, gate, name):
    """Early write, late inputs and host return of one gated call (tests/_stream_gate.py).  A case whose entry point is in
    MAY_BLOCK may hold the host; every other one must return with the blocker still running."""
    covers, build, may_block = CASES[name]
    assert not may_block or any(f in MAY_BLOCK for f in covers), "a case may hold the host only through a MAY_BLOCK entry point"
    c = build(ctx)
    try:
        rep = gate.run(c)
        torch.cuda.synchronize()
    except RuntimeError as err:
        if "HIP error" in str(err) or "hipError" in str(err):               # a device fault: nothing more is started on this GPU
            pytest.exit(f"{name}: {err}", returncode=3)
        getattr(c, "restore", lambda: None)()
        raise
    getattr(c, "restore", lambda: None)()
    rep.check(may_block=may_block)
    assert getattr(c, "after", lambda: True)(), f"{name}: the call reported an error through its outputs"


# ------------------------------------------------------------------------------------------------ the harness itself
def _two_stage(second):
    """A two-stage "operator" of torch kernels: tmp = 2 x, then out = tmp + 1.  `second(stream, fn)` issues the second stage."""
    c = Case("self_test")
    x = c.late(rnd(1, 4096))
    tmp, out = c.out("tmp", (4096,)), c.out("out", (4096,))

    def call(s):
        with torch.cuda.stream(s):                                          # (None: the current stream stays, the default one)
            torch.mul(x, 2.0, out=tmp)
        second(s, lambda: torch.add(tmp, 1.0, out=out))
        return 0
    c.call = call
    return c


def test_gate_catches_a_stage_that_escaped_to_the_default_stream(gate):
    """The second stage is issued on the default stream whatever stream the call was given: it runs in front of the blocker, on
    a `tmp` that nobody has written.  The gate must report an early write or a late-input mismatch of `out`."""
    def second(s, fn):
        fn()                                                                # (the current stream: the default one)
    rep = gate.run(_two_stage(second))
    assert not rep.inconclusive and not rep.errors, (rep.inconclusive, rep.errors)
    assert not rep.held_host
    assert "out" in rep.early_writes or "out" in rep.late_mismatch, "the gate did not notice a stage on the default stream"
    assert not rep.ordered
    R.measure(TAG + "/self_test/escape_seen_as_early_write", float("out" in rep.early_writes))
    R.measure(TAG + "/self_test/escape_seen_as_late_mismatch", float("out" in rep.late_mismatch))


def test_gate_passes_a_stage_on_a_stream_ordered_by_events(gate):
    """The second stage runs on another stream that waits for an event recorded on the caller's stream behind the first stage,
    and the caller's stream waits for the second stage in turn: ordered, though not on S.  Every check must pass."""
    side = torch.cuda.Stream()

    def second(s, fn):
        cur = s if s is not None else torch.cuda.default_stream()
        a, b = torch.cuda.Event(), torch.cuda.Event()
        a.record(cur)
        side.wait_event(a)
        with torch.cuda.stream(side):
            fn()
        b.record(side)
        cur.wait_event(b)
    rep = gate.run(_two_stage(second))
    rep.check()
    assert rep.ordered
