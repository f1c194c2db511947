"""References, bounds and planted faults for the text-stack operator tests (test_text_ops_cpu.py, test_text_ops_gpu.py).

Every reference takes a `dtype`: torch.float64 is the reference the kernels are judged against; torch.float32 is the same
formula evaluated in the kernels' own precision (the "restatement"), used on the CPU to show that a bound is wide enough for
correct fp32 arithmetic (>= 4x to spare) while a planted fault applied to the float64 reference misses it by >= 100x.
Shapes: qkv (B, L, 3H) = q | k | v with H = 64 * heads, mask (B, L) of 0 / 1, probs (B, heads, L, L), dctx (B, L, H)."""
import json
import os

import torch

HEAD = 64
MASK_KINDS = ("ones", "prefix", "token0", "hole", "zeros")


def measure(tag, value):
    """Print a measured figure and, with PNP_TEST_MEASURE_LOG set, append it to that file (as test_hip_parity._nerr does)."""
    value = float(value)
    print(f"[measured] {tag}: {value:.3e}")
    log = os.environ.get("PNP_TEST_MEASURE_LOG")
    if log:
        with open(log, "a") as f:
            f.write(json.dumps({"tag": tag, "value": value, "reduce": "max"}) + "\n")
    return value


# ------------------------------------------------------------------------------------------ inputs
def make_mask(kind, L):
    m = torch.zeros(L, dtype=torch.int64)
    if kind == "ones":
        m[:] = 1
    elif kind == "prefix":
        m[:max(L // 2, 1)] = 1
    elif kind == "token0":
        m[0] = 1
    elif kind == "hole":                      # live, a masked interior stretch, live again
        m[:] = 1
        m[L // 3:max(L // 3 + 1, 2 * L // 3)] = 0
        m[0] = 1
    elif kind != "zeros":
        raise ValueError(kind)
    return m


def make_masks(kinds, L):
    return torch.stack([make_mask(k, L) for k in kinds])


def make_qkv(B, L, heads, scale, seed, bf16=False):
    """q ~ scale * N(0, 1), k, v ~ N(0, 1); bf16: every operand is made bf16-exact before any reference sees it."""
    g = torch.Generator().manual_seed(seed)
    H = heads * HEAD
    qkv = torch.randn(B, L, 3 * H, generator=g)
    qkv[..., :H] *= scale
    return qkv.to(torch.bfloat16).float() if bf16 else qkv


def make_dctx(B, L, heads, seed):
    """N(0, 1) with two all-zero rows (token 0 of image 0, token L // 2 of the last image)."""
    g = torch.Generator().manual_seed(seed + 7)
    d = torch.randn(B, L, heads * HEAD, generator=g)
    d[0, 0] = 0
    d[B - 1, L // 2] = 0
    return d


def _heads(a, heads):
    B, L, _ = a.shape
    return a.reshape(B, L, heads, HEAD).permute(0, 2, 1, 3)


def _merge(a):
    B, h, L, _ = a.shape
    return a.permute(0, 2, 1, 3).reshape(B, L, h * HEAD)


def _split_qkv(qkv, heads, dtype):
    H = heads * HEAD
    qkv = qkv.to(dtype)
    return [_heads(qkv[..., i * H:(i + 1) * H], heads) for i in range(3)]


# ------------------------------------------------------------------------------------------ self-attention
def attn_fwd(qkv, mask, heads, dtype=torch.float64):
    """BertSelfAttention: softmax(q k^T / 8 + (1 - mask) * -10000) v.  Returns probs (B, heads, L, L), ctx (B, L, H)."""
    q, k, v = _split_qkv(qkv, heads, dtype)
    s = q @ k.transpose(-1, -2) * 0.125 + ((1.0 - mask.to(dtype)) * -10000.0)[:, None, None, :]
    p = s.softmax(-1)
    return p, _merge(p @ v)


def attn_bwd(qkv, dctx, probs, heads, dtype=torch.float64, fault=None):
    """The analytic backward from given probabilities: dP = dctx v^T, dS = P (dP - rowsum(dP P)), dq = dS k / 8,
    dk = dS^T q / 8, dv = P^T dctx.  Returns dq, dk, dv (B, L, H) and dS (B, heads, L, L)."""
    q, k, v = _split_qkv(qkv, heads, dtype)
    g = _heads(dctx.to(dtype), heads)
    p = probs.to(dtype)
    if fault == "neighbour_probs" and heads > 1:          # one (image, head) reads the next head's probabilities
        p = p.clone()
        p[0, 0] = p[0, 1]
    dp = g @ v.transpose(-1, -2)
    ds = p * (dp - (dp * p).sum(-1, keepdim=True))
    dq = ds @ k * (1.0 if fault == "dq_unscaled" else 0.125)
    dk = ds.transpose(-1, -2) @ q * 0.125
    dv = (p if fault == "dv_untransposed" else p.transpose(-1, -2)) @ g
    return _merge(dq), _merge(dk), _merge(dv), ds


def attn_bwd_autograd(qkv, mask, dctx, heads):
    """float64 autograd through attn_fwd: d(sum(ctx * dctx)) / d qkv, as dq, dk, dv (B, L, H)."""
    x = qkv.double().clone().requires_grad_(True)
    _, ctx = attn_fwd(x, mask, heads)
    ctx.backward(dctx.double())
    H = heads * HEAD
    gr = x.grad
    return gr[..., :H], gr[..., H:2 * H], gr[..., 2 * H:]


def attn_bound(ref):
    """fp32 self-attention outputs: 2e-5 * max(1, max|ref|) per output array -- the project's bound for this arithmetic
    (64-term fp32 dot products, __expf softmax, fp32 sums over the keys) in test_cross_attention_operator and
    test_vit_attention_operator."""
    # measured on MI355X, largest fraction of this bound over test_text_ops_gpu.py: forward probs 0.11, ctx 0.088; backward
    # dq 0.058, dk 0.062, dv 0.061, dS 0.033; at the benchmarked launches 0.013 at most
    return 2e-5 * max(1.0, float(ref.abs().max()))


def attn_bound_bf16(ref):
    """bf16 outputs (ctx, dqkv) of bf16-exact operands: 2^-8 * max|ref| for the one final rounding, on top of the fp32 bound.
    bf16 carries 8 significant bits, so half an ulp is at most 2^-8 of the value (at the bottom of a binade) and at most
    2^-8 * max|ref| anywhere in the array: a correctly rounded result can come close to this bound, it has no factor to spare
    (test_text_ops_cpu.py::test_bf16_bound_holds_for_a_correct_rounding)."""
    # measured on MI355X, largest fraction of this bound: ctx 0.94, dq 0.94, dk 0.96, dv 0.97 (the rounding of the largest
    # element; the CPU restatement rounded to bf16 gives the same figures)
    return 2.0 ** -8 * float(ref.abs().max()) + attn_bound(ref)


def zero_mask_terms(probs_ref_img, v_img):
    """Extra bound terms for an image whose mask is all zeros: score / 8 - 10000 in fp32 keeps only 2^-10 of the score (ulp of
    10000 is 2^-10, so each shifted score is off by <= 2^-11 and a ratio of two exponentials by <= 2^-10 relative):
    probs gain 2^-10 * max p, ctx 2^-10 * max|v|."""
    # measured on MI355X, largest fraction of the bound with these terms: probs 0.37, ctx 0.29 (fp32), 0.62 (bf16); the rows of
    # such an image sum to 1 within 4.0e-7 (asserted: 1e-6)
    return 2.0 ** -10 * float(probs_ref_img.max()), 2.0 ** -10 * float(v_img.abs().max())


def fault_mask(mask, fault):
    m = mask.clone()
    if fault == "drop_last_live_key":                     # one live key of one image masked
        live = torch.nonzero(m[0]).flatten()
        m[0, live[-1]] = 0
    elif fault == "mask_shifted":                         # mask column j read from column j - 1
        m = torch.roll(m, 1, dims=1)
    else:
        raise ValueError(fault)
    return m


# ------------------------------------------------------------------------------------------ LayerNorm
LN_KINDS = ("normal", "wide", "offset", "tight_offset", "constant")


def make_ln_rows(kind, rows, D, seed):
    g = torch.Generator().manual_seed(seed)
    n = torch.randn(rows, D, generator=g)
    if kind == "normal":
        return n
    if kind == "wide":
        return 3 * n + 1
    if kind == "offset":
        return n + 1000
    if kind == "tight_offset":
        return 0.01 * n + 1000
    if kind == "constant":                                # small integers: the fp32 row sum and mean are exact
        return torch.full((rows, D), 3.0)
    raise ValueError(kind)


def make_ln_weights(D, seed):
    g = torch.Generator().manual_seed(seed + 1)
    return 1 + 0.5 * torch.randn(D, generator=g), 0.3 * torch.randn(D, generator=g)


def ln_fwd(x, w, b, eps, dtype=torch.float64, fault=None):
    """Two-pass LayerNorm: xhat = (x - mean) * rstd, rstd = 1 / sqrt(mean((x - mean)^2) + eps), y = xhat * w + b."""
    x, w, b = x.to(dtype), w.to(dtype), b.to(dtype)
    mean = x.mean(-1, keepdim=True)
    if fault == "one_pass_variance":
        var = (x * x).mean(-1, keepdim=True) - mean * mean
    else:
        var = ((x - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=dtype))
    xhat = (x - mean) * rstd
    y = xhat * w + b
    if fault == "last_row_of_four_unwritten":             # the last row of a 4-row workgroup left at its input
        y, xhat = y.clone(), xhat.clone()
        r = min(3, x.shape[0] - 1)
        y[r], xhat[r] = x[r], x[r]
    return y, xhat, rstd[:, 0]


def ln_bwd(dy, w, xhat, rstd, dtype=torch.float64, fault=None):
    """dx = rstd (g - mean(g) - xhat mean(g xhat)), g = dy * w."""
    g = dy.to(dtype) * w.to(dtype)
    xhat, rstd = xhat.to(dtype), rstd.to(dtype)
    m1 = g.mean(-1, keepdim=True)
    m2 = (g * xhat).mean(-1, keepdim=True)
    if fault == "xhat_term_dropped":
        m2 = m2 * 0
    return rstd[:, None] * (g - m1 - xhat * m2)


def ln_xhat_bound(x, xhat, rstd):
    """16 * 2^-24 * (max|x| * max rstd + max|xhat|): the rounding of the mean and of each x - mean (both of size 2^-24 |x|,
    magnified by rstd) and of the final product; 16x for the summation tree and the spread between rows."""
    # measured on MI355X: 0.13 of it at most (CPU float32 restatement: 0.17)
    return 16 * 2.0 ** -24 * (float(x.abs().max()) * float(rstd.max()) + float(xhat.abs().max()))


def ln_rstd_bound(x, rstd):
    """Relative: 8 * 2^-24 * (1 + max|x| * max rstd), the same rounding of the differences seen through the variance."""
    # measured on MI355X: 0.056 of it at most
    return 8 * 2.0 ** -24 * (1 + float(x.abs().max()) * float(rstd.max()))


def ln_y_bound(x, xhat, rstd, w, y):
    # measured on MI355X: 0.12 of it at most
    return ln_xhat_bound(x, xhat, rstd) * float(w.abs().max()) + 2.0 ** -23 * float(y.abs().max())


def ln_bwd_bound(dy, w, xhat, rstd):
    """16 * 2^-24 * max rstd * max|g| * (1 + max|xhat|^2): two means of D products and three roundings per element."""
    g = dy.double() * w.double()
    # measured on MI355X: 0.12 of it at most
    return 16 * 2.0 ** -24 * float(rstd.max()) * float(g.abs().max()) * (1 + float(xhat.abs().max()) ** 2)


# ------------------------------------------------------------------------------------------ itm head
def itm_head(hlast, w, bias, dtype=torch.float64):
    """logits[b, c] = hlast[b, 0, :] . w[c, :] + bias[c]."""
    return hlast[:, 0].to(dtype) @ w.to(dtype).t() + bias.to(dtype)


def itm_bound(hlast, w, logits):
    """Per logit: 2^-22 * sum|h_d w_d| + 2^-23 |logit| (fp32 products and a sum in any order, one final add)."""
    # measured on MI355X: 0.30 of it at most at H = 64 (one product per lane), 0.073 at H = 768
    return 2.0 ** -22 * (hlast[:, 0].double().abs() @ w.double().abs().t()) + 2.0 ** -23 * logits.double().abs()
