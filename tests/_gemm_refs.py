"""References, input families, bounds and planted faults for the GEMM / ViT-attention operator tests (test_gemm_ops_cpu.py,
test_gemm_ops_gpu.py, test_attn_ops_gpu.py).  Everything here is plain torch on whatever device the inputs live on; float64 is
the reference the kernels are judged against.

Two input families for C = A . B^T:
  exact : integer-valued operands sized so that every product and every partial sum, in ANY summation order, is an integer
          below 2^24 -- fp32 accumulation is then exact, a linear epilogue with an fp32 output must equal the float64 reference
          bit for bit, a bf16 output must equal bf16(ref) (one rounding of an exact value), and a split output must be the
          split of ref.  No tolerance: an indexing, slab-order, tile-ownership or stream-K fix-up error fails outright.
  random: N(0, 1) with a few outlier channels (columns of A scaled by 30..100); for the GELU / GELU' epilogues and rounding.
          Its bounds are the ones tests/test_hip_parity.py uses for the same kernel and type, scaled by the row-norm product
          |A_m| |B_n| where the outliers make the operands non-unit-scale.
"""
import math

import torch

from _text_refs import measure          # noqa: F401  (re-exported: R.measure)

EXACT_LIMIT = 2 ** 24


# ------------------------------------------------------------------------------------------ exact family
def exact_mags(K, split=False):
    """(|A|max, |B|max) of the exact family at depth K.  plain: both <= 127 (bf16-exact integers); split: A up to 11
    significant bits (hi and lo both non-zero, hi + lo == A exactly), B a small bf16-exact integer (B_lo == 0, so the
    dropped lo.lo term is exactly 0).  Magnitudes shrink with K to keep K * (|A|max + 8) * |B|max + 2^17 below 2^24."""
    budget = (EXACT_LIMIT - 2 ** 18) // K
    if not split:
        a = min(127, int(math.isqrt(budget)))
        return a, a
    if budget >= 2056 * 3:
        return 2047, min(127, budget // 2056)
    return budget // 3 - 8, 3


def exact_operands(M, N, K, seed, split=None, device="cpu"):
    """Integer-valued fp32 A [M, K], B [N, K].  split: None (plain), "A" (A carries the 11-bit values), "B" (roles swapped)."""
    g = torch.Generator(device=device).manual_seed(seed)
    a, b = exact_mags(K, split is not None)
    if split == "B":
        a, b = b, a
    A = torch.randint(-a, a + 1, (M, K), generator=g, device=device).float()
    B = torch.randint(-b, b + 1, (N, K), generator=g, device=device).float()
    return A, B


def exact_vector(n, seed, mag=2 ** 15, device="cpu"):
    """Integer-valued bias / residual entries, |v| <= mag."""
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.randint(-mag, mag + 1, (n,) if isinstance(n, int) else tuple(n), generator=g, device=device).float()


def split_pair(x):
    """hi = bf16(x), lo = bf16(x - hi) (round to nearest even), as pnp_op_split and the kernels' split stores."""
    hi = x.float().to(torch.bfloat16)
    lo = (x.float() - hi.float()).to(torch.bfloat16)
    return hi, lo


def assert_exact_family(A, B, bias=None, resid=None, split=False):
    """The 2^24 condition, in float64.  For a split launch the kernel multiplies |hi| and |lo| separately."""
    if split:
        def absparts(x):
            hi, lo = split_pair(x)
            assert torch.equal(hi.float() + lo.float(), x.float()), "exact family: operand is not a (hi, lo) pair"
            return hi.double().abs() + lo.double().abs()
        a, b = absparts(A), absparts(B)
    else:
        a, b = A.double().abs(), B.double().abs()
    top = float((a @ b.t()).max())
    top += float(bias.abs().max()) if bias is not None else 0.0
    top += float(resid.abs().max()) if resid is not None else 0.0
    assert top < EXACT_LIMIT, (top, EXACT_LIMIT)
    return top


# ------------------------------------------------------------------------------------------ random family
def random_operands(M, N, K, seed, b_scale=1.0, outliers=3, device="cpu", bf16=False):
    """A ~ N(0, 1) with `outliers` columns scaled by 30, 65, 100 (as droploop_large_outliers' massive channels), B ~ b_scale *
    N(0, 1).  bf16: both are made bf16-exact before any reference sees them."""
    g = torch.Generator(device=device).manual_seed(seed)
    A = torch.randn(M, K, generator=g, device=device)
    B = torch.randn(N, K, generator=g, device=device) * b_scale
    cols = torch.randperm(K, generator=g, device=device)[:min(outliers, K)]
    for i, c in enumerate(cols.tolist()):
        A[:, c] *= (30.0, 65.0, 100.0)[i % 3]
    if bf16:
        A, B = A.to(torch.bfloat16).float(), B.to(torch.bfloat16).float()
    return A, B


def norm_scale(A, B):
    """[M, N] max(1, |A_m| |B_n| / K): 1 for unit-scale operands (|A_m| |B_n| ~ K), grows with the outlier channels."""
    K = A.shape[1]
    return (A.double().norm(dim=1)[:, None] * B.double().norm(dim=1)[None, :] / K).clamp_min(1.0)


def accum_bound(A, B, bf16):
    """test_hip_parity.test_gemm: (2e-4 fp32 | 2e-3 bf16 operands) * sqrt(K / 128) on unit-scale data, per element scaled by
    the row-norm product.  Operands are exact in the compute type, so this covers the fp32 accumulation order only."""
    K = A.shape[1]
    return (2e-3 if bf16 else 2e-4) * math.sqrt(K / 128) * norm_scale(A, B)


def x3_bound(A, B):
    """test_hip_parity._x3_case: six sigma of the 2^-16 per-product error, sigma = 2^-16 sqrt(sum (a_i b_i)^2) -- there
    2^-16 * sqrt(K) * 0.25 for A ~ N(0, 1), B ~ 0.25 N(0, 1), i.e. 2^-16 |A_m| |B_n| / sqrt(K) -- plus 1e-5."""
    K = A.shape[1]
    return 6 * 2.0 ** -16 * (A.double().norm(dim=1)[:, None] * B.double().norm(dim=1)[None, :]) / math.sqrt(K) + 1e-5


def bf16_out_bound(ref):
    """test_hip_parity._wide_bf16_case: one bf16 rounding of the largest output, 2^-8 max|ref| + 1e-3."""
    return 2.0 ** -8 * float(ref.abs().max()) + 1e-3


GELU_SLOPE = 1.13           # max |GELU'(x)| = 1.129 at x = 1.41


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))


def gelu_grad64(x):
    return 0.5 * (1.0 + torch.erf(x * 0.7071067811865476)) + x * 0.3989422804014327 * torch.exp(-0.5 * x * x)


def gelu_bound(lin_bound, pre):
    """An error e of the pre-activation leaves GELU as at most 1.13 e; the erf evaluation itself (libm erff, or Abramowitz-Stegun
    7.1.26 with |error| <= 1.5e-7 in the bf16-mode kernels) and the fp32 roundings of x * Phi(x) stay below 1e-6 max(1, |x|)."""
    return GELU_SLOPE * lin_bound + 1e-6 * pre.abs().clamp_min(1.0)


def gelu_grad_bound(lin_bound, lin):
    """out = v * GELU'(u): 1.13 times the error of v plus |v| times the fp32 evaluation error of GELU' (erff + fast exp: a few
    ulp, < 2e-6)."""
    return GELU_SLOPE * lin_bound + 2e-6 * lin.abs().clamp_min(1.0)


# ------------------------------------------------------------------------------------------ tiled product + planted faults
def tiled_product(A, B, tile_n=64, slab=32, order="fwd", fault=None, dtype=torch.float32, sk_parts=0):
    """numpy-style emulation of the kernels' tiling: C[:, tile] = sum over k-slabs of A[:, slab] . B[tile, slab]^T, partial
    products in `dtype`, slabs visited in `order` ("fwd" | "rev" | "even_odd"); sk_parts > 1: each column tile's slabs are cut
    into that many partial tiles that are summed afterwards (the stream-K fix-up).
    fault: None | "swap_tiles" (column tiles 0 and 1 land in each other's place) | "skip_last_slab" | "sk_twice" (one partial
    tile of the last column tile added twice) | "mask_off_by_one" (the ragged last column is not written)."""
    M, K = A.shape
    N = B.shape[0]
    A, B = A.to(dtype), B.to(dtype)
    nk = (K + slab - 1) // slab
    ks = list(range(nk))
    if order == "rev":
        ks = ks[::-1]
    elif order == "even_odd":
        ks = ks[0::2] + ks[1::2]
    if fault == "skip_last_slab":
        ks = [k for k in ks if k != nk - 1]
    C = torch.zeros(M, N, dtype=dtype)
    nt = (N + tile_n - 1) // tile_n
    for t in range(nt):
        n0, n1 = t * tile_n, min(N, (t + 1) * tile_n)
        parts = [ks[i::sk_parts] for i in range(sk_parts)] if sk_parts > 1 else [ks]
        tot = torch.zeros(M, n1 - n0, dtype=dtype)
        for pi, part in enumerate(parts):
            acc = torch.zeros(M, n1 - n0, dtype=dtype)
            for k in part:
                acc = acc + A[:, k * slab:(k + 1) * slab] @ B[n0:n1, k * slab:(k + 1) * slab].t()
            tot = tot + acc
            if fault == "sk_twice" and t == nt - 1 and pi == 0:
                tot = tot + acc
        C[:, n0:n1] = tot
    if fault == "swap_tiles" and nt >= 2:
        w = min(tile_n, N - tile_n)
        first = C[:, :w].clone()
        C[:, :w] = C[:, tile_n:tile_n + w]
        C[:, tile_n:tile_n + w] = first
    if fault == "mask_off_by_one":
        C[:, N - 1] = float("nan")               # the sentinel stays: "not written"
    return C


def split_product(A, B, fault=None):
    """The three-pass split-bf16 product in fp32: A_hi.B_hi + A_hi.B_lo + A_lo.B_hi (lo.lo dropped).
    fault "drop_lo_hi": the A_lo.B_hi pass is missing."""
    (ah, al), (bh, bl) = split_pair(A), split_pair(B)
    ah, al, bh, bl = ah.float(), al.float(), bh.float(), bl.float()
    C = ah @ bh.t() + ah @ bl.t()
    if fault != "drop_lo_hi":
        C = C + al @ bh.t()
    return C


def row_remap(m, row_div, fault=False):
    """Patch row m -> token row (skip the cls row of every image).  fault: the `+ 1` is missing."""
    b, p = divmod(m, row_div)
    return b * (row_div + 1) + p + (0 if fault else 1)


def bf16_truncate(x):
    """A bf16 store that drops the low 16 bits instead of rounding to nearest even (planted fault)."""
    bits = x.float().contiguous().view(torch.int32)
    return (bits & ~0xFFFF).view(torch.float32).to(torch.bfloat16)


# ------------------------------------------------------------------------------------------ attention
ATTN_CASES = ("random", "max_last", "max_first", "constant", "outliers")


def make_attn_qkv(case, B, N, heads, seed, device="cpu"):
    """q, k, v (B, N, heads * 64) fp32 for softmax(q k^T / 8) v.
      random   : N(0, 1)
      max_last : every query's largest score belongs to the last key (only the last key tile raises the running maximum there)
      max_first: key 0 wins and every later score is at least 100 lower (all later tiles underflow against the first)
      constant : all keys equal -- each row of scores is constant, the softmax uniform, ctx the mean of v
      outliers : two channels of q and k scaled by 12 (ViT-L's massive channels): scaled scores reach the hundreds"""
    g = torch.Generator(device=device).manual_seed(seed)
    D = heads * 64
    q = torch.randn(B, N, D, generator=g, device=device)
    k = torch.randn(B, N, D, generator=g, device=device)
    v = torch.randn(B, N, D, generator=g, device=device)
    if case in ("max_last", "max_first"):
        # per head, |u| = 1.  max_last: q = 0.5 noise + 4 u, last key = 16 u -> its score is 8 + noise, the others |s| < 3: the
        # winner carries e^8 against N - 1 keys of order 1, a real mixture.  max_first: q = 0.05 noise + 40 u, key 0 = 40 u ->
        # 200 against |s| < 25: the margin is > 100 and every later tile underflows
        u = torch.randn(heads, 64, generator=g, device=device)
        u = (u / u.norm(dim=1, keepdim=True)).reshape(D)
        if case == "max_last":
            q = 0.5 * q + 4.0 * u
            k = 0.5 * k
            k[:, N - 1] = 16.0 * u
        else:
            q = 0.05 * q + 40.0 * u
            k = 0.5 * k
            k[:, 0] = 40.0 * u
    elif case == "constant":
        k = k[:, :1].expand(B, N, D).clone()
    elif case == "outliers":
        for h in range(heads):
            for c in (h * 64 + 5, h * 64 + 41):
                q[..., c] *= 12.0
                k[..., c] *= 12.0
    elif case != "random":
        raise ValueError(case)
    return q, k, v


def _heads(a, heads):
    B, N, _ = a.shape
    return a.reshape(B, N, heads, 64).permute(0, 2, 1, 3)


def attn64(q, k, v, heads, scale=0.125):
    """float64 softmax(q k^T scale) v -> (ctx (B, N, D), scores (B, heads, N, N))."""
    qh, kh, vh = (_heads(a.double(), heads) for a in (q, k, v))
    s = qh @ kh.transpose(-1, -2) * scale
    ctx = (s.softmax(-1) @ vh).permute(0, 2, 1, 3).reshape(q.shape)
    return ctx, s


def attn_restated(q, k, v, heads, kind, scale=0.125, tile=64):
    """The kernels' arithmetic in float32: scores in fp32, then the online softmax over 64-key tiles in key order (running
    maximum, rescale of the running sum and output by exp(m_old - m_new), p = exp(s - m)), P.V accumulated in fp32.
    kind "f32": nothing else.  "bf16": operands are bf16 already, P is rounded to bf16 before P.V and the context is stored as
    bf16.  "x3": q, k, v are (hi, lo) pairs, both products drop their lo.lo term, P is split after the exp and the context
    leaves as a pair.  Returns the context as float64 (B, N, D)."""
    f = torch.float32
    qh, kh, vh = (_heads(a.to(f), heads) for a in (q, k, v))

    def qk(a, b):
        # the 64 products of a score are added one channel at a time with plain fp32 multiplies and adds: the same bits on
        # every machine (a BLAS call may order, block and fuse them differently), so the measured error is reproducible
        out = torch.zeros(a.shape[:-1] + (b.shape[-2],), dtype=f, device=a.device)
        for d in range(a.shape[-1]):
            out += a[..., :, d:d + 1] * b[..., None, :, d]
        return out
    if kind == "x3":
        (q1, q2), (k1, k2), (v1, v2) = (tuple(t.float() for t in split_pair(a)) for a in (qh, kh, vh))
        s = qk(q1, k1) + qk(q1, k2) + qk(q2, k1)
    else:
        s = qk(qh, kh)
    N = s.shape[-1]
    m = torch.full(s.shape[:-1] + (1,), -float("inf"), dtype=f, device=s.device)
    l = torch.zeros_like(m)
    o = torch.zeros(qh.shape, dtype=f, device=s.device)
    sc = torch.tensor(scale, dtype=f)
    for t0 in range(0, N, tile):
        st = s[..., t0:t0 + tile]
        m_new = torch.maximum(m, st.max(-1, keepdim=True).values)
        alpha = torch.exp((m - m_new) * sc)
        p = torch.exp((st - m_new) * sc)
        l = l * alpha + p.sum(-1, keepdim=True)
        vt = vh[..., t0:t0 + tile, :]
        if kind == "bf16":
            pv = p.to(torch.bfloat16).float() @ vt
        elif kind == "x3":
            p1, p2 = (t.float() for t in split_pair(p))
            pv = p1 @ v1[..., t0:t0 + tile, :] + p2 @ v1[..., t0:t0 + tile, :] + p1 @ v2[..., t0:t0 + tile, :]
        else:
            pv = p @ vt
        o = o * alpha + pv
        m = m_new
    o = (o / l).permute(0, 2, 1, 3).reshape(q.shape)
    if kind == "bf16":
        o = o.to(torch.bfloat16)
    elif kind == "x3":
        hi, lo = split_pair(o)
        return hi.double() + lo.double()
    return o.double()


# Project bounds (tests/test_hip_parity.py), each times max(1, max|ref|): ViT attention fp32 2e-5, bf16 2e-2, split-bf16 5e-5;
# cross attention 2e-5 / 3e-2.  Where the float32 restatement above cannot stay within a quarter of a bound on a structured
# score case, that case's bound is four times the restatement's measured error (test_gemm_ops_cpu.py measures it; DESIGN.md
# records both numbers).
ATTN_TOL = {"f32": 2e-5, "bf16": 2e-2, "x3": 5e-5}
# "outliers" (scaled scores up to ~320): one fp32 ulp of such a score is 3e-5, which the exp turns into that relative error of a
# probability; the split form also drops the lo.lo term of q.k, 2^-18 |q| |k| / 8.  Restatement, worst over N in {1, 33, 65,
# 257, 442, 769} x heads in {12, 16}: fp32 3.98e-5, split 3.81e-4 (of max(1, max|ref|)), rounded up to 4.0e-5 / 3.9e-4, x 4.
ATTN_TOL_CASE = {("f32", "outliers"): 4 * 4.0e-5, ("x3", "outliers"): 4 * 3.9e-4}
XATTN_TOL = {"f32": 2e-5, "bf16": 3e-2}


def attn_tol(kind, case):
    return ATTN_TOL_CASE.get((kind, case), ATTN_TOL[kind])


def attn_bound(kind, case, ref):
    return attn_tol(kind, case) * max(1.0, float(ref.abs().max()))
