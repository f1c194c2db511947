"""Case generators, references and planted faults for the post-processing operator tests (test_post_ops_cpu.py,
test_post_ops_gpu.py): pipeline_kernels.hip, crf_lattice.hip / crf_meanfield.hip and the post-processing entry points of post.hip.

The reference is the oracle alone (oracle/pipeline_np.py, `OP.*`): threshold / upsample, blur and labels are compared bit for
bit, DenseCRF marginals to atol = 1e-6 (the criterion of test_hip_parity.test_postprocess_stages_bit_exact_vs_oracle).

Every case works on the 8 x 8 patch grid of blip_itm_small(128) with one caption token per class, so the merge step is the
identity: rows 3 .. 3 + C of an image's (T, 8, 8) map are its class maps, every other row is zero.

CRF input rule (`class_maps`): the class maps of an image are zero outside the top-left `reg` x `reg` cells of the grid, every
class has a strong cell in grid row 0 and one in grid column 0 (so a 1 x W or H x 1 image, which samples that row / column
alone, still sees a non-constant map) and class 0 peaks at cell (0, 0).  Pixel (0, 0) then belongs to a class and the pixel in
the opposite corner to none: the background channel is neither empty nor full, no channel is constant, and nothing blurs to
0 / 0 = NaN.  `check_crf_input` asserts exactly that on the oracle's maps."""
import functools

import numpy as np

from oracle import pipeline_np as OP

F32 = np.float32
GRID = 8
THRESHOLD = 0.15
Q_ATOL = 1e-6


# ------------------------------------------------------------------------------------------ inputs
def photo_like(h, w, seed):
    """Smooth gradients + texture + per-pixel noise (not constant, many bilateral lattice points per pixel)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([128 + 90 * np.sin(xx / 37.0 + yy / 91.0), 128 + 80 * np.cos(xx / 53.0 - yy / 29.0), (3 * xx + 2 * yy) % 256], -1)
    return np.clip(img + rng.normal(0, 6, img.shape), 0, 255).astype(np.uint8)


def class_maps(rng, n_cls, reg):
    """(n_cls, 8, 8) maps following the CRF input rule of the module docstring."""
    m = np.zeros((n_cls, GRID, GRID), dtype=F32)
    for c in range(n_cls):
        n = int(rng.integers(3, 7))
        ys, xs = rng.integers(0, reg, size=n), rng.integers(0, reg, size=n)
        m[c, ys, xs] = rng.random(n, dtype=F32) ** 3                      # some of these fall under the threshold
        m[c, 0, int(rng.integers(0, reg))] = F32(0.5) + rng.random(dtype=F32) / 2
        m[c, int(rng.integers(0, reg)), 0] = F32(0.5) + rng.random(dtype=F32) / 2
    m[0, 0, 0] = F32(1.0)
    return m


class Case:
    """One prepared batch: sizes, class counts, maps (two sets: the second is the N-drop side of a paired run), RGB, LUTs."""

    def __init__(self, sizes, n_cls, has_bg, seed, n_class=21, reg=5):
        rng = np.random.default_rng(seed)
        self.sizes = [tuple(s) for s in sizes]
        self.B = len(sizes)
        self.n_cls = list(n_cls)
        self.has_bg = list(has_bg)
        self.K = [c + int(b) for c, b in zip(self.n_cls, self.has_bg)]
        self.n_class = n_class
        self.T = max(self.n_cls) + 4
        self.maps = np.zeros((self.B, self.T, GRID, GRID), dtype=F32)
        self.maps_n = np.zeros_like(self.maps)
        for b, c in enumerate(self.n_cls):
            self.maps[b, 3:3 + c] = class_maps(rng, c, reg)
            self.maps_n[b, 3:3 + c] = class_maps(rng, c, reg)
        self.rgb = [photo_like(h, w, seed * 100 + i) for i, (h, w) in enumerate(self.sizes)]
        self.best = [[int(v) for v in rng.permutation(n_class - 1)[:c]] for c in self.n_cls]
        self.luts = [[int(v) for v in OP.remap_labels(np.arange(k, dtype=F32), bst, hb)]
                     for k, bst, hb in zip(self.K, self.best, self.has_bg)]
        self.plans = [[([i], 1) for i in range(c)] for c in self.n_cls]
        self.gts = [rng.integers(0, n_class, size=s).astype(F32) for s in self.sizes]

    def sub(self, b):
        """The single-image batch made of image b."""
        o = object.__new__(Case)
        o.sizes, o.B, o.n_cls, o.has_bg, o.K = [self.sizes[b]], 1, [self.n_cls[b]], [self.has_bg[b]], [self.K[b]]
        o.n_class, o.T = self.n_class, self.T
        o.maps, o.maps_n = self.maps[b:b + 1], self.maps_n[b:b + 1]
        o.rgb, o.best, o.luts, o.plans, o.gts = [self.rgb[b]], [self.best[b]], [self.luts[b]], [self.plans[b]], [self.gts[b]]
        return o

    # -------------------------------------------------------------------------------------- oracle stages (cached per object)
    def ref_pre(self, b, scale01, second=False):
        key = ("pre", b, bool(scale01), second)
        if key not in self.__dict__.setdefault("_cache", {}):
            m = (self.maps_n if second else self.maps)[b, 3:3 + self.n_cls[b]]
            with np.errstate(all="ignore"):
                self._cache[key] = OP.threshold_upsample(m, *self.sizes[b], THRESHOLD, scale01, self.has_bg[b])
        return self._cache[key]

    def ref_blur(self, b, scale01, second=False):
        key = ("blur", b, bool(scale01), second)
        if key not in self.__dict__.setdefault("_cache", {}):
            pre = self.ref_pre(b, scale01, second)
            self._cache[key] = np.stack([OP.blurring(pre[k], self.sizes[b]) for k in range(self.K[b])])
        return self._cache[key]

    def ref_crf(self, b, scale01, second=False, **kw):
        """(labels (H, W) argmax indices, marginals (K, H, W), [gaussian points, bilateral points])."""
        key = ("crf", b, bool(scale01), second, tuple(sorted(kw.items())))
        if key not in self.__dict__.setdefault("_cache", {}):
            self._cache[key] = OP.densecrf(self.rgb[b], self.ref_blur(b, scale01, second), want_q=True, **kw)
        return self._cache[key]

    def remap(self, b, lab):
        return OP.remap_labels(lab, self.best[b], self.has_bg[b])


def check_crf_input(case, scale01, second=False):
    """The input rule every CRF case must pass on the oracle's maps: no NaN after the blur, background neither empty nor full."""
    for b in range(case.B):
        pre, blur = case.ref_pre(b, scale01, second), case.ref_blur(b, scale01, second)
        assert not np.isnan(pre).any() and not np.isnan(blur).any(), (b, case.sizes[b])
        if case.has_bg[b]:
            bg = pre[0]
            assert 0 < bg.sum() < bg.size, (b, case.sizes[b], float(bg.sum()), bg.size)
        for k in range(case.K[b]):
            assert pre[k].min() < pre[k].max(), (b, k)


def _cyc(seq, n):
    return [seq[i % len(seq)] for i in range(n)]


@functools.lru_cache(maxsize=None)
def case_chunked():
    """A: 9 ragged images, K cycling 2 / 3 / 5 / 21.  With crf_chunk = 4 the mean-field runs images [0, 4), [4, 8), [8, 9)."""
    K = _cyc([2, 3, 5, 21], 9)
    return Case(_cyc([(24, 40), (33, 45), (40, 24), (17, 64)], 9), [k - 1 for k in K], [True] * 9, seed=11)


@functools.lru_cache(maxsize=None)
def case_wide():
    """A: two 48 x 64 images of K = 151 channels (rows of 152 floats, 304 paired)."""
    return Case([(48, 64), (48, 64)], [150, 150], [True, True], seed=12, n_class=151)


@functools.lru_cache(maxsize=None)
def case_mixed():
    """A: K = 151 next to K = 3 in one batch."""
    return Case([(48, 64), (33, 45)], [150, 2], [True, True], seed=13, n_class=151)


@functools.lru_cache(maxsize=None)
def case_args():
    """B: the batch the pnp_densecrf arguments are varied on."""
    return Case([(33, 101), (200, 9), (64, 64)], [2, 4, 1], [True, True, True], seed=14)


CRF_ARGS = [dict(iters=0), dict(iters=1), dict(iters=3),
            dict(iters=10, pos_w=0.0, bi_w=10.0), dict(iters=10, pos_w=7.0, bi_w=0.0), dict(iters=10, pos_w=3.5, bi_w=4.25)]

# C: (H, W) -> what it exercises; see the module docstring of test_post_ops_gpu.py
THIN_SHAPES = [(9, 200), (200, 9), (3, 160), (1, 140), (140, 1)]
EDGE_BATCHES = {
    # odd-sized images first: the planes of every later image start at an odd float offset
    "odd_first": dict(sizes=[(33, 45), (31, 101), (9, 200), (200, 9), (32, 64)], n_cls=[2, 5, 1, 3, 5],
                      has_bg=[True, True, True, False, True]),
    # an aligned (32, 64) first (the 16-byte staging path), then the degenerate shapes
    "aligned_first": dict(sizes=[(32, 64), (5, 7), (3, 160), (1, 140), (140, 1)], n_cls=[2, 5, 2, 1, 6],
                          has_bg=[True, True, True, True, False]),
}


@functools.lru_cache(maxsize=None)
def case_edge(name):
    d = EDGE_BATCHES[name]
    return Case(d["sizes"], d["n_cls"], d["has_bg"], seed=15 + sorted(EDGE_BATCHES).index(name))


# ------------------------------------------------------------------------------------------ value edge cases of the class maps
def value_case(kind):
    """D: two images of two classes + background with one value edge planted in both map sets.  "constant": class 0 of image 0
    is 0.25 everywhere; "inf" / "nan": one such cell in class 0 of image 0; "tie": class 1 is a copy of class 0, and class 0
    covers the top-left 4 x 4 cells -- the tied pair halves its probability mass, and on a smaller region the mean-field hands
    every one of its pixels to the background, which leaves no tie to break."""
    case = Case([(33, 45), (24, 40)], [2, 2], [True, True], seed=51)
    for m in (case.maps, case.maps_n):
        if kind == "constant":
            m[0, 3] = F32(0.25)
        elif kind == "inf":
            m[0, 3, 2, 3] = np.inf
        elif kind == "nan":
            m[0, 3, 2, 3] = np.nan
        elif kind == "tie":
            m[:, 3, :4, :4] = np.maximum(m[:, 3, :4, :4], F32(0.5))
            m[:, 4] = m[:, 3]
        else:
            raise ValueError(kind)
    return case


# ------------------------------------------------------------------------------------------ blur: planted fault
def blur_single_reflection(x, sigma):
    """OP.gaussian_blur with the reflection folded ONCE (what blur_axis_kernel's reflect_fast alone would compute): correct
    while the radius is below the axis length, clamped to the border beyond."""
    w, r = OP.gaussian_kernel1d(sigma)

    def corr(x, axis):
        x = np.moveaxis(x, axis, -1).astype(np.float64)
        n = x.shape[-1]
        idx = np.arange(-r, n + r)
        idx = np.where(idx < 0, -idx - 1, np.where(idx >= n, 2 * n - 1 - idx, idx))
        ext = x[..., np.clip(idx, 0, n - 1)]
        out = ext[..., r:r + n] * w[r]
        for j in range(r, 0, -1):
            out = out + (ext[..., r - j:r - j + n] + ext[..., r + j:r + j + n]) * w[r - j]
        return np.moveaxis(out.astype(F32), -1, axis)
    return corr(corr(x.astype(F32), 0), 1)


# ------------------------------------------------------------------------------------------ drop step
def topk_smaller_index_wins(sal, picked, k=10):
    """Planted fault: OP.select_topk with ties broken towards the SMALLER index."""
    s = sal.flatten().copy()
    for p in picked:
        s[p] = 0
    n = s.size
    order = np.argsort(s[::-1], kind="stable")              # ascending; among equals the larger original index first
    return [int(n - 1 - i) for i in order[-k:]]


def topk_nan_smallest(sal, picked, k=10):
    """Planted fault: NaN ordered below every number instead of above."""
    s = sal.flatten().copy()
    for p in picked:
        s[p] = 0
    s = np.where(np.isnan(s), -np.inf, s)
    return [int(i) for i in np.argsort(s, kind="stable")[-k:]]


def drop_reference(gs, npick=10, max_picks=None, topk=OP.select_topk):
    """The bookkeeping of OP.drop_loop (PnP.py:619-647, 716-721) on prepared maps gs[it] (B, T, P, P), with the pick list cut at
    `max_picks` slots per image as pnp_drop_step does: a pick whose slot it * npick + j lies past it is neither stored nor
    flagged.  Returns (g0, agg, dropped (B, PP) uint8, picks (B, max_picks) int32 with -1 in unused slots)."""
    iters = len(gs)
    B, T, P, _ = gs[0].shape
    max_picks = iters * npick if max_picks is None else max_picks
    picks = [[] for _ in range(B)]
    out = np.full((B, max_picks), -1, dtype=np.int32)
    g0 = agg = None
    with np.errstate(all="ignore"):
        for it, g in enumerate(gs):
            pred = g.copy()
            for b in range(B):
                for p in picks[b]:
                    pred[b, :, p // P, p % P] = 0
            if it == 0:
                g0, agg = pred.copy(), (pred + pred).astype(F32)
            else:
                agg = (agg + pred).astype(F32)
            for b in range(B):
                sal = g[b, 3:-1].sum(axis=0, dtype=F32)
                sel = topk(sal, picks[b], npick)
                for j, p in enumerate(sel):
                    if it * npick + j < max_picks:
                        out[b, it * npick + j] = p
                        picks[b].append(p)
    dropped = np.zeros((B, P * P), dtype=np.uint8)
    for b in range(B):
        dropped[b, picks[b]] = 1
    return g0, agg, dropped, out


DROP_INPUTS = ("zeros", "four_cells", "plateaus", "neg_zero", "nan")


def drop_maps(kind, P, T, iters=3, seed=0):
    """iters maps (2, T, P, P).  Salience = sum of rows 3 .. T - 2 (empty for T = 4).  Values are small multiples of 1 / 8, so
    every row sum is exact whatever its order and equal cells tie exactly."""
    rng = np.random.default_rng(seed + 31 * P + T)
    gs = []
    for it in range(iters):
        g = np.zeros((2, T, P, P), dtype=F32)
        flat = g.reshape(2, T, P * P)
        rows = list(range(3, T - 1))
        if kind == "zeros" or not rows:
            pass
        elif kind == "four_cells":
            for b in range(2):
                cells = rng.choice(P * P, size=4, replace=False)
                for r in rows:
                    flat[b, r, cells] = rng.integers(1, 9, size=4) / F32(8)
        elif kind in ("plateaus", "neg_zero", "nan"):
            for b in range(2):
                level = rng.integers(0, 4, size=P * P)              # four levels: plateaus far wider than npick
                for r in rows:
                    flat[b, r] = level / F32(8)
                if kind == "neg_zero":
                    for r in rows:
                        flat[b, r, level == 0] = F32(-0.0)
                        flat[b, r, level == 1] = F32(-0.0) if r != rows[0] else F32(0.125)
            if kind == "nan":
                c = rng.choice(P * P, size=2, replace=False)
                flat[1, rows[-1], c] = np.nan                        # image 1 only
        else:
            raise ValueError(kind)
        flat[:, :3] = rng.integers(0, 9, size=(2, 3, P * P)) / F32(8)    # rows outside the salience sum: bookkeeping only
        flat[:, T - 1] = rng.integers(0, 9, size=(2, P * P)) / F32(8)
        gs.append(g)
    return gs


# ------------------------------------------------------------------------------------------ lattice key range
def bilateral_key_extent(x, y, rgb, sxy=50.0, srgb=5.0):
    """Largest |coordinate| of the six bilateral lattice keys of one pixel, by lattice_embed_kernel's float32 rule
    (crf_lattice.hip; oracle/densecrf_ref.c::lattice_init).  The kernel packs 11 bits per coordinate and refuses a key with
    |coordinate| >= 2^10 - (D + 1) = 1018."""
    D = 5
    f = [F32(x) / F32(sxy), F32(y) / F32(sxy)] + [F32(c) / F32(srgb) for c in rgb]
    inv_std = F32(np.sqrt(2.0 / 3.0) * (D + 1))
    scale = [F32(1.0 / np.sqrt(float((i + 2) * (i + 1))) * float(inv_std)) for i in range(D)]
    elev = [F32(0)] * (D + 1)
    sm = F32(0)
    for j in range(D, 0, -1):
        cf = F32(f[j - 1] * scale[j - 1])
        elev[j] = F32(sm - F32(F32(j) * cf))
        sm = F32(sm + cf)
    elev[0] = sm
    down, up_f = F32(1.0) / F32(D + 1), F32(D + 1)
    ext = 0
    for i in range(D):                                        # key coordinates are elevated axes 0 .. D - 1
        v = F32(down * elev[i])
        up, dn = F32(np.ceil(v) * up_f), F32(np.floor(v) * up_f)
        rem0 = int(up) if F32(up - elev[i]) < F32(elev[i] - dn) else int(dn)
        ext = max(ext, abs(rem0) + D + 1)                     # canonical offsets span [-(D + 1), D + 1] around rem0
    return ext


KEY_LIMIT = (1 << 10) - 6
RANGE_W = 12600            # a white 1 x RANGE_W image: 0.0693 * x + 173.7 (the colour terms) passes 1018 near x = 12190


# ------------------------------------------------------------------------------------------ histogram
def hist_case(n_class, seed):
    """Labels, ground truth and LUT for confusion_hist: gt holds 255, -1, n_class and n_class - 1; the LUT sends two argmax
    indices to ids >= n_class.  np.bincount(n_class * gt + pred) counts such a prediction in the NEXT row of the matrix
    (PnP.py:1106-1112 does the same) and cannot be reshaped once an index passes n_class^2, so pixels whose truth is the
    last class never carry one of those two predictions."""
    rng = np.random.default_rng(seed)
    sizes = [(33, 45), (17, 64)]
    K = 6
    lut = [int(v) for v in rng.permutation(n_class)[:K - 2]] + [n_class, min(n_class + 7, 255)]
    idx = [rng.integers(0, K, size=s) for s in sizes]                       # the argmax index every pixel will get
    gts = []
    for s, ix in zip(sizes, idx):
        g = rng.integers(0, n_class, size=s).astype(F32)
        special = rng.random(s)
        g[special < 0.05] = 255
        g[(special >= 0.05) & (special < 0.10)] = -1
        g[(special >= 0.10) & (special < 0.15)] = n_class
        g[(special >= 0.15) & (special < 0.25)] = n_class - 1
        g[(g == n_class - 1) & (ix >= K - 2)] = n_class - 2
        gts.append(g)
    return sizes, K, lut, idx, gts


def hist_reference(gts, idx, lut, n_class, ignore_rule=None):
    """OP.scores' histogram of the LUT-mapped labels.  ignore_rule: a planted fault replacing fast_hist's mask."""
    preds = [np.asarray(lut)[ix].astype(F32) for ix in idx]
    if ignore_rule is None:
        return OP.scores(gts, preds, n_class)[1].astype(np.int64)
    h = np.zeros(n_class * n_class, dtype=np.int64)
    for g, p in zip(gts, preds):
        m = ignore_rule(g.ravel(), n_class)
        np.add.at(h, (n_class * g.ravel()[m] + p.ravel()[m]).astype(np.int64) % h.size, 1)    # out-of-range bins wrap: still seen
    return h.reshape(n_class, n_class)
