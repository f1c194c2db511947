"""Reference for the general stand-alone DenseCRF (per-axis widths, label-compatibility matrices, stepwise inference, KL): a
numpy float32 restatement of the mean-field that follows oracle/densecrf_ref.c operation for operation -- the embedding
(lattice_init, here with one width per feature axis), the sequential splat in pixel order (np.add.at adds unbuffered, in index
order), the axis blurs `old + 0.5 * (n1 + n2)` through double, the slice times alpha, the symmetric normaliser -- and takes the
softmax from the oracle itself (exp_and_normalize with include/pnp_math.h's exp, reached through OP.densecrf_variant with no
iterations).  The compatibility step is the loop include/pnp_hip.h fixes for pnp_crf_set_compat:

    acc_t[l] = 0;  for k ascending: acc_t[l] = acc_t[l] + M_t[l][k] * msg_t[k]        (float32, product and sum rounded apart)
    logit[l] = (-U[l] + acc_g[l]) + acc_b[l]

Written from this repository's oracle and the papers it cites (Kraehenbuehl & Koltun 2011; Adams et al. 2010).  Lattice point
ids differ from the oracle's hash order; no result depends on them.  Also here: the KL divergence of pnp_crf_kl in float64, and
a float64 brute force (all N^2 kernel entries, general widths and weights) for statistical checks on small images."""
import numpy as np

from oracle import pipeline_np as OP

F32 = np.float32


class Lattice:
    """Permutohedral lattice of feature (N, d) float32: offset (N, d + 1) ids, bary (N, d + 1), n1 / n2 (d + 1, M), -1 absent."""

    def __init__(self, feature):
        feature = np.ascontiguousarray(feature, dtype=F32)
        N, d = feature.shape
        self.N, self.d = N, d
        inv_std = F32(np.sqrt(2.0 / 3.0) * (d + 1))
        scale = [F32(1.0 / np.sqrt(float((i + 2) * (i + 1))) * float(inv_std)) for i in range(d)]
        el = np.zeros((N, d + 1), F32)
        sm = np.zeros(N, F32)
        for j in range(d, 0, -1):
            cf = feature[:, j - 1] * scale[j - 1]
            el[:, j] = sm - F32(j) * cf
            sm = sm + cf
        el[:, 0] = sm
        down, up = F32(1.0) / F32(d + 1), F32(d + 1)
        rem0 = np.zeros((N, d + 1), F32)
        total = np.zeros(N, np.int32)
        for i in range(d + 1):
            v = down * el[:, i]
            hi, lo = np.ceil(v) * up, np.floor(v) * up
            rd2 = np.where(hi - el[:, i] < el[:, i] - lo, hi, lo).astype(np.int16).astype(np.int32)
            rem0[:, i] = rd2.astype(F32)
            total = (total.astype(F32) + rd2.astype(F32) * down).astype(np.int32)
        rank = np.zeros((N, d + 1), np.int32)
        diff = el - rem0
        for i in range(d):
            for j in range(i + 1, d + 1):
                less = diff[:, i] < diff[:, j]
                rank[:, i] += less
                rank[:, j] += ~less
        rank += total[:, None]
        neg, over = rank < 0, rank > d
        rank = np.where(neg, rank + d + 1, np.where(over, rank - (d + 1), rank))
        rem0 = np.where(neg, rem0 + F32(d + 1), np.where(over, rem0 - F32(d + 1), rem0)).astype(F32)
        bary = np.zeros((N, d + 2), F32)
        rows = np.arange(N)
        for i in range(d + 1):
            v = (el[:, i] - rem0[:, i]) * down
            bary[rows, d - rank[:, i]] += v
            bary[rows, d - rank[:, i] + 1] -= v
        bary[:, 0] += F32(1.0) + bary[:, d + 1]
        keys = np.zeros((N, d + 1, d), np.int16)
        for rem in range(d + 1):
            canon = np.where(rank[:, :d] <= d - rem, rem, rem - (d + 1))
            keys[:, rem, :] = (rem0[:, :d] + canon.astype(F32)).astype(np.int16)
        ukeys, inv = np.unique(keys.reshape(-1, d), axis=0, return_inverse=True)
        M = len(ukeys)
        self.M = M
        self.offset = inv.reshape(N, d + 1).astype(np.int64)
        self.bary = np.ascontiguousarray(bary[:, :d + 1])
        self.n1 = np.zeros((d + 1, M), np.int64)
        self.n2 = np.zeros((d + 1, M), np.int64)
        wide = ukeys.astype(np.int32)
        self.keys = wide                                     # (M, d) the lattice points' keys, in id order
        for j in range(d + 1):
            a, b = wide - 1, wide + 1
            if j < d:
                a[:, j] = wide[:, j] + d
                b[:, j] = wide[:, j] - d
            self.n1[j] = self._find(wide, a)
            self.n2[j] = self._find(wide, b)

    @staticmethod
    def _find(ukeys, wanted):
        """Row index of every `wanted` key in `ukeys` (unique rows), -1 where absent."""
        M = len(ukeys)
        _, inv = np.unique(np.concatenate([ukeys, wanted]), axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        ids = np.full(inv.max() + 1, -1, np.int64)
        ids[inv[:M]] = np.arange(M)
        return ids[inv[M:]]

    def splat(self, x):
        """The sequential splat, contributors in (pixel, vertex) order: x (N, vs) float32 -> values (M + 1, vs) float32, row 0
        the absent neighbour (zeros), row id + 1 the lattice point id."""
        x = np.ascontiguousarray(x, dtype=F32)
        values = np.zeros((self.M + 1, x.shape[1]), F32)
        o = (self.offset + 1).reshape(-1)
        np.add.at(values, o, self.bary.reshape(-1, 1) * np.repeat(x, self.d + 1, axis=0))
        return values

    def blur(self, values, axes=None):
        """The axis blurs `old + 0.5 * (n1 + n2)` through double along `axes` in turn (default 0 .. d: lattice_compute's order;
        d .. 0 is its reverse = true); values as splat() leaves them."""
        for j in range(self.d + 1) if axes is None else axes:
            t = values[self.n1[j] + 1] + values[self.n2[j] + 1]
            new = np.zeros_like(values)
            new[1:] = (values[1:].astype(np.float64) + 0.5 * t.astype(np.float64)).astype(F32)
            values = new
        return values

    def slice(self, values):
        """values (M + 1, vs) -> (N, vs): sum over the vertices, in order, of (bary * value) * alpha."""
        d = self.d
        alpha = F32(1.0) / (F32(1.0) + F32(2.0 ** -d))
        out = np.zeros((self.N, values.shape[1]), F32)
        for j in range(d + 1):
            out = out + self.bary[:, j, None] * values[self.offset[:, j] + 1] * alpha
        return out

    def compute(self, x):
        """lattice_compute: x (N, vs) float32 -> (N, vs) float32."""
        return self.slice(self.blur(self.splat(x)))

    def norm(self):
        ones = self.compute(np.ones((self.N, 1), F32))
        return (1.0 / np.sqrt(ones.astype(np.float64) + 1e-20)).astype(F32)       # (N, 1)


def _three(v, n):
    a = np.asarray(v, dtype=np.float64).reshape(-1)
    return [F32(x) for x in (np.repeat(a, n) if a.size == 1 else a)]


def features(rgb, pos_xy, bi_xy, bi_rgb):
    """(Gaussian (N, 2), bilateral (N, 5)) float32 features: x / sx, y / sy, r / sr, g / sg, b / sb."""
    H, W = rgb.shape[:2]
    yy, xx = np.mgrid[0:H, 0:W]
    x, y = xx.reshape(-1).astype(F32), yy.reshape(-1).astype(F32)
    col = rgb.reshape(-1, 3).astype(F32)
    px, bx, bc = _three(pos_xy, 2), _three(bi_xy, 2), _three(bi_rgb, 3)
    fg = np.stack([x / px[0], y / px[1]], 1)
    fb = np.stack([x / bx[0], y / bx[1], col[:, 0] / bc[0], col[:, 1] / bc[1], col[:, 2] / bc[2]], 1)
    return fg.astype(F32), fb.astype(F32)


def as_matrix(compat, K):
    """A term's message weights as a (K, K) float32 matrix: a number w -> w I, a vector -> diag(v), a matrix as it is."""
    a = np.asarray(compat, dtype=F32)
    if a.ndim == 0:
        return np.diag(np.full(K, a, F32))
    if a.ndim == 1:
        return np.diag(a)
    assert a.shape == (K, K)
    return a


class MeanField:
    """The model of one image.  U: (K, H * W) float32 energies.  Marginals are (K, H, W) float32, as the solver returns them."""

    def __init__(self, rgb, U, pos_xy=3.0, bi_xy=50.0, bi_rgb=5.0):
        self.H, self.W = rgb.shape[:2]
        self.K = U.shape[0]
        self.U = np.ascontiguousarray(U.reshape(self.K, -1).T, dtype=F32)          # pixel-major (N, K), as the oracle holds it
        fg, fb = features(rgb, pos_xy, bi_xy, bi_rgb)
        self.lat = [Lattice(fg), Lattice(fb)]
        self.norm = [L.norm() for L in self.lat]
        self._zeros = (np.zeros((self.H, self.W, 3), np.uint8), np.zeros((self.K, self.H, self.W), F32))

    def _softmax(self, logit):
        """The oracle's exp_and_normalize of pixel-major logits: its mean-field with no iterations is softmax(-unary)."""
        planes = np.ascontiguousarray((-logit).T).reshape(self.K, self.H, self.W)
        _, q = OP.densecrf_variant(self._zeros[0], self._zeros[1], variant=0, unary=planes, iters=0)
        return np.ascontiguousarray(q.reshape(self.K, -1).T)

    def _rows(self, q):
        return np.ascontiguousarray(q.reshape(self.K, -1).T, dtype=F32)

    def _planes(self, rows):
        return np.ascontiguousarray(rows.T).reshape(self.K, self.H, self.W)

    def start(self):
        return self._planes(self._softmax(-self.U))

    def messages(self, q):
        """msg_t (N, K) of both terms at marginals q: norm * lattice(norm * Q)."""
        rows = self._rows(q)
        return [self.lat[t].compute(rows * self.norm[t]) * self.norm[t] for t in range(2)]

    def acc(self, q, compat_g, compat_b):
        """acc_t (N, K) of both terms: one float32 accumulator per output, k ascending, product and sum rounded apart."""
        out = []
        for msg, compat in zip(self.messages(q), (compat_g, compat_b)):
            M = as_matrix(compat, self.K)
            a = np.zeros_like(msg)
            for k in range(self.K):
                a = a + M[None, :, k] * msg[:, k, None]
            out.append(a)
        return out

    def step(self, q, compat_g, compat_b):
        ag, ab = self.acc(q, compat_g, compat_b)
        return self._planes(self._softmax((-self.U + ag) + ab))

    def run(self, iters, compat_g, compat_b):
        q = self.start()
        for _ in range(iters):
            q = self.step(q, compat_g, compat_b)
        return q

    def kl(self, q, compat_g, compat_b):
        """(KL divergence in float64, sum of |log max(Q, 1e-20)| + 1 + |U| + 2 (|acc_g| + |acc_b|): what a change of every
        marginal by one unit moves the divergence by, to first order)."""
        rows = self._rows(q).astype(np.float64)
        ag, ab = [a.astype(np.float64) for a in self.acc(q, compat_g, compat_b)]
        U = self.U.astype(np.float64)
        lg = np.log(np.maximum(rows, 1e-20))
        value = (rows * lg).sum() + (rows * U).sum() - (rows * ag).sum() - (rows * ab).sum()
        reach = (np.abs(lg) + 1.0 + np.abs(U) + 2.0 * (np.abs(ag) + np.abs(ab))).sum()
        return float(value), float(reach)


def labels_of(q):
    return np.argmax(q, axis=0).astype(np.uint8)


def brute_force(rgb, U, iters, pos_xy, bi_xy, bi_rgb, compat_g, compat_b):
    """Float64 mean-field with every kernel entry evaluated: k(i, j) = exp(-|f_i - f_j|^2 / 2) on the per-axis features, self
    term included, symmetric normalisation; Q <- softmax(-U + M_g (Q K_g) + M_b (Q K_b)).  U (K, H * W).  -> Q (K, H, W)."""
    H, W = rgb.shape[:2]
    K = U.shape[0]
    U = np.asarray(U, dtype=np.float64).reshape(K, -1)
    yy, xx = np.mgrid[0:H, 0:W]
    xy = np.stack([xx.reshape(-1), yy.reshape(-1)], 1).astype(np.float64)
    col = rgb.reshape(-1, 3).astype(np.float64)
    px, bx, bc = (np.array(_three(v, n), np.float64) for v, n in ((pos_xy, 2), (bi_xy, 2), (bi_rgb, 3)))

    def kernel(f):
        sq = (f * f).sum(1)
        km = np.exp(-0.5 * np.maximum(sq[:, None] + sq[None, :] - 2.0 * (f @ f.T), 0.0))
        nrm = 1.0 / np.sqrt(km.sum(1) + 1e-20)
        return km * nrm[:, None] * nrm[None, :]
    Kg, Kb = kernel(xy / px), kernel(np.concatenate([xy / bx, col / bc], 1))
    Mg, Mb = as_matrix(compat_g, K).astype(np.float64), as_matrix(compat_b, K).astype(np.float64)

    def softmax(t):
        e = np.exp(t - t.max(0, keepdims=True))
        return e / e.sum(0, keepdims=True)
    Q = softmax(-U)
    for _ in range(iters):
        Q = softmax(-U + Mg @ (Q @ Kg) + Mb @ (Q @ Kb))
    return Q.reshape(K, H, W)
