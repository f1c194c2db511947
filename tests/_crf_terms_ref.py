"""Reference for the DenseCRF with any number of pairwise terms over caller-supplied features (pnp_crf_set_batch_terms,
pnp_ovss.crf.FeatureCRF): the T-term mean-field of include/pnp_hip.h built from tests/_crf_general_ref.py -- its Lattice (the
embedding, the sequential splat, the axis blurs through double, the slice times alpha, the symmetric normaliser) per term and
its softmax (the oracle's exp_and_normalize) -- with the update

    acc_t[l] = sum_k M_t[l][k] * msg_t[k]     (float32, one accumulator, k ascending; a scalar: w_t * msg_t[l])
    logit    = ((-U + acc_0) + acc_1) + ... + acc_{T-1}

Also here: the inputs of the tests (test_crf_op_gpu.inputs plus a depth plane), their feature sets and cases, and a float64 brute
force over every kernel entry for statistical checks on small images."""
import functools

import numpy as np

import _crf_general_ref as G
import test_crf_op_gpu as T

F32 = np.float32
ITERS = 5


@functools.lru_cache(maxsize=None)
def depth_plane(K, H, W):
    """0.5 + 0.4 sin(x / 7) cos(y / 5) + N(0, 0.02), seed 7 + K: (H, W) float32, read-only."""
    rng = np.random.default_rng(7 + K)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    d = (0.5 + 0.4 * np.sin(xx / 7.0) * np.cos(yy / 5.0) + rng.normal(0, 0.02, (H, W))).astype(F32)
    d.setflags(write=False)
    return d


def _div(a, w):
    return np.asarray(a, dtype=F32) / F32(w)


def feature_set(name, rgb, depth):
    """(d, H, W) float32 features of one of the sets d1 .. d6; every quotient a float32 division of float32 operands."""
    H, W = rgb.shape[:2]
    yy, xx = np.mgrid[0:H, 0:W]
    r, g, b = (rgb[:, :, c] for c in range(3))
    sets = {
        "d1": [(r, 8)],
        "d2": [(xx, 3), (yy, 3)],
        "d3": [(xx, 20), (yy, 20), (g, 6)],
        "d4": [(xx, 30), (yy, 30), (r, 7), (depth, 0.2)],
        "d5": [(xx, 50), (yy, 50), (r, 5), (g, 5), (b, 5)],
        "d6": [(xx, 50), (yy, 50), (r, 5), (g, 5), (b, 5), (depth, 0.1)],
    }
    f = np.stack([_div(a, w) for a, w in sets[name]])
    f.setflags(write=False)
    return f


# ((K, H, W), feature sets, weights)
CASES = [((3, 13, 17), ("d1",), (5,)),
         ((3, 13, 17), ("d3",), (8,)),
         ((3, 13, 17), ("d2", "d4"), (3, 6)),
         ((21, 23, 31), ("d2", "d3", "d6"), (3, 4, 6)),
         ((5, 19, 23), ("d2", "d5", "d4", "d6"), (3, 5, 3, 3)),
         ((33, 17, 21), ("d6",), (10,)),
         ((150, 9, 13), ("d3", "d4"), (5, 5))]


@functools.lru_cache(maxsize=None)
def case_inputs(shape, names):
    """-> (U (K, H*W), [features (d, H, W)] per name) of a case, read-only."""
    K, H, W = shape
    rgb, U = T.inputs(K, H, W)
    depth = depth_plane(K, H, W)
    return U, [feature_set(n, rgb, depth) for n in names]


class _Softmax(G.MeanField):
    """G.MeanField's softmax (the oracle's exp_and_normalize) for K labels on H x W pixels, without its two lattices."""

    def __init__(self, K, H, W):
        self.K, self.H, self.W = K, H, W
        self._zeros = (np.zeros((H, W, 3), np.uint8), np.zeros((K, H, W), F32))


class TermsMeanField:
    """The model of one image.  U: (K, H*W) float32; features: per term (d, H, W) or (d, H*W) float32.  Marginals (K, H, W)."""

    def __init__(self, U, H, W, features):
        self.K, self.H, self.W = U.shape[0], H, W
        self.U = np.ascontiguousarray(U.reshape(self.K, -1).T, dtype=F32)
        self.lat = [G.Lattice(np.ascontiguousarray(np.asarray(f).reshape(f.shape[0], -1).T)) for f in features]
        self.norm = [L.norm() for L in self.lat]
        self.soft = _Softmax(self.K, H, W)

    def start(self):
        return self.soft._planes(self.soft._softmax(-self.U))

    def step(self, q, compats):
        rows = self.soft._rows(q)
        logit = -self.U
        for L, nrm, compat in zip(self.lat, self.norm, compats):
            msg = L.compute(rows * nrm) * nrm
            c = np.asarray(compat, dtype=F32)
            if c.ndim == 0:
                acc = c * msg
            else:
                M = G.as_matrix(c, self.K)
                acc = np.zeros_like(msg)
                for k in range(self.K):
                    acc = acc + M[None, :, k] * msg[:, k, None]
            logit = logit + acc
        return self.soft._planes(self.soft._softmax(logit))

    def run(self, iters, compats):
        q = self.start()
        for _ in range(iters):
            q = self.step(q, compats)
        return q


@functools.lru_cache(maxsize=None)
def model(shape, names):
    U, feats = case_inputs(shape, names)
    return TermsMeanField(U, shape[1], shape[2], feats)


def reference(shape, names, compats, iters=ITERS):
    """-> (labels, marginals) of the reference, read-only."""
    q = model(shape, names).run(iters, compats)
    lab = G.labels_of(q)
    q.setflags(write=False)
    lab.setflags(write=False)
    return lab, q


def brute_force(U, features, compats, iters):
    """Float64 mean-field with every kernel entry evaluated: k_t(i, j) = exp(-|f_i - f_j|^2 / 2) on term t's features, self term
    included, symmetric normalisation; Q <- softmax(-U + sum_t M_t (Q K_t)).  U (K, N); features (d, ...).  -> Q (K, N)."""
    K = U.shape[0]
    U = np.asarray(U, dtype=np.float64).reshape(K, -1)

    def kernel(f):
        f = np.asarray(f, dtype=np.float64).reshape(f.shape[0], -1).T
        sq = (f * f).sum(1)
        km = np.exp(-0.5 * np.maximum(sq[:, None] + sq[None, :] - 2.0 * (f @ f.T), 0.0))
        nrm = 1.0 / np.sqrt(km.sum(1) + 1e-20)
        return km * nrm[:, None] * nrm[None, :]
    Ks = [kernel(f) for f in features]
    Ms = [G.as_matrix(c, K).astype(np.float64) for c in compats]

    def softmax(t):
        e = np.exp(t - t.max(0, keepdims=True))
        return e / e.sum(0, keepdims=True)
    Q = softmax(-U)
    for _ in range(iters):
        Q = softmax(-U + sum(M @ (Q @ Kt) for M, Kt in zip(Ms, Ks)))
    return Q
