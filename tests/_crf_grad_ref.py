"""Float64 reference for the gradients of the feature-term mean-field (pnp_crf_backward_terms, FeatureCRF.marginals).

Every term's operator is built explicitly from the lattice of tests/_crf_general_ref.Lattice (offset, bary, n1, n2):

    A_t = alpha N S^T B_d .. B_1 B_0 S N

with S the splat (M x N: the float32 barycentric weights, cast to float64), B_j = I + 0.5 (P1_j + P2_j) one blur axis (P1_j, P2_j
the neighbour permutations of axis j, absent neighbours dropped), alpha = 1 / (1 + 2^-d) and N = diag(1 / sqrt(rowsum + 1e-20)),
rowsum = alpha S^T B_d .. B_0 S 1, in float64.  The mean-field is torch float64 on the CPU,

    Q_0 = softmax(-U);  Q_i = softmax(-U + sum_t (A_t Q_{i-1}) C_t^T)

and the gradients are torch autograd's for a fixed random cotangent.  Each B_j is symmetric but their product is not: with
`transposed` every A_t is replaced by its transpose, which is what a backward pass that kept the forward's blur order would
differentiate -- the wrong answer the GPU test's bound has to tell from the right one."""
import functools

import numpy as np
import scipy.sparse as sp
import torch

import _crf_terms_ref as TR

ITERS = 5

# max |g - g_ref| / max |g_ref| per gradient tensor that the GPU test allows.  Measured on the MI355X over GRAD_CASES by
# tools/crf_bench.py --grad_errors (profiles/crf_grad.json, `errors`, which tests/test_crf_grad_cpu.py
# holds these two constants to): the worst is WORST_MEASURED; the bound is ten times that, rounded up to a power of ten, and
# may not exceed 1e-3 (a thirteenth of the smallest discrepancy of a backward pass with the forward's blur order)
WORST_MEASURED = 4.7e-6         # the matrix gradient of the (33, 17, 21) d6 case
BOUND = 1e-4


def _matrix(K, w, seed):
    return (w * np.eye(K) + 0.3 * np.random.default_rng(seed).normal(size=(K, K))).astype(np.float32)


def _vector(K, w, seed):
    return (w + 0.3 * np.random.default_rng(seed).normal(size=K)).astype(np.float32)


# (index into TR.CASES, compatibility kinds per term): one of each kind among them, every case at a dispatch that can go wrong --
# the commuting axes of d1; scalar + vector; three terms with two matrices; the widest D1; Kp = 152
GRAD_CASES = [(0, "s"), (2, "sv"), (3, "smm"), (5, "m"), (6, "mm")]


@functools.lru_cache(maxsize=None)
def case(index, kinds):
    """-> (shape, names, compats): a float for 's', a (K,) float32 vector for 'v', a (K, K) float32 matrix for 'm'."""
    shape, names, weights = TR.CASES[index]
    K = shape[0]
    compats = []
    for t, (kind, w) in enumerate(zip(kinds, weights)):
        compats.append(float(w) if kind == "s" else _vector(K, w, 100 + t) if kind == "v" else _matrix(K, w, 200 + t))
    return shape, names, tuple(compats)


@functools.lru_cache(maxsize=None)
def cotangent(shape):
    """(K, H, W) float32 N(0, 1), seed 11 + K; read-only."""
    g = np.random.default_rng(11 + shape[0]).normal(size=shape).astype(np.float32)
    g.setflags(write=False)
    return g


def _operator(L):
    """Dense float64 A of one Lattice."""
    N, d, M = L.N, L.d, L.M
    rows = L.offset.reshape(-1)
    cols = np.repeat(np.arange(N), d + 1)
    S = sp.csr_matrix((L.bary.reshape(-1).astype(np.float64), (rows, cols)), shape=(M, N))
    P = sp.identity(M, format="csr", dtype=np.float64)
    ids = np.arange(M)
    for j in range(d + 1):
        B = sp.identity(M, format="csr", dtype=np.float64)
        for n in (L.n1[j], L.n2[j]):
            ok = n >= 0
            B = B + 0.5 * sp.csr_matrix((np.ones(ok.sum()), (ids[ok], n[ok])), shape=(M, M))
        P = B @ P                                       # B_j .. B_0
    alpha = 1.0 / (1.0 + 2.0 ** -d)
    F = alpha * (S.T @ P @ S).toarray()
    nrm = 1.0 / np.sqrt(F.sum(1) + 1e-20)
    return nrm[:, None] * F * nrm[None, :]


@functools.lru_cache(maxsize=None)
def operators(shape, names):
    """Per term the dense (N, N) float64 torch operator A_t of a case of TR.CASES."""
    return tuple(torch.from_numpy(_operator(L)) for L in TR.model(shape, names).lat)


def meanfield(U, ops, compats, iters=ITERS):
    """U: (K, N) float64 torch; ops: (N, N); compats: 0-d, (K,) or (K, K) float64 torch.  -> Q (K, N), differentiable."""
    Ur = U.T
    Q = torch.softmax(-Ur, 1)
    for _ in range(iters):
        logit = -Ur
        for A, c in zip(ops, compats):
            msg = A @ Q
            logit = logit + (c * msg if c.ndim < 2 else msg @ c.T)
        Q = torch.softmax(logit, 1)
    return Q.T


def forward(shape, names, compats, iters=ITERS):
    """-> Q (K, H, W) float64 numpy."""
    U, _ = TR.case_inputs(shape, names)
    with torch.no_grad():
        q = meanfield(torch.from_numpy(np.asarray(U, np.float64)), operators(shape, names),
                      [torch.as_tensor(np.asarray(c, np.float64)) for c in compats], iters)
    return q.numpy().reshape(shape)


def loss_inputs(shape, names, compats, transposed=False):
    U, _ = TR.case_inputs(shape, names)
    ops = operators(shape, names)
    if transposed:
        ops = tuple(A.T.contiguous() for A in ops)
    U = torch.from_numpy(np.array(U, np.float64)).requires_grad_(True)
    cs = [torch.from_numpy(np.array(c, np.float64)).requires_grad_(True) for c in compats]
    g = torch.from_numpy(cotangent(shape).astype(np.float64).reshape(shape[0], -1))
    return U, ops, cs, g


@functools.lru_cache(maxsize=None)
def gradients(index, kinds, transposed=False, iters=ITERS):
    """-> (grad_unary (K, H, W), [grad_compat per term]) float64 numpy of sum(cotangent * Q_iters); read-only."""
    shape, names, compats = case(index, kinds)
    U, ops, cs, g = loss_inputs(shape, names, compats, transposed)
    (meanfield(U, ops, cs, iters) * g).sum().backward()
    out = [U.grad.numpy().reshape(shape)] + [c.grad.numpy() for c in cs]
    for a in out:
        a.setflags(write=False)
    return out[0], out[1:]


def rel_err(got, ref):
    """max |got - ref| / max |ref|"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max() / np.abs(ref).max())
