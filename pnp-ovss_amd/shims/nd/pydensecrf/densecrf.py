"""pydensecrf.densecrf of the N-D shim (pnp-ovss_amd/shims/nd): DenseCRF(N, K) and DenseCRF2D(W, H, K) with any number of
pairwise terms, run by pnp_ovss.crf.FeatureCRF on the GPU.

Covered: setUnaryEnergy; addPairwiseEnergy(features (D, N) float32 with D <= 6, compat); on DenseCRF2D also
addPairwiseGaussian / addPairwiseBilateral, any number of each, with a number or per-axis tuple for sxy / srgb; compat as a
number, a (K,) vector or a (K, K) matrix; inference(n); map(n); startInference / stepInference.  Terms act in the order they
were added.  DenseCRF2D's own terms use the features of the other shims (x / sx, y / sy, then r, g, b over srgb), so one
Gaussian and one bilateral term with numbers for compat give their marginals bit for bit.
Still NotImplementedError, never approximated: klDivergence, CONST_KERNEL / FULL_KERNEL, any normalisation but
NORMALIZE_SYMMETRIC, setUnary.

compat becomes pnp_ovss.crf's message weights in pnp_ovss.crf.message_weights (a number w -> Potts weight w; a vector v ->
diag(-v); a matrix m -> -0.5 * (m + m^T)): this project's reading of densecrf, pinned by nothing the reference holds -- see
pnp-ovss_amd/shims/general/pydensecrf/densecrf.py.
"""
import numpy as np

CONST_KERNEL, DIAG_KERNEL, FULL_KERNEL = 0, 1, 2
NO_NORMALIZATION, NORMALIZE_BEFORE, NORMALIZE_AFTER, NORMALIZE_SYMMETRIC = 0, 1, 2, 3

_KERNELS = {CONST_KERNEL: "CONST_KERNEL", DIAG_KERNEL: "DIAG_KERNEL", FULL_KERNEL: "FULL_KERNEL"}
_NORMS = {NO_NORMALIZATION: "NO_NORMALIZATION", NORMALIZE_BEFORE: "NORMALIZE_BEFORE", NORMALIZE_AFTER: "NORMALIZE_AFTER",
          NORMALIZE_SYMMETRIC: "NORMALIZE_SYMMETRIC"}


def _defaults_only(kernel, normalization, where):
    if kernel != DIAG_KERNEL:
        raise NotImplementedError(f"{where}: kernel={_KERNELS.get(kernel, kernel)} is not supported (DIAG_KERNEL only)")
    if normalization != NORMALIZE_SYMMETRIC:
        raise NotImplementedError(f"{where}: normalization={_NORMS.get(normalization, normalization)} is not supported "
                                  f"(NORMALIZE_SYMMETRIC only)")


def _grid(n):
    """Any H x W = n serves a DenseCRF(N, K): the solver's pixel grid only tiles the work, no result depends on it."""
    for w in range(int(n ** 0.5), 15, -1):
        if n % w == 0:
            return n // w, w
    return 1, n


class _Marginals:
    """What startInference hands out as Q: a live view of the solver's marginals -- np.array(Q) reads them, (nlabels, N)."""

    def __init__(self, owner):
        self._owner = owner

    def __array__(self, dtype=None, copy=None):
        q = self._owner._read()
        return q if dtype is None else q.astype(dtype)


class DenseCRF:
    def __init__(self, nvar, nlabels):
        self.n, self.nlabels = int(nvar), int(nlabels)
        if self.n < 1 or self.nlabels < 2:
            raise ValueError(f"DenseCRF({nvar}, {nlabels}): at least one variable and two labels")
        self._size = _grid(self.n)
        self._U = None
        self._terms = []         # (features (D, N) float32, Potts weight or None, message weights or None)
        self._solver = None      # the pnp_ovss.crf solver of a started stepwise inference

    def setUnaryEnergy(self, U):
        U = np.asarray(U)
        if U.dtype != np.float32:
            raise ValueError(f"setUnaryEnergy: float32 expected, not {U.dtype}")
        if U.shape != (self.nlabels, self.n):
            raise ValueError(f"setUnaryEnergy: shape {U.shape}, expected ({self.nlabels}, {self.n})")
        if not U.flags["C_CONTIGUOUS"]:
            raise ValueError("setUnaryEnergy: a C-contiguous array is required")
        self._U = U.copy()

    def _add(self, features, compat, where):
        from pnp_ovss import crf
        self._terms.append((features,) + crf.message_weights(compat, self.nlabels, where))

    def addPairwiseEnergy(self, features, compat, kernel=DIAG_KERNEL, normalization=NORMALIZE_SYMMETRIC):
        where = "addPairwiseEnergy"
        _defaults_only(kernel, normalization, where)
        f = np.asarray(features)
        if f.dtype != np.float32:
            raise ValueError(f"{where}: float32 features expected, not {f.dtype}")
        if f.ndim != 2 or f.shape[1] != self.n:
            raise ValueError(f"{where}: features are (D, {self.n}), not {f.shape}")
        if not 1 <= f.shape[0] <= 6:
            raise NotImplementedError(f"{where}: {f.shape[0]} features per variable; the pnp_ovss shim holds 1..6")
        self._add(np.ascontiguousarray(f).copy(), compat, where)

    def _run(self, n, want_q):
        if self._U is None:
            raise ValueError("inference: setUnaryEnergy was not called")
        if not self._terms:
            raise ValueError("inference: no pairwise term was added")
        from pnp_ovss import crf
        h, w = self._size
        terms = [crf.Term([f], wgt if m is None else m) for f, wgt, m in self._terms]
        plan = crf.plan_terms([(h, w)], [self.nlabels], [t.dims for t in terms])
        solver = crf.feature_solver(plan)
        _, q = solver.run([self._U.reshape(self.nlabels, h, w)], terms, iters=int(n), want_q=want_q)
        return solver, q

    def inference(self, n):
        """n mean-field iterations -> the marginals, float32 (nlabels, N)."""
        _, q = self._run(n, True)
        return q[0].reshape(self.nlabels, self.n).cpu().numpy()

    def map(self, n):
        """argmax over the labels of inference(n): (N,) label indices."""
        return np.argmax(self.inference(n), axis=0)

    def startInference(self):
        """-> (Q, tmp1, tmp2).  Q: a live view of the marginals (np.array(Q) reads them); tmp1 / tmp2: placeholders."""
        self._solver, _ = self._run(0, False)
        self._token = self._solver.batch_token()
        return _Marginals(self), None, None

    def _started(self, what):
        if self._solver is None or self._solver.batch_token() != self._token:
            raise RuntimeError(f"{what}: no inference is in progress (startInference first; another CRF run on this device "
                               f"ends it)")
        return self._solver

    def stepInference(self, Q=None, tmp1=None, tmp2=None):
        self._started("stepInference").step(1)

    def _read(self):
        _, q = self._started("np.array(Q)").read(want_q=True, want_labels=False)
        return q[0].reshape(self.nlabels, self.n).cpu().numpy()

    def klDivergence(self, Q=None):
        raise NotImplementedError("klDivergence is not supported for terms over arbitrary features by the pnp_ovss shim")

    def setUnary(self, *a, **k):
        raise NotImplementedError("setUnary (a Unary object) is not supported by the pnp_ovss shim: use setUnaryEnergy")


class DenseCRF2D(DenseCRF):
    def __init__(self, w, h, nlabels):
        if int(w) < 1 or int(h) < 1:
            raise ValueError(f"DenseCRF2D({w}, {h}, {nlabels}): positive size and at least two labels")
        DenseCRF.__init__(self, int(w) * int(h), nlabels)
        self.w, self.h = int(w), int(h)
        self._size = (self.h, self.w)

    def addPairwiseGaussian(self, sxy, compat, kernel=DIAG_KERNEL, normalization=NORMALIZE_SYMMETRIC):
        where = "addPairwiseGaussian"
        _defaults_only(kernel, normalization, where)
        from pnp_ovss import crf
        try:
            f = crf.position_features([self._size], sxy)[0]
        except ValueError as e:
            raise ValueError(f"{where}: {e}") from None
        self._add(f.reshape(2, -1), compat, where)

    def addPairwiseBilateral(self, sxy, srgb, rgbim, compat, kernel=DIAG_KERNEL, normalization=NORMALIZE_SYMMETRIC):
        where = "addPairwiseBilateral"
        _defaults_only(kernel, normalization, where)
        im = np.asarray(rgbim)
        if im.dtype != np.uint8 or im.shape != (self.h, self.w, 3):
            raise ValueError(f"{where}: rgbim is ({self.h}, {self.w}, 3) uint8, not {im.shape} {im.dtype}")
        from pnp_ovss import crf
        try:
            f = crf.image_features([im], sxy, srgb)[0]
        except ValueError as e:
            raise ValueError(f"{where}: {e}") from None
        self._add(f.reshape(5, -1), compat, where)
