"""pydensecrf.densecrf of the general shim (pnp-ovss_amd/shims/general): DenseCRF2D with one Gaussian and one bilateral term,
run by pnp_ovss.crf on the GPU.  With a number for compat and equal widths it hands pnp_ovss.crf what the shim under
pnp-ovss_amd/shims hands it: the same marginals, bit for bit.

Covered: setUnaryEnergy; addPairwiseGaussian / addPairwiseBilateral with a number or per-axis tuple for sxy / srgb and a number,
a (K,) vector or a (K, K) matrix for compat; inference(n); map(n); the startInference / stepInference / klDivergence loop.
Still NotImplementedError, never approximated: a second Gaussian or bilateral term, addPairwiseEnergy / DenseCRF (arbitrary
features), CONST_KERNEL / FULL_KERNEL, any normalisation but NORMALIZE_SYMMETRIC.

compat is converted to pnp_ovss.crf's message weights in ONE place, pnp_ovss.crf.message_weights: a number w -> Potts weight w; a vector v ->
diag(-v); a matrix m -> -0.5 * (m + m^T).  That is densecrf's PottsCompatibility / DiagonalCompatibility / MatrixCompatibility
(a label-cost matrix, symmetrised, applied with a minus sign to the filtered marginals) AS REMEMBERED: neither pydensecrf nor
densecrf's sources were at hand when this was written, and nothing in this repository pins the sign, the symmetrisation or the
klDivergence formula to the library (oracle/README.md).  Check them against your pydensecrf before relying on the vector /
matrix forms or on KL values.
"""
import numbers

import numpy as np

CONST_KERNEL, DIAG_KERNEL, FULL_KERNEL = 0, 1, 2
NO_NORMALIZATION, NORMALIZE_BEFORE, NORMALIZE_AFTER, NORMALIZE_SYMMETRIC = 0, 1, 2, 3

_KERNELS = {CONST_KERNEL: "CONST_KERNEL", DIAG_KERNEL: "DIAG_KERNEL", FULL_KERNEL: "FULL_KERNEL"}
_NORMS = {NO_NORMALIZATION: "NO_NORMALIZATION", NORMALIZE_BEFORE: "NORMALIZE_BEFORE", NORMALIZE_AFTER: "NORMALIZE_AFTER",
          NORMALIZE_SYMMETRIC: "NORMALIZE_SYMMETRIC"}


def message_weights(compat, nlabels, where):
    """pydensecrf's compat -> (Potts weight, None) for a number, (None, (K, K) float32 message weights) for a vector
    (diag(-v)) or a matrix (-0.5 * (m + m^T)): see the module docstring.  The conversion itself is pnp_ovss.crf's."""
    from pnp_ovss import crf
    return crf.message_weights(compat, nlabels, where)


def _widths(v, n, name, where):
    if isinstance(v, numbers.Real) and not isinstance(v, bool):
        vals = [float(v)] * n
    else:
        vals = [float(x) for x in np.asarray(v).reshape(-1)]
        if len(vals) != n:
            raise ValueError(f"{where}: {name} is a scalar or {n} values, not {v!r}")
    if not all(x > 0 for x in vals):
        raise ValueError(f"{where}: {name} must be positive, not {v!r}")
    return tuple(vals)


def _defaults_only(kernel, normalization, where):
    if kernel != DIAG_KERNEL:
        raise NotImplementedError(f"{where}: kernel={_KERNELS.get(kernel, kernel)} is not supported (DIAG_KERNEL only)")
    if normalization != NORMALIZE_SYMMETRIC:
        raise NotImplementedError(f"{where}: normalization={_NORMS.get(normalization, normalization)} is not supported "
                                  f"(NORMALIZE_SYMMETRIC only)")


class _Marginals:
    """What startInference hands out as Q: a live view of the solver's marginals -- np.array(Q) reads them, (nlabels, h * w)."""

    def __init__(self, owner):
        self._owner = owner

    def __array__(self, dtype=None, copy=None):
        q = self._owner._read()
        return q if dtype is None else q.astype(dtype)


class DenseCRF2D:
    def __init__(self, w, h, nlabels):
        self.w, self.h, self.nlabels = int(w), int(h), int(nlabels)
        if self.w < 1 or self.h < 1 or self.nlabels < 2:
            raise ValueError(f"DenseCRF2D({w}, {h}, {nlabels}): positive size and at least two labels")
        self._U = None
        self._gauss = None       # (sxy, Potts weight or None, message weights or None)
        self._bilat = None       # (sxy, srgb, image, Potts weight or None, message weights or None)
        self._solver = None      # the pnp_ovss.crf solver of a started stepwise inference

    def setUnaryEnergy(self, U):
        U = np.asarray(U)
        if U.dtype != np.float32:
            raise ValueError(f"setUnaryEnergy: float32 expected, not {U.dtype}")
        if U.shape != (self.nlabels, self.h * self.w):
            raise ValueError(f"setUnaryEnergy: shape {U.shape}, expected ({self.nlabels}, {self.h * self.w})")
        if not U.flags["C_CONTIGUOUS"]:
            raise ValueError("setUnaryEnergy: a C-contiguous array is required")
        self._U = U.copy()

    def addPairwiseGaussian(self, sxy, compat, kernel=DIAG_KERNEL, normalization=NORMALIZE_SYMMETRIC):
        where = "addPairwiseGaussian"
        if self._gauss is not None:
            raise NotImplementedError(f"{where}: a second Gaussian term is not supported")
        _defaults_only(kernel, normalization, where)
        self._gauss = (_widths(sxy, 2, "sxy", where),) + message_weights(compat, self.nlabels, where)

    def addPairwiseBilateral(self, sxy, srgb, rgbim, compat, kernel=DIAG_KERNEL, normalization=NORMALIZE_SYMMETRIC):
        where = "addPairwiseBilateral"
        if self._bilat is not None:
            raise NotImplementedError(f"{where}: a second bilateral term is not supported")
        _defaults_only(kernel, normalization, where)
        im = np.asarray(rgbim)
        if im.dtype != np.uint8 or im.shape != (self.h, self.w, 3):
            raise ValueError(f"{where}: rgbim is ({self.h}, {self.w}, 3) uint8, not {im.shape} {im.dtype}")
        self._bilat = (_widths(sxy, 2, "sxy", where), _widths(srgb, 3, "srgb", where), np.ascontiguousarray(im).copy()) + \
            message_weights(compat, self.nlabels, where)

    def _params(self):
        """-> (image, DenseCRF.run keyword arguments).  The Gaussian term first, as the reference adds them; a term that was
        not added has weight 0 (its lattice is built at the default width and contributes nothing)."""
        if self._U is None:
            raise ValueError("inference: setUnaryEnergy was not called")
        from pnp_ovss import crf
        p = dict(crf.DEFAULTS)
        p["pos_w"], p["bi_w"] = 0.0, 0.0
        p["pos_compat"] = p["bi_compat"] = None
        image = np.zeros((self.h, self.w, 3), np.uint8)
        if self._gauss is not None:
            p["pos_xy"], w, p["pos_compat"] = self._gauss
            p["pos_w"] = 0.0 if w is None else w
        if self._bilat is not None:
            p["bi_xy"], p["bi_rgb"], image, w, p["bi_compat"] = self._bilat
            p["bi_w"] = 0.0 if w is None else w
        return image, p

    def inference(self, n):
        """n mean-field iterations -> the marginals, float32 (nlabels, h * w)."""
        image, p = self._params()
        from pnp_ovss import crf
        p["iters"] = int(n)
        _, q = crf.densecrf(self._U, image, **p)
        return q.reshape(self.nlabels, self.h * self.w).cpu().numpy()

    def map(self, n):
        """argmax over the labels of inference(n): (h * w,) label indices."""
        return np.argmax(self.inference(n), axis=0)

    # ---- pydensecrf's convergence-monitored loop:
    #      Q, tmp1, tmp2 = d.startInference(); for i in range(n): d.stepInference(Q, tmp1, tmp2); kl = d.klDivergence(Q)
    def startInference(self):
        """-> (Q, tmp1, tmp2).  Q: a live view of the marginals (np.array(Q) reads them); tmp1 / tmp2: placeholders that
        stepInference accepts (the solver owns its workspace)."""
        image, p = self._params()
        from pnp_ovss import crf
        p["iters"] = 0
        crf.densecrf(self._U, image, want_q=False, **p)          # sets the batch and the compatibilities; Q = softmax(-U)
        self._solver = crf.module_solver(self._U)
        self._token = self._solver.batch_token()
        return _Marginals(self), None, None

    def _started(self, what):
        if self._solver is None or self._solver.batch_token() != self._token:
            raise RuntimeError(f"{what}: no inference is in progress (startInference first; another CRF run on this device "
                               f"ends it)")
        return self._solver

    def stepInference(self, Q=None, tmp1=None, tmp2=None):
        self._started("stepInference").step(1)

    def klDivergence(self, Q=None):
        return self._started("klDivergence").kl()[0]

    def _read(self):
        _, q = self._started("np.array(Q)").read(want_q=True, want_labels=False)
        return q[0].reshape(self.nlabels, self.h * self.w).cpu().numpy()

    def addPairwiseEnergy(self, *a, **k):
        raise NotImplementedError("addPairwiseEnergy (arbitrary features) is not supported by the pnp_ovss shim")

    def setUnary(self, *a, **k):
        raise NotImplementedError("setUnary (a Unary object) is not supported by the pnp_ovss shim: use setUnaryEnergy")


class DenseCRF:
    def __init__(self, *a, **k):
        raise NotImplementedError("DenseCRF (arbitrary pairwise features) is not supported by the pnp_ovss shim: use DenseCRF2D")
