"""pydensecrf.densecrf: DenseCRF2D with one Gaussian and one bilateral Potts term, run by pnp_ovss.crf on the GPU."""
import numbers

import numpy as np

CONST_KERNEL, DIAG_KERNEL, FULL_KERNEL = 0, 1, 2
NO_NORMALIZATION, NORMALIZE_BEFORE, NORMALIZE_AFTER, NORMALIZE_SYMMETRIC = 0, 1, 2, 3

_KERNELS = {CONST_KERNEL: "CONST_KERNEL", DIAG_KERNEL: "DIAG_KERNEL", FULL_KERNEL: "FULL_KERNEL"}
_NORMS = {NO_NORMALIZATION: "NO_NORMALIZATION", NORMALIZE_BEFORE: "NORMALIZE_BEFORE", NORMALIZE_AFTER: "NORMALIZE_AFTER",
          NORMALIZE_SYMMETRIC: "NORMALIZE_SYMMETRIC"}


def _scalar_compat(compat, where):
    if isinstance(compat, numbers.Real) and not isinstance(compat, bool):
        return float(compat)
    raise NotImplementedError(f"{where}: compat={type(compat).__name__} -- only a scalar Potts compatibility is supported "
                              f"(no per-label vector or matrix)")


def _isotropic(v, n, name, where):
    if isinstance(v, numbers.Real) and not isinstance(v, bool):
        return float(v)
    vals = [float(x) for x in np.asarray(v).reshape(-1)]
    if len(vals) != n:
        raise ValueError(f"{where}: {name} is a scalar or {n} values, not {v!r}")
    if any(x != vals[0] for x in vals):
        raise NotImplementedError(f"{where}: anisotropic {name}={v!r} is not supported (one width for all axes)")
    return vals[0]


def _defaults_only(kernel, normalization, where):
    if kernel != DIAG_KERNEL:
        raise NotImplementedError(f"{where}: kernel={_KERNELS.get(kernel, kernel)} is not supported (DIAG_KERNEL only)")
    if normalization != NORMALIZE_SYMMETRIC:
        raise NotImplementedError(f"{where}: normalization={_NORMS.get(normalization, normalization)} is not supported "
                                  f"(NORMALIZE_SYMMETRIC only)")


class DenseCRF2D:
    def __init__(self, w, h, nlabels):
        self.w, self.h, self.nlabels = int(w), int(h), int(nlabels)
        if self.w < 1 or self.h < 1 or self.nlabels < 2:
            raise ValueError(f"DenseCRF2D({w}, {h}, {nlabels}): positive size and at least two labels")
        self._U = None
        self._gauss = None       # (sxy, compat)
        self._bilat = None       # (sxy, srgb, image, compat)

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
        self._gauss = (_isotropic(sxy, 2, "sxy", where), _scalar_compat(compat, where))

    def addPairwiseBilateral(self, sxy, srgb, rgbim, compat, kernel=DIAG_KERNEL, normalization=NORMALIZE_SYMMETRIC):
        where = "addPairwiseBilateral"
        if self._bilat is not None:
            raise NotImplementedError(f"{where}: a second bilateral term is not supported")
        _defaults_only(kernel, normalization, where)
        im = np.asarray(rgbim)
        if im.dtype != np.uint8 or im.shape != (self.h, self.w, 3):
            raise ValueError(f"{where}: rgbim is ({self.h}, {self.w}, 3) uint8, not {im.shape} {im.dtype}")
        self._bilat = (_isotropic(sxy, 2, "sxy", where), _isotropic(srgb, 3, "srgb", where), np.ascontiguousarray(im).copy(),
                       _scalar_compat(compat, where))

    def inference(self, n):
        """n mean-field iterations -> the marginals, float32 (nlabels, h * w)."""
        if self._U is None:
            raise ValueError("inference: setUnaryEnergy was not called")
        from pnp_ovss import crf
        # the Gaussian term first, as the reference adds them; a term that was not added has weight 0 (its lattice is
        # built at the default width and contributes nothing)
        p = dict(crf.DEFAULTS)
        p["iters"] = int(n)
        p["pos_w"], p["bi_w"] = 0.0, 0.0
        image = np.zeros((self.h, self.w, 3), np.uint8)
        if self._gauss is not None:
            p["pos_xy"], p["pos_w"] = self._gauss
        if self._bilat is not None:
            p["bi_xy"], p["bi_rgb"], image, p["bi_w"] = self._bilat
        _, q = crf.densecrf(self._U, image, **p)
        return q.reshape(self.nlabels, self.h * self.w).cpu().numpy()

    def addPairwiseEnergy(self, *a, **k):
        raise NotImplementedError("addPairwiseEnergy (arbitrary features) is not supported by the pnp_ovss shim")

    def setUnary(self, *a, **k):
        raise NotImplementedError("setUnary (a Unary object) is not supported by the pnp_ovss shim: use setUnaryEnergy")

    def startInference(self, *a, **k):
        raise NotImplementedError("startInference is not supported by the pnp_ovss shim: use inference(n)")

    def stepInference(self, *a, **k):
        raise NotImplementedError("stepInference is not supported by the pnp_ovss shim: use inference(n)")

    def klDivergence(self, *a, **k):
        raise NotImplementedError("klDivergence is not supported by the pnp_ovss shim")

    def map(self, *a, **k):
        raise NotImplementedError("map is not supported by the pnp_ovss shim: use np.argmax(inference(n), axis=0)")


class DenseCRF:
    def __init__(self, *a, **k):
        raise NotImplementedError("DenseCRF (arbitrary pairwise features) is not supported by the pnp_ovss shim: use DenseCRF2D")
