"""CPU: the host side of the stand-alone DenseCRF -- the batch layout (pnp_ovss.crf.plan_batch), the pydensecrf import shim's
argument handling (pnp-ovss_amd/shims/pydensecrf) and the argument checks of the pnp_crf_* C ABI that sit in front of any HIP
call.  The device side is tests/test_crf_op_gpu.py."""
import ctypes
import importlib
import importlib.util
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIMS = os.path.join(ROOT, "pnp-ovss_amd", "shims")
LIB = os.path.join(ROOT, "pnp-ovss_amd", "pnp_ovss", "libpnp_hip.so")

PNP_ERR_ARG, PNP_ERR_STATE = -22, -1


@pytest.fixture()
def shim(monkeypatch):
    """(pydensecrf.densecrf, pydensecrf.utils) of the shim, imported for this test only."""
    monkeypatch.syspath_prepend(SHIMS)
    for m in [m for m in sys.modules if m == "pydensecrf" or m.startswith("pydensecrf.")]:
        monkeypatch.delitem(sys.modules, m)
    importlib.invalidate_caches()
    dcrf = importlib.import_module("pydensecrf.densecrf")
    utils = importlib.import_module("pydensecrf.utils")
    assert sys.modules["pydensecrf"].__pnp_ovss_shim__ is True
    yield dcrf, utils
    for m in [m for m in sys.modules if m == "pydensecrf" or m.startswith("pydensecrf.")]:
        monkeypatch.delitem(sys.modules, m, raising=False)


def test_plan_batch_offsets_by_hand():
    from pnp_ovss import crf
    p = crf.plan_batch([(37, 53), (45, 61), (29, 41)], [3, 21, 33])
    n = [37 * 53, 45 * 61, 29 * 41]                       # 1961, 2745, 1189
    assert n == [1961, 2745, 1189]
    assert p["Kp"] == [4, 24, 36]
    assert p["pix0"] == [0, 1961, 1961 + 2745]
    assert p["off"] == [0, 3 * 1961, 3 * 1961 + 21 * 2745] == [0, 5883, 63528]
    assert p["qoff"] == [0, 4 * 1961, 4 * 1961 + 24 * 2745] == [0, 7844, 73724]
    assert p["voff"] == [(0, 0), (3 * 1961 * 4, 6 * 1961 * 4), (3 * 1961 * 4 + 3 * 2745 * 24, 6 * 1961 * 4 + 6 * 2745 * 24)]
    assert p["voff"][2] == (221172, 442344)
    assert (p["max_batch"], p["max_total_pixels"], p["max_pixels_per_image"], p["max_labels"]) == (3, 5895, 2745, 33)
    assert p["total_unary"] == 63528 + 33 * 1189


def test_plan_batch_refuses_what_the_solver_cannot_hold():
    from pnp_ovss import crf
    with pytest.raises(ValueError, match="labels"):
        crf.plan_batch([(4, 4)], [1])
    with pytest.raises(ValueError, match="labels"):
        crf.plan_batch([(4, 4)], [256])
    with pytest.raises(ValueError, match="at most 64"):
        crf.plan_batch([(4, 4)] * 65, [2] * 65)
    with pytest.raises(ValueError):
        crf.plan_batch([(4, 4), (4, 4)], [2])
    with pytest.raises(ValueError, match="size"):
        crf.plan_batch([(0, 4)], [2])


def test_unary_from_softmax_matches_the_numpy_formula(shim):
    _, utils = shim
    rng = np.random.default_rng(0)
    x = rng.normal(0, 3, (5, 7, 9)).astype(np.float32)
    e = np.exp(x - x.max(0))
    p = (e / e.sum(0)).astype(np.float32)
    p[0, 0, 0] = 0.0                                        # clipped to 1e-5, not -log(0) = inf
    u = utils.unary_from_softmax(p)
    ref = -np.log(np.clip(p, 1e-5, 1.0)).astype(np.float32)   # tests/test_oracle_golden.py:388
    assert u.dtype == np.float32 and u.shape == (5, 63)
    assert np.array_equal(u, ref.reshape(5, -1))
    assert np.isfinite(u).all()
    s = 0.7
    us = utils.unary_from_softmax(p, scale=s)
    mixed = np.clip(s * p + (1 - s) * (np.ones(p.shape) / 5), 1e-5, 1.0)
    assert us.dtype == np.float32 and np.array_equal(us, (-np.log(mixed)).reshape(5, -1).astype(np.float32))
    un = utils.unary_from_softmax(p[:, 1:], clip=None)
    assert np.array_equal(un, (-np.log(p[:, 1:])).reshape(5, -1).astype(np.float32))
    with pytest.raises(ValueError):
        utils.unary_from_softmax(p, scale=0.0)


def test_shim_constants(shim):
    dcrf, _ = shim
    assert (dcrf.CONST_KERNEL, dcrf.DIAG_KERNEL, dcrf.FULL_KERNEL) == (0, 1, 2)
    assert (dcrf.NO_NORMALIZATION, dcrf.NORMALIZE_BEFORE, dcrf.NORMALIZE_AFTER, dcrf.NORMALIZE_SYMMETRIC) == (0, 1, 2, 3)


def test_shim_checks_shapes(shim):
    dcrf, _ = shim
    w, h, c = 6, 5, 3
    d = dcrf.DenseCRF2D(w, h, c)
    U = np.zeros((c, h * w), np.float32)
    d.setUnaryEnergy(U)
    for bad in (np.zeros((c, h, w), np.float32), np.zeros((c + 1, h * w), np.float32), np.zeros((h * w, c), np.float32)):
        with pytest.raises(ValueError, match="shape"):
            d.setUnaryEnergy(bad)
    with pytest.raises(ValueError, match="float32"):
        d.setUnaryEnergy(U.astype(np.float64))
    with pytest.raises(ValueError, match="contiguous"):
        d.setUnaryEnergy(np.zeros((h * w, c), np.float32).T)
    with pytest.raises(ValueError, match="rgbim"):
        d.addPairwiseBilateral(sxy=50, srgb=5, rgbim=np.zeros((w, h, 3), np.uint8), compat=10)      # (w, h) swapped
    with pytest.raises(ValueError, match="rgbim"):
        d.addPairwiseBilateral(sxy=50, srgb=5, rgbim=np.zeros((h, w, 3), np.float32), compat=10)
    with pytest.raises(ValueError, match="setUnaryEnergy"):
        dcrf.DenseCRF2D(w, h, c).inference(1)
    with pytest.raises(ValueError):
        dcrf.DenseCRF2D(w, h, 1)


def test_shim_refuses_what_it_does_not_compute(shim):
    dcrf, utils = shim
    w, h, c = 6, 5, 3
    img = np.zeros((h, w, 3), np.uint8)

    def fresh():
        return dcrf.DenseCRF2D(w, h, c)
    # matrix / vector compatibility
    with pytest.raises(NotImplementedError, match="compat"):
        fresh().addPairwiseGaussian(sxy=3, compat=np.eye(c, dtype=np.float32))
    with pytest.raises(NotImplementedError, match="compat"):
        fresh().addPairwiseBilateral(sxy=50, srgb=5, rgbim=img, compat=np.ones(c, np.float32))
    # anisotropic widths
    with pytest.raises(NotImplementedError, match="sxy"):
        fresh().addPairwiseGaussian(sxy=(3, 4), compat=7)
    with pytest.raises(NotImplementedError, match="sxy"):
        fresh().addPairwiseBilateral(sxy=(50, 40), srgb=5, rgbim=img, compat=10)
    with pytest.raises(NotImplementedError, match="srgb"):
        fresh().addPairwiseBilateral(sxy=50, srgb=(5, 5, 6), rgbim=img, compat=10)
    # other kernels / normalisations
    for norm in (dcrf.NO_NORMALIZATION, dcrf.NORMALIZE_BEFORE, dcrf.NORMALIZE_AFTER):
        with pytest.raises(NotImplementedError, match="NORMALIZ"):
            fresh().addPairwiseGaussian(sxy=3, compat=7, normalization=norm)
        with pytest.raises(NotImplementedError, match="NORMALIZ"):
            fresh().addPairwiseBilateral(sxy=50, srgb=5, rgbim=img, compat=10, normalization=norm)
    for kern in (dcrf.CONST_KERNEL, dcrf.FULL_KERNEL):
        with pytest.raises(NotImplementedError, match="_KERNEL"):
            fresh().addPairwiseGaussian(sxy=3, compat=7, kernel=kern)
    # a second term of a kind
    d = fresh()
    d.addPairwiseGaussian(sxy=(3, 3), compat=7)                     # equal values: isotropic, accepted
    d.addPairwiseBilateral(sxy=(50, 50), srgb=(5, 5, 5), rgbim=img, compat=10.0)
    with pytest.raises(NotImplementedError, match="second Gaussian"):
        d.addPairwiseGaussian(sxy=3, compat=7)
    with pytest.raises(NotImplementedError, match="second bilateral"):
        d.addPairwiseBilateral(sxy=50, srgb=5, rgbim=img, compat=10)
    # the rest of the interface
    with pytest.raises(NotImplementedError, match="DenseCRF "):
        dcrf.DenseCRF(h * w, c)
    for name in ("addPairwiseEnergy", "startInference", "stepInference", "klDivergence"):
        with pytest.raises(NotImplementedError, match=name):
            getattr(d, name)()
    for name in ("unary_from_labels", "create_pairwise_gaussian", "create_pairwise_bilateral"):
        with pytest.raises(NotImplementedError, match=name):
            getattr(utils, name)()


def test_no_device_means_an_error_not_a_fallback(shim):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from pnp_ovss import crf
    dcrf, _ = shim
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        crf.DenseCRF(1, 16, 16, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        crf.densecrf(np.zeros((3, 4, 4), np.float32), np.zeros((4, 4, 3), np.uint8))
    d = dcrf.DenseCRF2D(4, 4, 3)
    d.setUnaryEnergy(np.zeros((3, 16), np.float32))
    d.addPairwiseGaussian(sxy=3, compat=7)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        d.inference(2)


def test_cabi_argument_checks_need_no_gpu():
    if not os.path.exists(LIB):
        import subprocess
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "pnp-ovss_amd", "csrc"), "-j8"])
    lib = ctypes.CDLL(LIB)
    lib.pnp_crf_last_error.restype = ctypes.c_char_p
    lib.pnp_crf_last_error.argtypes = [ctypes.c_void_p]
    lib.pnp_crf_allocated_bytes.restype = ctypes.c_size_t
    lib.pnp_crf_allocated_bytes.argtypes = [ctypes.c_void_p]
    lib.pnp_crf_create.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32,
                                   ctypes.POINTER(ctypes.c_void_p)]
    lib.pnp_crf_set_batch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_void_p]
    lib.pnp_crf_infer.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_float, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p,
                                  ctypes.c_void_p]
    assert lib.pnp_crf_last_error(None) == b"null solver"
    assert lib.pnp_crf_allocated_bytes(None) == 0
    assert lib.pnp_crf_set_batch(None, None, 3.0, 50.0, 5.0, None) == PNP_ERR_ARG
    assert lib.pnp_crf_infer(None, 10, 7.0, 10.0, None, None, None) == PNP_ERR_ARG
    lib.pnp_crf_destroy(None)                                        # a no-op
    # bad bounds are refused before the device is touched, and no handle is handed out
    h = ctypes.c_void_p()
    assert lib.pnp_crf_create(0, 1, 16, 16, 3, None) == PNP_ERR_ARG
    for bounds in ((0, 16, 16, 3), (65, 16, 16, 3), (1, 0, 16, 3), (1, 16, 0, 3), (1, 16, 32, 3), (1, 16, 16, 1), (1, 16, 16, 256)):
        h.value = 1
        assert lib.pnp_crf_create(0, *bounds, ctypes.byref(h)) == PNP_ERR_ARG, bounds
        assert not h.value
    assert lib.pnp_crf_create(-1, 1, 16, 16, 3, ctypes.byref(h)) == PNP_ERR_ARG


def test_shim_is_found_only_after_opting_in(monkeypatch):
    """The session's sys.path (the repository root and pnp-ovss_amd, tests/conftest.py) must not resolve `pydensecrf` to the
    shim: tests/golden/make_crf_golden.py imports the real package with that path to pin the oracle."""
    for m in [m for m in sys.modules if m == "pydensecrf" or m.startswith("pydensecrf.")]:
        monkeypatch.delitem(sys.modules, m)
    importlib.invalidate_caches()
    spec = importlib.util.find_spec("pydensecrf")
    if spec is not None:                                             # a real pydensecrf is installed: it is not ours
        assert not os.path.abspath(spec.origin or "").startswith(os.path.join(ROOT, ""))
    assert not os.path.exists(os.path.join(ROOT, "pnp-ovss_amd", "pydensecrf"))
    monkeypatch.syspath_prepend(SHIMS)
    importlib.invalidate_caches()
    spec = importlib.util.find_spec("pydensecrf")
    assert spec is not None and os.path.abspath(spec.origin) == os.path.join(SHIMS, "pydensecrf", "__init__.py")
