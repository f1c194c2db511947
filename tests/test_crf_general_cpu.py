"""CPU: the general stand-alone DenseCRF (per-axis widths, compatibility matrices, stepwise inference) -- its reference
(tests/_crf_general_ref.py) against the oracle where the oracle reaches (scalar weights, equal widths) and against its own
float64 brute force where it does not, and the host-side argument handling of pnp_ovss.crf, the pydensecrf shim and the C ABI.
The device side is tests/test_crf_general_gpu.py."""
import ctypes
import importlib
import importlib.util
import os
import sys

import numpy as np
import pytest

import _crf_general_ref as G
import _post_refs as R
import test_crf_op_gpu as T
from oracle import pipeline_np as OP
from oracle.densecrf_exact import densecrf_exact

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIMS = os.path.join(ROOT, "pnp-ovss_amd", "shims")
LIB = os.path.join(ROOT, "pnp-ovss_amd", "pnp_ovss", "libpnp_hip.so")
PNP_ERR_ARG = -22


GENERAL = os.path.join(SHIMS, "general")                     # the general shim: a package of its own, opted into by this path


@pytest.fixture()
def shim(monkeypatch):
    """pydensecrf.densecrf of the general shim, imported for this test only."""
    monkeypatch.syspath_prepend(GENERAL)
    for m in [m for m in sys.modules if m == "pydensecrf" or m.startswith("pydensecrf.")]:
        monkeypatch.delitem(sys.modules, m)
    importlib.invalidate_caches()
    dcrf = importlib.import_module("pydensecrf.densecrf")
    assert sys.modules["pydensecrf"].__pnp_ovss_shim__ is True and sys.modules["pydensecrf"].__pnp_ovss_shim_general__ is True
    yield dcrf
    for m in [m for m in sys.modules if m == "pydensecrf" or m.startswith("pydensecrf.")]:
        monkeypatch.delitem(sys.modules, m, raising=False)


@pytest.mark.parametrize("shape", [(3, 37, 53), (21, 45, 61)], ids=["K3", "K21"])
@pytest.mark.parametrize("pi", [0, 1, 2])
def test_reference_matches_the_oracle_where_the_oracle_reaches(shape, pi):
    """Scalar weights and equal widths: the numpy restatement against oracle/densecrf_ref.c, marginals within Q_ATOL and labels
    equal away from the oracle's near-ties (the rule of tests/test_crf_op_gpu.py, asserted on the oracle first)."""
    K, H, W = shape
    rgb, U = T.inputs(K, H, W)
    ref_lab, ref_q = T.oracle(shape, pi)
    p = dict(OP.CRF_PARAMS)
    p.update(T.PARAMS[pi])
    q = G.MeanField(rgb, U, p["pos_xy"], p["bi_xy"], p["bi_rgb"]).run(p["iters"], p["pos_w"], p["bi_w"])
    T.check_against_oracle(G.labels_of(q), q, ref_lab, ref_q, f"reference {shape} {T.PARAMS[pi]}")


def test_reference_matches_its_brute_force_as_well_as_the_oracle_matches_its_own():
    """One anisotropic case with full, non-symmetric matrices on a 24 x 24 image: the lattice reference against the float64
    brute force of every kernel entry.  The lattice approximates the kernels, so this is a sanity bound: the new case may be at
    most 1.5 x as far from its brute force as the isotropic Potts oracle is from oracle/densecrf_exact.py on the same image,
    in max |dQ| and in the share of differing labels."""
    K, H, W = 5, 24, 24
    rgb = R.photo_like(H, W, seed=3)
    maps = np.log(np.array(T.softmax_input(K, H, W)))                    # softmax(maps) = the probabilities
    _, base_q, _ = OP.densecrf(rgb, maps.astype(np.float32), want_q=True)
    ex_lab, ex_q = densecrf_exact(rgb, maps)
    base_dq = float(np.abs(base_q - ex_q).max())
    base_dl = float((base_q.argmax(0) != ex_lab).mean())
    U = np.ascontiguousarray(OP.crf_unary(maps.astype(np.float32)).reshape(K, -1))
    rng = np.random.default_rng(11)
    Mg = (np.diag(np.full(K, 7.0)) + rng.uniform(-2.1, 0, (K, K)) * (1 - np.eye(K))).astype(np.float32)
    Mb = (np.diag(np.full(K, 10.0)) + rng.uniform(-3.0, 0, (K, K)) * (1 - np.eye(K))).astype(np.float32)
    widths = dict(pos_xy=(2.0, 4.0), bi_xy=(40.0, 70.0), bi_rgb=(4.0, 6.0, 9.0))
    q = G.MeanField(rgb, U, **widths).run(10, Mg, Mb)
    bf = G.brute_force(rgb, U, 10, widths["pos_xy"], widths["bi_xy"], widths["bi_rgb"], Mg, Mb)
    new_dq = float(np.abs(q - bf).max())
    new_dl = float((q.argmax(0) != bf.argmax(0)).mean())
    print(f"isotropic Potts, oracle vs exact: max |dQ| {base_dq:.4f}, labels differing {100 * base_dl:.2f} %")
    print(f"anisotropic matrices, reference vs brute force: max |dQ| {new_dq:.4f}, labels differing {100 * new_dl:.2f} %")
    assert new_dq <= 1.5 * base_dq
    assert new_dl <= 1.5 * base_dl


def test_widths_and_batch_plans_take_tuples():
    from pnp_ovss import crf
    assert crf._widths(3, 2, "pos_xy") == [3.0, 3.0]
    assert crf._widths((2, 4), 2, "pos_xy") == [2.0, 4.0]
    assert crf._widths(np.float32(5), 3, "bi_rgb") == [5.0, 5.0, 5.0]
    assert crf._widths([4, 6, 9], 3, "bi_rgb") == [4.0, 6.0, 9.0]
    for bad in ((2, 4, 6), ()):
        with pytest.raises(ValueError, match="pos_xy"):
            crf._widths(bad, 2, "pos_xy")
    for bad in (0, -1.0, (3, 0), float("nan")):
        with pytest.raises(ValueError, match="positive"):
            crf._widths(bad, 2, "pos_xy")
    p = crf.plan_batch(((37, 53), (45, 61)), (21, 21))                   # tuples as well as lists
    assert p["Kp"] == [24, 24] and p["pix0"] == [0, 37 * 53]


def test_compat_arguments():
    from pnp_ovss import crf
    assert crf.compat_values(None, "pos_compat") == (crf.COMPAT_SCALAR, None, 0)
    kind, vals, k = crf.compat_values(np.arange(4, dtype=np.float32), "pos_compat")
    assert (kind, k) == (crf.COMPAT_DIAGONAL, 4) and vals.dtype == np.float32
    m = np.arange(9, dtype=np.float32).reshape(3, 3)
    kind, vals, k = crf.compat_values(m.T, "bi_compat")                  # a non-contiguous view is copied row-major
    assert (kind, k) == (crf.COMPAT_MATRIX, 3) and vals.flags["C_CONTIGUOUS"] and np.array_equal(vals, m.T)
    for bad in (np.zeros((3, 4), np.float32), np.zeros((2, 2, 2), np.float32), np.zeros(1, np.float32), np.zeros((256, 256), np.float32)):
        with pytest.raises(ValueError, match="bi_compat"):
            crf.compat_values(bad, "bi_compat")
    with pytest.raises(ValueError, match="float32"):
        crf.compat_values(np.eye(3), "pos_compat")
    # a vector or matrix fixes the label count of the batch
    crf.check_compat_labels(21, [21, 21, 21], "bi_compat")
    crf.check_compat_labels(0, [3, 21], "bi_compat")                     # scalar terms take any mix
    with pytest.raises(ValueError, match="every image"):
        crf.check_compat_labels(21, [21, 3], "bi_compat")


def test_shim_converts_compat_to_message_weights(shim):
    K = 4
    assert shim.message_weights(7, K, "t") == (7.0, None)
    assert shim.message_weights(np.float32(2.5), K, "t") == (2.5, None)
    v = np.array([1, 2, 3, 4], np.float32)
    w, M = shim.message_weights(v, K, "t")
    assert w is None and M.dtype == np.float32 and np.array_equal(M, np.diag(-v))
    m = np.arange(16, dtype=np.float32).reshape(K, K)
    w, M = shim.message_weights(m, K, "t")
    assert w is None and M.dtype == np.float32 and np.array_equal(M, -0.5 * (m + m.T)) and np.array_equal(M, M.T)
    assert np.array_equal(shim.message_weights(m.astype(np.int64), K, "t")[1], M)
    for bad in (np.zeros(K + 1, np.float32), np.zeros((K, K + 1), np.float32), np.zeros((K, K, 1), np.float32)):
        with pytest.raises(ValueError, match="compat"):
            shim.message_weights(bad, K, "t")
    d = shim.DenseCRF2D(6, 5, K)
    d.addPairwiseGaussian(sxy=(3, 4), compat=v)
    assert d._gauss[0] == (3.0, 4.0) and d._gauss[1] is None and np.array_equal(d._gauss[2], np.diag(-v))
    d.addPairwiseBilateral(sxy=(50, 40), srgb=(5, 5, 6), rgbim=np.zeros((5, 6, 3), np.uint8), compat=m)
    assert d._bilat[:2] == ((50.0, 40.0), (5.0, 5.0, 6.0)) and np.array_equal(d._bilat[4], M)
    for bad in (0, (3, -1), (1, 2, 3)):
        with pytest.raises(ValueError, match="sxy"):
            shim.DenseCRF2D(6, 5, K).addPairwiseGaussian(sxy=bad, compat=7)
    with pytest.raises(ValueError, match="srgb"):
        shim.DenseCRF2D(6, 5, K).addPairwiseBilateral(sxy=50, srgb=(5, 5), rgbim=np.zeros((5, 6, 3), np.uint8), compat=10)


def test_general_shim_is_a_package_of_its_own(shim, monkeypatch):
    """pnp-ovss_amd/shims/general serves the general form; pnp-ovss_amd/shims keeps the Potts-only shim and its refusals (what
    tests/test_crf_op_cpu.py holds it to); both hand out the one utils module."""
    import pydensecrf
    import pydensecrf.utils as utils
    assert os.path.abspath(pydensecrf.__file__) == os.path.join(GENERAL, "pydensecrf", "__init__.py")
    p = np.full((3, 2, 2), 1 / 3, np.float32)
    assert np.array_equal(utils.unary_from_softmax(p), -np.log(p).reshape(3, -1))
    with pytest.raises(NotImplementedError, match="create_pairwise_bilateral"):
        utils.create_pairwise_bilateral()
    # what the general shim still refuses, and approximates nothing of
    img = np.zeros((5, 6, 3), np.uint8)
    d = shim.DenseCRF2D(6, 5, 3)
    d.addPairwiseGaussian(sxy=3, compat=7)
    d.addPairwiseBilateral(sxy=50, srgb=5, rgbim=img, compat=10)
    with pytest.raises(NotImplementedError, match="second Gaussian"):
        d.addPairwiseGaussian(sxy=3, compat=7)
    with pytest.raises(NotImplementedError, match="second bilateral"):
        d.addPairwiseBilateral(sxy=50, srgb=5, rgbim=img, compat=10)
    for name in ("addPairwiseEnergy", "setUnary"):
        with pytest.raises(NotImplementedError, match=name):
            getattr(d, name)()
    with pytest.raises(NotImplementedError, match="DenseCRF "):
        shim.DenseCRF(30, 3)
    for kern in (shim.CONST_KERNEL, shim.FULL_KERNEL):
        with pytest.raises(NotImplementedError, match="_KERNEL"):
            shim.DenseCRF2D(6, 5, 3).addPairwiseGaussian(sxy=3, compat=7, kernel=kern)
    for norm in (shim.NO_NORMALIZATION, shim.NORMALIZE_BEFORE, shim.NORMALIZE_AFTER):
        with pytest.raises(NotImplementedError, match="NORMALIZ"):
            shim.DenseCRF2D(6, 5, 3).addPairwiseBilateral(sxy=50, srgb=5, rgbim=img, compat=10, normalization=norm)
    # the other path entry alone: the Potts-only shim, as before
    for m in [m for m in sys.modules if m == "pydensecrf" or m.startswith("pydensecrf.")]:
        monkeypatch.delitem(sys.modules, m)
    monkeypatch.setattr(sys, "path", [SHIMS] + [q for q in sys.path if os.path.abspath(q) != GENERAL])
    importlib.invalidate_caches()
    strict = importlib.import_module("pydensecrf.densecrf")
    assert sys.modules["pydensecrf"].__pnp_ovss_shim__ is True and not hasattr(sys.modules["pydensecrf"], "__pnp_ovss_shim_general__")
    with pytest.raises(NotImplementedError, match="compat"):
        strict.DenseCRF2D(6, 5, 3).addPairwiseGaussian(sxy=3, compat=np.eye(3, dtype=np.float32))


def test_shim_stepwise_calls_need_a_start(shim):
    d = shim.DenseCRF2D(6, 5, 3)
    for call in (d.stepInference, d.klDivergence):
        with pytest.raises(RuntimeError, match="startInference"):
            call()
    with pytest.raises(ValueError, match="setUnaryEnergy"):
        d.startInference()
    with pytest.raises(ValueError, match="setUnaryEnergy"):
        d.map(1)


def test_new_entry_points_refuse_a_null_solver_without_a_device():
    """What the C ABI lets a machine without a device check: every new entry point returns PNP_ERR_ARG for a null solver (a
    solver cannot be created without a device, so PNP_ERR_STATE before start is checked on the GPU)."""
    if not os.path.exists(LIB):
        import subprocess
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "pnp-ovss_amd", "csrc"), "-j8"])
    lib = ctypes.CDLL(LIB)
    vp, f32, i32 = ctypes.c_void_p, ctypes.c_float, ctypes.c_int32
    lib.pnp_crf_set_batch_aniso.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.pnp_crf_set_compat.argtypes = [vp, i32, i32, vp, i32]
    lib.pnp_crf_start.argtypes = [vp, vp]
    lib.pnp_crf_step.argtypes = [vp, i32, f32, f32, vp]
    lib.pnp_crf_read.argtypes = [vp, vp, vp, vp]
    lib.pnp_crf_kl.argtypes = [vp, f32, f32, vp, vp]
    out = (ctypes.c_double * 1)()
    assert lib.pnp_crf_set_batch_aniso(None, None, None, None, None, None) == PNP_ERR_ARG
    assert lib.pnp_crf_set_compat(None, 0, 2, None, 3) == PNP_ERR_ARG
    assert lib.pnp_crf_start(None, None) == PNP_ERR_ARG
    assert lib.pnp_crf_step(None, 1, 7.0, 10.0, None) == PNP_ERR_ARG
    assert lib.pnp_crf_read(None, None, None, None) == PNP_ERR_ARG
    assert lib.pnp_crf_kl(None, 7.0, 10.0, out, None) == PNP_ERR_ARG


def test_shim_stays_off_the_default_import_path(monkeypatch):
    for m in [m for m in sys.modules if m == "pydensecrf" or m.startswith("pydensecrf.")]:
        monkeypatch.delitem(sys.modules, m)
    importlib.invalidate_caches()
    import pnp_ovss.crf  # noqa: F401  (importing the solver's module does not bring the shim in)
    assert "pydensecrf" not in sys.modules
    spec = importlib.util.find_spec("pydensecrf")
    if spec is not None:
        assert not os.path.abspath(spec.origin or "").startswith(os.path.join(ROOT, ""))