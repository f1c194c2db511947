"""What the DenseCRF with caller-supplied feature terms (pnp_crf_set_batch_terms, pnp_ovss.crf.FeatureCRF) lets a machine without
a device check: the T-term restatement against the two-term one, a sanity bound against a float64 brute force, the layout
arithmetic, the argument checks of the Python layer, and the C ABI's refusals that come before any HIP call."""
import ctypes
import os

import numpy as np
import pytest

import _crf_general_ref as G
import _crf_terms_ref as TR
import _post_refs as R
import test_crf_op_gpu as T
from oracle import pipeline_np as OP
from oracle.densecrf_exact import densecrf_exact

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "pnp-ovss_amd", "pnp_ovss", "libpnp_hip.so")
PNP_ERR_ARG = -22


@pytest.mark.parametrize("shape", [(3, 37, 53), (21, 45, 61)], ids=["K3", "K21"])
def test_terms_restatement_equals_the_two_term_one(shape):
    """[xy / 3, xy / 50 . rgb / 5] with weights 7 / 10 through the T-term restatement: G.MeanField.run value for value."""
    K, H, W = shape
    rgb, U = T.inputs(K, H, W)
    two = G.MeanField(rgb, U).run(TR.ITERS, 7.0, 10.0)
    fg, fb = G.features(rgb, 3.0, 50.0, 5.0)
    q = TR.TermsMeanField(U, H, W, [fg.T.reshape(2, H, W), fb.T.reshape(5, H, W)]).run(TR.ITERS, (7.0, 10.0))
    assert np.array_equal(q, two)
    M = [np.diag(np.full(K, w)).astype(np.float32) for w in (7.0, 10.0)]            # and w I as a matrix, as there
    assert np.array_equal(G.MeanField(rgb, U).run(2, M[0], M[1]), TR.TermsMeanField(U, H, W, [fg.T.reshape(2, H, W), fb.T.reshape(5, H, W)]).run(2, M))


@pytest.fixture(scope="module")
def small():
    """The 5 x 24 x 24 image of test_crf_general_cpu: (rgb, depth, U (K, N), share of labels the isotropic oracle leaves
    different from its exact evaluation)."""
    K, H, W = 5, 24, 24
    rgb = R.photo_like(H, W, seed=3)
    maps = np.log(np.array(T.softmax_input(K, H, W)))
    _, base_q, _ = OP.densecrf(rgb, maps.astype(np.float32), want_q=True)
    ex_lab, _ = densecrf_exact(rgb, maps)
    base_dl = float((base_q.argmax(0) != ex_lab).mean())
    U = np.ascontiguousarray(OP.crf_unary(maps.astype(np.float32)).reshape(K, -1))
    return rgb, TR.depth_plane(K, H, W), U, base_dl


@pytest.mark.parametrize("names,weights", [(("d2", "d3", "d6"), (3, 4, 6)), (("d2", "d4"), (7, 10)), (("d3",), (8,))],
                         ids=["d2-d3-d6", "d2-d4", "d3"])
def test_reference_is_as_close_to_its_brute_force_as_the_oracle_to_its_own(small, names, weights):
    """The lattice approximates the kernels, so this is a sanity bound: ten iterations of the T-term reference may leave at most
    1.5 x the share of labels different from the float64 brute force of every kernel entry that the isotropic two-term oracle
    leaves on the same image (6.25 %)."""
    rgb, depth, U, base_dl = small
    K, (H, W) = U.shape[0], rgb.shape[:2]
    feats = [TR.feature_set(n, rgb, depth) for n in names]
    q = TR.TermsMeanField(U, H, W, feats).run(10, weights)
    bf = TR.brute_force(U, feats, weights, 10).reshape(K, H, W)
    dl = float((q.argmax(0) != bf.argmax(0)).mean())
    print(f"{names}: labels differing from the brute force {100 * dl:.2f} %; isotropic oracle vs exact {100 * base_dl:.2f} %")
    assert abs(base_dl - 0.0625) < 1e-9
    assert dl <= 1.5 * base_dl


def test_plan_terms_against_hand_arithmetic():
    from pnp_ovss import crf
    p = crf.plan_terms([(13, 17), (19, 23)], [3, 5], [2, 6])
    n0, n1 = 13 * 17, 19 * 23
    assert p["Kp"] == [4, 8] and p["pix0"] == [0, n0] and p["off"] == [0, 3 * n0] and p["qoff"] == [0, 4 * n0]
    assert p["tvoff"] == [[0, 3 * n0 * 4], [0, 7 * n0 * 4]]
    assert p["foff"] == [[0, 2 * n0], [0, 6 * n0]]
    assert p["total_features"] == [2 * (n0 + n1), 6 * (n0 + n1)]
    assert p["value_floats"] == 7 * (n0 * 4 + n1 * 8)
    assert (p["max_terms"], p["max_dims"], p["max_batch"], p["max_total_pixels"], p["max_labels"]) == (2, 6, 2, n0 + n1, 5)
    for bad in ([], [1] * 9, [0], [7]):
        with pytest.raises(ValueError, match="term"):
            crf.plan_terms([(13, 17)], [3], bad)


def test_term_and_feature_helper_arguments():
    from pnp_ovss import crf
    f = np.zeros((3, 5, 6), np.float32)
    t = crf.Term([f], 4)
    assert (t.dims, t.weight, t.kind, t.K) == (3, 4.0, crf.COMPAT_SCALAR, 0)
    t = crf.Term([f.reshape(3, -1)], np.arange(4, dtype=np.float32))
    assert (t.kind, t.K) == (crf.COMPAT_DIAGONAL, 4)
    assert crf.Term([f], np.eye(4, dtype=np.float32)).kind == crf.COMPAT_MATRIX
    with pytest.raises(ValueError, match="float32"):
        crf.Term([f.astype(np.float64)], 1)
    with pytest.raises(ValueError, match="feature axes"):
        crf.Term([np.zeros((7, 5, 6), np.float32)], 1)
    with pytest.raises(ValueError, match="feature axes"):
        crf.Term([f, np.zeros((2, 5, 6), np.float32)], 1)
    with pytest.raises(ValueError, match="at least one image"):
        crf.Term([], 1)
    with pytest.raises(ValueError, match="compat"):
        crf.Term([f], np.zeros((3, 4), np.float32))
    with pytest.raises(ValueError, match="float32"):
        crf.Term([f], np.eye(3))
    # the helpers: float32 quotients of float32 operands, x before y, channels after
    pos = crf.position_features([(5, 6)], (3, 4))[0]
    assert pos.shape == (2, 5, 6) and pos.dtype == np.float32
    assert pos[0, 2, 5] == np.float32(5) / np.float32(3) and pos[1, 2, 5] == np.float32(2) / np.float32(4)
    rgb = R.photo_like(5, 6, seed=1)
    fg, fb = G.features(rgb, 3.0, 50.0, 5.0)
    assert np.array_equal(crf.position_features([(5, 6)], 3)[0].reshape(2, -1).T, fg)
    assert np.array_equal(crf.image_features([rgb], 50, 5)[0].reshape(5, -1).T, fb)
    grey = crf.image_features([rgb[:, :, 0].astype(np.float64)], 50, 8)[0]
    assert grey.shape == (3, 5, 6) and grey[2, 1, 2] == np.float32(rgb[1, 2, 0]) / np.float32(8)
    with pytest.raises(ValueError, match="feature axes"):
        crf.image_features([np.zeros((5, 6, 5))], 50, 5)
    with pytest.raises(ValueError, match="schan"):
        crf.image_features([rgb], 50, (5, 5))


def test_feature_solver_bounds_need_no_device(monkeypatch):
    from pnp_ovss import crf
    for bad in (dict(max_terms=0), dict(max_terms=9), dict(max_dims=0), dict(max_dims=7)):
        with pytest.raises(ValueError, match="terms"):
            crf.FeatureCRF(1, 100, 100, 3, **bad)


def test_new_entry_points_refuse_bad_arguments_without_a_device():
    """Every new entry point returns PNP_ERR_ARG before any HIP call for a null solver (whatever else it is given: a null term
    array, 0 or 9 terms, 0 or 7 feature axes), and pnp_crf_create_terms for counts out of range or a null result pointer."""
    if not os.path.exists(LIB):
        import subprocess
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "pnp-ovss_amd", "csrc"), "-j8"])
    lib = ctypes.CDLL(LIB)
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64

    class Term(ctypes.Structure):
        _fields_ = [("dims", i32), ("d_features", vp)]
    lib.pnp_crf_create_terms.argtypes = [i32, i32, i64, i32, i32, i32, i32, vp]
    lib.pnp_crf_set_batch_terms.argtypes = [vp, vp, i32, vp, vp]
    lib.pnp_crf_set_term_compat.argtypes = [vp, i32, i32, vp, i32]
    lib.pnp_crf_infer_terms.argtypes = [vp, i32, vp, vp, vp, vp]
    lib.pnp_crf_step_terms.argtypes = [vp, i32, vp, vp]
    out = vp()
    for terms, dims in ((0, 6), (9, 6), (4, 0), (4, 7)):
        assert lib.pnp_crf_create_terms(0, 1, 100, 100, 3, terms, dims, ctypes.byref(out)) == PNP_ERR_ARG
        assert not out
    assert lib.pnp_crf_create_terms(0, 1, 100, 100, 3, 4, 6, None) == PNP_ERR_ARG
    assert lib.pnp_crf_create_terms(0, 65, 100, 100, 3, 4, 6, ctypes.byref(out)) == PNP_ERR_ARG and not out
    for dims in (0, 3, 7):
        arr = (Term * 9)(*[Term(dims, None) for _ in range(9)])
        for n in (0, 1, 9):
            assert lib.pnp_crf_set_batch_terms(None, None, n, arr, None) == PNP_ERR_ARG
    assert lib.pnp_crf_set_batch_terms(None, None, 1, None, None) == PNP_ERR_ARG
    assert lib.pnp_crf_set_term_compat(None, 0, 2, None, 3) == PNP_ERR_ARG
    w = (ctypes.c_float * 8)(*([1.0] * 8))
    assert lib.pnp_crf_infer_terms(None, 1, w, None, None, None) == PNP_ERR_ARG
    assert lib.pnp_crf_infer_terms(None, 1, None, None, None, None) == PNP_ERR_ARG
    assert lib.pnp_crf_step_terms(None, 1, w, None) == PNP_ERR_ARG
    assert lib.pnp_crf_step_terms(None, 1, None, None) == PNP_ERR_ARG


SHIMS = os.path.join(ROOT, "pnp-ovss_amd", "shims")
ND = os.path.join(SHIMS, "nd")


def _fresh_pydensecrf(monkeypatch, first):
    import importlib
    import sys
    for m in [m for m in sys.modules if m == "pydensecrf" or m.startswith("pydensecrf.")]:
        monkeypatch.delitem(sys.modules, m)
    others = {os.path.abspath(p) for p in (SHIMS, os.path.join(SHIMS, "general"), ND)}
    monkeypatch.setattr(sys, "path", [first, os.path.join(ROOT, "pnp-ovss_amd")] + [p for p in sys.path if os.path.abspath(p) not in others])
    importlib.invalidate_caches()
    return importlib.import_module("pydensecrf.densecrf"), importlib.import_module("pydensecrf.utils")


def test_nd_shim_is_a_package_of_its_own(monkeypatch):
    import importlib.util
    import sys
    for m in [m for m in sys.modules if m == "pydensecrf" or m.startswith("pydensecrf.")]:
        monkeypatch.delitem(sys.modules, m)
    spec = importlib.util.find_spec("pydensecrf")                             # off the default import path
    assert spec is None or not os.path.abspath(spec.origin or "").startswith(os.path.join(ROOT, ""))
    img = np.zeros((5, 6, 3), np.uint8)
    # the two other shims refuse exactly as before
    for first, second in ((SHIMS, "compat"), (os.path.join(SHIMS, "general"), "second Gaussian")):
        dcrf, utils = _fresh_pydensecrf(monkeypatch, first)
        assert not hasattr(sys.modules["pydensecrf"], "__pnp_ovss_shim_nd__")
        d = dcrf.DenseCRF2D(6, 5, 3)
        with pytest.raises(NotImplementedError, match="addPairwiseEnergy"):
            d.addPairwiseEnergy()
        d.addPairwiseGaussian(sxy=3, compat=7)
        with pytest.raises(NotImplementedError, match="second Gaussian"):
            d.addPairwiseGaussian(sxy=3, compat=7)
        with pytest.raises(NotImplementedError, match="create_pairwise_bilateral"):
            utils.create_pairwise_bilateral()
        with pytest.raises(NotImplementedError, match="DenseCRF "):
            dcrf.DenseCRF(30, 3)
    # the N-D shim: any number of terms, features as pydensecrf's utils lay them out (axes in the order of `shape`)
    dcrf, utils = _fresh_pydensecrf(monkeypatch, ND)
    assert sys.modules["pydensecrf"].__pnp_ovss_shim_nd__ is True
    g = utils.create_pairwise_gaussian((3, 4), (5, 6))
    assert g.shape == (2, 30) and g.dtype == np.float32
    assert g[0, 7] == np.float32(1) / np.float32(3) and g[1, 7] == np.float32(1) / np.float32(4)
    b = utils.create_pairwise_bilateral((50, 40), (5, 6, 7), np.full((5, 6, 3), 14, np.uint8), chdim=2)
    assert b.shape == (5, 30) and np.array_equal(b[:, 7], np.array([1 / 50, 1 / 40, 14 / 5, 14 / 6, 2.0], np.float32))
    assert utils.create_pairwise_bilateral((50, 40), 0.5, np.ones((5, 6)), chdim=-1).shape == (3, 30)
    p = np.full((3, 2, 2), 1 / 3, np.float32)
    assert np.array_equal(utils.unary_from_softmax(p), -np.log(p).reshape(3, -1))
    d = dcrf.DenseCRF2D(6, 5, 3)
    d.addPairwiseGaussian(sxy=3, compat=7)
    d.addPairwiseGaussian(sxy=(3, 4), compat=np.ones(3, np.float32))
    d.addPairwiseBilateral(sxy=50, srgb=5, rgbim=img, compat=10)
    d.addPairwiseBilateral(sxy=20, srgb=(5, 5, 6), rgbim=img, compat=np.eye(3))
    d.addPairwiseEnergy(g, 4)
    assert len(d._terms) == 5 and d._terms[1][1] is None and np.array_equal(d._terms[1][2], -np.eye(3, dtype=np.float32))
    with pytest.raises(NotImplementedError, match="klDivergence"):
        d.klDivergence()
    with pytest.raises(NotImplementedError, match="_KERNEL"):
        d.addPairwiseEnergy(g, 4, kernel=dcrf.FULL_KERNEL)
    with pytest.raises(NotImplementedError, match="NORMALIZ"):
        d.addPairwiseEnergy(g, 4, normalization=dcrf.NORMALIZE_BEFORE)
    with pytest.raises(ValueError, match="float32"):
        d.addPairwiseEnergy(g.astype(np.float64), 4)
    with pytest.raises(NotImplementedError, match="1..6"):
        dcrf.DenseCRF(30, 3).addPairwiseEnergy(np.zeros((7, 30), np.float32), 4)
    with pytest.raises(RuntimeError, match="startInference"):
        d.stepInference()


def test_compat_conversion_lives_in_one_place(monkeypatch):
    from pnp_ovss import crf
    dcrf, _ = _fresh_pydensecrf(monkeypatch, os.path.join(SHIMS, "general"))
    m = np.arange(16, dtype=np.float32).reshape(4, 4)
    assert dcrf.message_weights(7, 4, "t") == crf.message_weights(7, 4, "t") == (7.0, None)
    assert np.array_equal(dcrf.message_weights(m, 4, "t")[1], crf.message_weights(m, 4, "t")[1])
    assert np.array_equal(crf.message_weights(m, 4, "t")[1], -0.5 * (m + m.T))
    assert np.array_equal(crf.message_weights(m[0], 4, "t")[1], np.diag(-m[0]))
