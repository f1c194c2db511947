"""GPU: the stand-alone DenseCRF (pnp_crf_* in csrc/crf_op.hip, pnp_ovss.crf, the pydensecrf shim) against the oracle with
external unary energies: OP.densecrf_variant(rgb, zeros, variant=0, unary=U, **params).

Shapes (K, H, W) are the smallest that reach every dispatch of crf_filter / crf_update / the planes <-> rows kernels:
(3, 37, 53) LPP 8; (21, 45, 61) LPP 8, narrow rows; (33, 29, 41) LPP 16, wide rows; (100, 25, 33) LPP 32; (150, 23, 31) MULTI
splat, wave softmax.  Marginals are held to _post_refs.Q_ATOL (1e-6, the project's bound for this arithmetic), labels to
equality wherever the oracle's two largest marginals differ by more than 4 * Q_ATOL; such near-tie pixels may be at most 1 %
of an image, asserted on the oracle first."""
import functools
import importlib
import importlib.util
import os
import sys

import numpy as np
import pytest

import _post_refs as R
from oracle import pipeline_np as OP

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIMS = os.path.join(ROOT, "pnp-ovss_amd", "shims")

SHAPES = [(3, 37, 53), (21, 45, 61), (33, 29, 41), (100, 25, 33), (150, 23, 31)]
PARAMS = [dict(),
          dict(pos_w=3.0, pos_xy=3.0, bi_w=10.0, bi_xy=80.0, bi_rgb=13.0),
          dict(pos_w=3.0, pos_xy=1.0, bi_w=4.0, bi_xy=67.0, bi_rgb=3.0, iters=5),
          dict(pos_w=0.0, bi_w=10.0),
          dict(pos_w=7.0, bi_w=0.0),
          dict(iters=0)]
# the full parameter list at K = 21, the first two sets at the other shapes
CASES = [(s, p) for s in SHAPES for p in range(len(PARAMS)) if s[0] == 21 or p < 2]
NEAR_TIE = 4 * R.Q_ATOL
NEAR_TIE_CAP = 0.01


def _shim_utils():
    spec = importlib.util.spec_from_file_location("_pnp_shim_utils", os.path.join(SHIMS, "pydensecrf", "utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def softmax_input(K, H, W):
    """K smooth sinusoid planes + N(0, 0.3) noise, softmax over the planes: (K, H, W) float32 probabilities."""
    rng = np.random.default_rng(1000 + K)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    k = np.arange(K, dtype=np.float64)[:, None, None]
    logits = 2.0 * np.sin(xx / (5.0 + k % 7) + 0.9 * k) * np.cos(yy / (4.0 + k % 5) - 0.4 * k) + rng.normal(0, 0.3, (K, H, W))
    e = np.exp(logits - logits.max(0))
    p = (e / e.sum(0)).astype(np.float32)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def inputs(K, H, W):
    """(rgb (H, W, 3) uint8, U (K, H*W) float32), read-only."""
    rgb = R.photo_like(H, W, seed=K)
    U = np.ascontiguousarray(_shim_utils().unary_from_softmax(softmax_input(K, H, W)))
    rgb.setflags(write=False)
    U.setflags(write=False)
    return rgb, U


def _oracle(rgb, U, K, H, W, params):
    lab, q = OP.densecrf_variant(rgb, np.zeros((K, H, W), np.float32), variant=0, unary=U.reshape(K, H, W), **params)
    lab = lab.astype(np.uint8)
    lab.setflags(write=False)
    q.setflags(write=False)
    return lab, q


@functools.lru_cache(maxsize=None)
def oracle(shape, pi):
    K, H, W = shape
    rgb, U = inputs(K, H, W)
    return _oracle(rgb, U, K, H, W, PARAMS[pi])


def check_against_oracle(lab, q, ref_lab, ref_q, what):
    """lab (H, W) uint8 / q (K, H, W) float32 numpy from the device against the oracle's."""
    top2 = np.sort(ref_q, axis=0)[-2:]
    tie = (top2[1] - top2[0]) <= NEAR_TIE
    print(f"{what}: oracle near-tie pixels {int(tie.sum())} of {tie.size}")
    assert tie.mean() <= NEAR_TIE_CAP, f"{what}: the oracle itself leaves {int(tie.sum())} near-tie pixels of {tie.size}"
    assert q.shape == ref_q.shape and q.dtype == np.float32
    assert not np.isnan(q).any(), f"{what}: NaN marginals"
    err = float(np.abs(q.astype(np.float64) - ref_q.astype(np.float64)).max())
    print(f"{what}: max |Q - oracle| = {err:.3e}")
    assert err <= R.Q_ATOL, f"{what}: max |Q - oracle| = {err:.3e} > {R.Q_ATOL}"
    assert lab.shape == ref_lab.shape and lab.dtype == np.uint8
    bad = (lab != ref_lab) & ~tie
    assert not bad.any(), f"{what}: {int(bad.sum())} labels differ from the oracle away from its near-ties"


def _np(t):
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def crf():
    from pnp_ovss import crf as mod
    return mod


@pytest.fixture(scope="module")
def solver(crf):
    """One solver large enough for every batch of this module."""
    plan = crf.plan_batch([s[1:] for s in SHAPES], [s[0] for s in SHAPES])
    s = crf.DenseCRF(len(SHAPES), plan["max_total_pixels"], plan["max_pixels_per_image"], plan["max_labels"])
    yield s
    s.close()


@pytest.mark.parametrize("shape,pi", CASES, ids=[f"K{s[0]}-{s[1]}x{s[2]}-p{p}" for s, p in CASES])
def test_single_image_matches_oracle(solver, shape, pi):
    K, H, W = shape
    rgb, U = inputs(K, H, W)
    ref_lab, ref_q = oracle(shape, pi)
    labels, q = solver.run([U], [rgb], **PARAMS[pi])
    assert tuple(labels[0].shape) == (H, W) and tuple(q[0].shape) == (K, H, W)
    check_against_oracle(_np(labels[0]), _np(q[0]), ref_lab, ref_q, f"{shape} {PARAMS[pi]}")
    if pi == 0:                                              # not vacuous: the CRF moves labels away from the unary argmax
        changed = float((ref_lab != U.reshape(K, H, W).argmin(0)).mean())
        print(f"{shape}: the CRF changes {100 * changed:.1f} % of the unary argmax labels")
        assert changed > 0.01


def test_labels_without_marginals(solver):
    K, H, W = SHAPES[1]
    rgb, U = inputs(K, H, W)
    labels, q = solver.run([U], [rgb], want_q=False)
    assert q is None
    ref_lab, ref_q = oracle(SHAPES[1], 0)
    top2 = np.sort(ref_q, axis=0)[-2:]
    tie = (top2[1] - top2[0]) <= NEAR_TIE
    assert not ((_np(labels[0]) != ref_lab) & ~tie).any()


def test_batch_equals_single_runs_bit_for_bit(solver):
    import torch
    three = SHAPES[:3]
    ins = [inputs(*s) for s in three]
    lab_b, q_b = solver.run([u for _, u in ins], [im for im, _ in ins])
    for i, (im, u) in enumerate(ins):
        lab_1, q_1 = solver.run([u], [im])
        assert torch.equal(q_b[i], q_1[0]), f"image {i}: marginals of the batch differ from the single run"
        assert torch.equal(lab_b[i], lab_1[0]), f"image {i}: labels of the batch differ from the single run"


def test_mixed_width_batch_matches_oracle(solver):
    """The narrowest and the widest rows in one batch: every kernel is dispatched for the widest (Kp = 152: wide planes <-> rows
    kernels, MULTI splat, wave softmax) and runs the 4-float rows of the other image too."""
    two = [SHAPES[0], SHAPES[4]]
    ins = [inputs(*s) for s in two]
    labels, q = solver.run([u for _, u in ins], [im for im, _ in ins])
    for i, s in enumerate(two):
        ref_lab, ref_q = oracle(s, 0)
        check_against_oracle(_np(labels[i]), _np(q[i]), ref_lab, ref_q, f"batch image {s}")


def test_solver_reuse_leaves_no_trace(crf):
    import torch
    A = [inputs(*SHAPES[0]), inputs(*SHAPES[1])]
    Bt = [inputs(*SHAPES[2])]
    pix = [s[1] * s[2] for s in SHAPES[:3]]

    def make():                                              # holds batch A (two images, 3 and 21 labels) and the 33-label image
        return crf.DenseCRF(2, pix[0] + pix[1], max(pix), 33)

    def run(s, batch, pi):
        lab, q = s.run([u for _, u in batch], [im for im, _ in batch], **PARAMS[pi])
        return [t.clone() for t in lab], [t.clone() for t in q]

    def same(x, y):
        return all(torch.equal(a, b) for a, b in zip(x[0], y[0])) and all(torch.equal(a, b) for a, b in zip(x[1], y[1]))
    used, fresh0, fresh1 = make(), make(), make()
    try:
        first = run(used, A, 0)
        run(used, Bt, 0)                                     # another batch size in between
        again = run(used, A, 0)
        assert same(first, again)
        assert same(again, run(fresh0, A, 0))
        # same image sizes and pos_xy, other bilateral widths: the used solver keeps its Gaussian lattice, a fresh one builds it
        assert same(run(used, A, 1), run(fresh1, A, 1))
    finally:
        for s in (used, fresh0, fresh1):
            s.close()


def test_device_tensors_in_give_the_same_bits(solver):
    import torch
    K, H, W = SHAPES[1]
    rgb, U = inputs(K, H, W)
    lab_n, q_n = solver.run([U], [rgb])
    lab_n, q_n = lab_n[0].clone(), q_n[0].clone()
    dU = torch.from_numpy(U.copy()).cuda().view(K, H, W)
    dI = torch.from_numpy(rgb.copy()).cuda()
    lab_d, q_d = solver.run([dU], [dI])
    assert lab_d[0].is_cuda and q_d[0].is_cuda and lab_d[0].dtype == torch.uint8 and q_d[0].dtype == torch.float32
    assert torch.equal(q_d[0], q_n) and torch.equal(lab_d[0], lab_n)


def test_key_range_refusal_is_an_error_return(crf):
    """A colour width so small that a bilateral coordinate leaves the 11-bit lattice key: pnp_crf_set_batch refuses the batch
    (an error return, no device fault), and the same solver then runs a width that fits."""
    H, W, K = 30, 40, 3
    white = np.full((H, W, 3), 255, np.uint8)
    corners = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)]
    assert max(R.bilateral_key_extent(x, y, (255, 255, 255), sxy=50.0, srgb=0.5) for x, y in corners) > R.KEY_LIMIT
    assert max(R.bilateral_key_extent(x, y, (255, 255, 255), sxy=50.0, srgb=1.0) for x, y in corners) < R.KEY_LIMIT
    U = np.ascontiguousarray(_shim_utils().unary_from_softmax(softmax_input(K, H, W)))
    s = crf.DenseCRF(1, H * W, H * W, K)
    try:
        with pytest.raises((ValueError, RuntimeError), match="key range") as ei:
            s.run([U], [white], bi_rgb=0.5)
        assert "bi_rgb" in str(ei.value) and str(R.KEY_LIMIT) in str(ei.value)
        assert s.lib.pnp_crf_infer(s.h, 1, 7.0, 10.0, None, None, None) == -1      # PNP_ERR_STATE: the failed set left no batch
        labels, q = s.run([U], [white], bi_rgb=1.0)
        ref_lab, ref_q = _oracle(white, U, K, H, W, dict(bi_rgb=1.0))
        check_against_oracle(_np(labels[0]), _np(q[0]), ref_lab, ref_q, "white image, bi_rgb = 1")
    finally:
        s.close()


def test_shim_end_to_end(crf, monkeypatch):
    """The call sequence of the reference's densecrf() (PnP_OVSS_0514_updated_segmentation.py:1063-1073), argument for argument, on
    the shim -- restated as tests/golden/make_crf_golden.py restates it, not copied."""
    import torch
    monkeypatch.syspath_prepend(SHIMS)
    for m in [m for m in sys.modules if m == "pydensecrf" or m.startswith("pydensecrf.")]:
        monkeypatch.delitem(sys.modules, m)
    importlib.invalidate_caches()
    import pydensecrf.densecrf as dcrf
    import pydensecrf.utils as utils
    assert sys.modules["pydensecrf"].__pnp_ovss_shim__ is True
    try:
        shape = SHAPES[1]
        rgb, _ = inputs(*shape)
        probs = np.array(softmax_input(*shape))              # what the reference's F.softmax(mask, dim=0).cpu().numpy() hands over
        pic = np.ascontiguousarray(rgb).copy()
        n_lab, hh, ww = probs.shape
        # the calls of the reference's densecrf(), restated with its keyword arguments and its integer constants
        # (MAX_ITER 10, POS_W 7, POS_XY_STD 3, Bi_W 10, Bi_XY_STD 50, Bi_RGB_STD 5: PnP.py:1036-1041)
        energies = np.ascontiguousarray(utils.unary_from_softmax(probs))
        model = dcrf.DenseCRF2D(ww, hh, n_lab)
        model.setUnaryEnergy(energies)
        model.addPairwiseGaussian(sxy=3, compat=7)
        model.addPairwiseBilateral(sxy=50, srgb=5, rgbim=pic, compat=10)
        marg = model.inference(10)
        assert isinstance(marg, np.ndarray) and marg.dtype == np.float32 and marg.shape == (n_lab, hh * ww)
        assert np.argmax(marg, axis=0).shape == (hh * ww,)   # the reference's two uses of Q: np.array(Q).reshape((c, h, w)) and
        marg = np.array(marg).reshape((n_lab, hh, ww))       # np.argmax(Q, axis=0).reshape((h, w)).astype(np.float32)
        best = np.argmax(marg, axis=0).reshape((hh, ww)).astype(np.float32)
        ref_lab, ref_q = oracle(shape, 0)
        check_against_oracle(best.astype(np.uint8), marg, ref_lab, ref_q, "shim")
        _, q_direct = crf.densecrf(energies, pic)
        assert np.array_equal(marg, _np(q_direct)), "the shim's marginals differ from pnp_ovss.crf.densecrf's"
        # the two terms added in the other order: the same bits
        other = dcrf.DenseCRF2D(ww, hh, n_lab)
        other.setUnaryEnergy(energies)
        other.addPairwiseBilateral(sxy=50, srgb=5, rgbim=pic, compat=10)
        other.addPairwiseGaussian(sxy=3, compat=7)
        assert np.array_equal(np.array(other.inference(10)).reshape((n_lab, hh, ww)), marg)
    finally:
        for m in [m for m in sys.modules if m == "pydensecrf" or m.startswith("pydensecrf.")]:
            monkeypatch.delitem(sys.modules, m, raising=False)
        torch.cuda.synchronize()
