"""pnp_ovss.crf.FeatureCRF (pnp_crf_create_terms ... pnp_crf_infer_terms) on the GPU: any number of pairwise terms over features
the caller brings.  Bit for bit against DenseCRF.run where the two coincide (xy and xy+rgb features), against the numpy
reference of tests/_crf_terms_ref.py elsewhere under the project's tolerances (marginals within Q_ATOL, labels equal away from
the reference's near-ties, whose share is capped at 1 % and asserted on the reference first)."""
import functools

import numpy as np
import pytest

import _crf_terms_ref as TR
import test_crf_general_gpu as TG
import test_crf_op_gpu as T

pytestmark = pytest.mark.gpu

MIXED = 3                                                    # the (21, 23, 31) case: three terms
BATCH = [(3, 13, 17), (5, 19, 23), (21, 23, 31)]
ALL_SHAPES = sorted({c[0] for c in TR.CASES} | {(3, 37, 53), (21, 45, 61), (150, 23, 31)})


def _np(t):
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def crf():
    from pnp_ovss import crf as mod
    return mod


@pytest.fixture(scope="module")
def solver(crf):
    """One solver large enough for every batch of this module."""
    pix = sorted(s[1] * s[2] for s in ALL_SHAPES)
    s = crf.FeatureCRF(3, sum(pix[-3:]), pix[-1], 150, max_terms=4, max_dims=6)
    yield s
    s.close()


def terms_of(crf, shape, names, compats):
    _, feats = TR.case_inputs(shape, names)
    return [crf.Term([f], c) for f, c in zip(feats, compats)]


def run_case(crf, solver, shape, names, compats, iters=TR.ITERS):
    U, _ = TR.case_inputs(shape, names)
    labels, q = solver.run([U], terms_of(crf, shape, names, compats), iters=iters)
    return labels[0].clone(), q[0].clone()


@functools.lru_cache(maxsize=None)
def case_reference(ci):
    shape, names, weights = TR.CASES[ci]
    return TR.reference(shape, names, weights)


def mixed_compats(K):
    """A scalar, a vector and a non-symmetric matrix for the three terms of the (21, 23, 31) case."""
    rng = np.random.default_rng(400 + K)
    return 3.0, rng.uniform(2.0, 4.0, K).astype(np.float32), TG.matrix(K, 6.0, 500 + K)


# ---- 1. the xy + xy.rgb problem is DenseCRF.run bit for bit
@pytest.mark.parametrize("shape,kind", [((3, 37, 53), "potts"), ((21, 45, 61), "potts"), ((150, 23, 31), "potts"),
                                        ((21, 45, 61), "matrix"), ((21, 45, 61), "aniso")], ids=lambda v: str(v).replace(" ", ""))
def test_position_and_image_features_equal_densecrf_bit_for_bit(crf, solver, shape, kind):
    import torch
    K, H, W = shape
    rgb, U = T.inputs(K, H, W)
    widths = dict(TG.ANISO) if kind == "aniso" else dict(pos_xy=3.0, bi_xy=50.0, bi_rgb=5.0)
    cg, cb = (TG.matrix(K, 7.0, 100 + K), TG.matrix(K, 10.0, 200 + K)) if kind == "matrix" else (7.0, 10.0)
    two = crf.DenseCRF(1, H * W, H * W, K)
    try:
        kw = dict(pos_compat=cg, bi_compat=cb) if kind == "matrix" else {}
        lab2, q2 = two.run([U], [rgb], iters=TR.ITERS, pos_w=7.0, bi_w=10.0, **widths, **kw)
        terms = [crf.Term(crf.position_features([(H, W)], widths["pos_xy"]), cg),
                 crf.Term(crf.image_features([rgb], widths["bi_xy"], widths["bi_rgb"]), cb)]
        lab, q = solver.run([U], terms, iters=TR.ITERS)
        assert torch.equal(q[0], q2[0]), f"{shape} {kind}: marginals differ from DenseCRF.run"
        assert torch.equal(lab[0], lab2[0]), f"{shape} {kind}: labels differ from DenseCRF.run"
    finally:
        two.close()


# ---- 2. the seven cases against the reference
@pytest.mark.parametrize("ci", range(len(TR.CASES)), ids=[f"K{c[0][0]}-" + "+".join(c[1]) for c in TR.CASES])
def test_case_matches_reference(crf, solver, ci):
    shape, names, weights = TR.CASES[ci]
    K, H, W = shape
    ref_lab, ref_q = case_reference(ci)
    lab, q = run_case(crf, solver, shape, names, weights)
    assert tuple(lab.shape) == (H, W) and tuple(q.shape) == (K, H, W)
    T.check_against_oracle(_np(lab), _np(q), ref_lab, ref_q, f"{shape} {names}")
    U, _ = TR.case_inputs(shape, names)
    changed = float((ref_lab != U.reshape(K, H, W).argmin(0)).mean())
    print(f"{shape} {names}: the CRF changes {100 * changed:.1f} % of the unary argmax labels")
    assert changed > 0.01


# ---- 3. a scalar, a vector and a matrix in one run
def test_mixed_compatibility_matches_reference(crf, solver):
    shape, names, weights = TR.CASES[MIXED]
    compats = mixed_compats(shape[0])
    ref_lab, ref_q = TR.reference(shape, names, compats)
    lab, q = run_case(crf, solver, shape, names, compats)
    T.check_against_oracle(_np(lab), _np(q), ref_lab, ref_q, f"{shape} mixed compatibility")
    _, q_scalar = run_case(crf, solver, shape, names, weights)
    assert float((q - q_scalar).abs().max()) > 100 * T.R.Q_ATOL


# ---- 4. batches
def test_batch_equals_single_runs_bit_for_bit(crf, solver):
    import torch
    names, weights = ("d2", "d4"), (3, 6)
    ins = [TR.case_inputs(s, names) for s in BATCH]
    terms = [crf.Term([feats[t] for _, feats in ins], weights[t]) for t in range(2)]
    lab_b, q_b = solver.run([U for U, _ in ins], terms, iters=TR.ITERS)
    lab_b, q_b = [x.clone() for x in lab_b], [x.clone() for x in q_b]
    for i, s in enumerate(BATCH):
        lab_1, q_1 = run_case(crf, solver, s, names, weights)
        assert torch.equal(q_b[i], q_1), f"image {i}: marginals of the batch differ from the single run"
        assert torch.equal(lab_b[i], lab_1), f"image {i}: labels of the batch differ from the single run"


def test_batch_with_a_matrix_equals_single_runs_and_mixed_labels_are_refused(crf, solver):
    import torch
    names = ("d2", "d4")
    shapes = [(5, 19, 23), (5, 13, 17)]
    M = TG.matrix(5, 6.0, 505)
    ins = [TR.case_inputs(s, names) for s in shapes]
    terms = [crf.Term([feats[0] for _, feats in ins], 3.0), crf.Term([feats[1] for _, feats in ins], M)]
    lab_b, q_b = solver.run([U for U, _ in ins], terms, iters=TR.ITERS)
    lab_b, q_b = [x.clone() for x in lab_b], [x.clone() for x in q_b]
    for i, s in enumerate(shapes):
        lab_1, q_1 = run_case(crf, solver, s, names, (3.0, M))
        assert torch.equal(q_b[i], q_1) and torch.equal(lab_b[i], lab_1), f"image {i}: the batch differs from the single run"
    mixed = [TR.case_inputs(s, names) for s in BATCH[:2]]                 # 3 and 5 labels under a 5-label matrix
    bad = [crf.Term([feats[0] for _, feats in mixed], 3.0), crf.Term([feats[1] for _, feats in mixed], M)]
    with pytest.raises(ValueError, match="every image"):
        solver.run([U for U, _ in mixed], bad, iters=TR.ITERS)
    lab_1, q_1 = run_case(crf, solver, shapes[0], names, (3.0, M))        # the solver stays usable
    assert torch.equal(q_b[0], q_1) and torch.equal(lab_b[0], lab_1)


# ---- 5. stepwise
def test_stepwise_equals_one_call_bit_for_bit(crf, solver):
    import torch
    shape, names, _ = TR.CASES[MIXED]
    compats = mixed_compats(shape[0])
    lab, q = run_case(crf, solver, shape, names, compats)
    solver.start()
    solver.step(3)
    solver.step(2)
    lab_s, q_s = solver.read()
    assert torch.equal(q_s[0], q) and torch.equal(lab_s[0], lab)
    U, feats = TR.case_inputs(shape, names)
    fresh = crf.FeatureCRF(1, shape[1] * shape[2], shape[1] * shape[2], shape[0], max_terms=3)
    try:
        d_unary, d_feats, sizes, labels = fresh._gather([U], [crf.Term([f]) for f in feats])
        fresh.set_batch(d_unary, d_feats, [f.shape[0] for f in feats], sizes, labels)
        with pytest.raises(RuntimeError, match="pnp_crf_start"):
            fresh.step()
        with pytest.raises(RuntimeError, match="pnp_crf_start"):
            fresh.read()
        # the two-term calls do not serve a terms batch
        assert fresh.lib.pnp_crf_infer(fresh.h, 1, 7.0, 10.0, None, None, None) == -1          # PNP_ERR_STATE
        assert fresh.lib.pnp_crf_step(fresh.h, 1, 7.0, 10.0, None) == -1
    finally:
        fresh.close()


# ---- 6. refusals
def test_refusals_leave_the_solver_usable(crf, solver):
    import torch
    shape, names, weights = TR.CASES[5]                                   # (33, 17, 21), [d6]
    U, (d6,) = TR.case_inputs(shape, names)
    good = run_case(crf, solver, shape, names, weights)

    def still_good():
        lab, q = run_case(crf, solver, shape, names, weights)
        assert torch.equal(q, good[1]) and torch.equal(lab, good[0])
    far = d6.copy()
    far[5] *= 1e4
    with pytest.raises(ValueError, match="key range") as ei:
        solver.run([U], [crf.Term([far], 10)])
    assert "term 0" in str(ei.value) and "505" in str(ei.value) and "wider" in str(ei.value)
    assert solver.lib.pnp_crf_infer_terms(solver.h, 1, (crf.C.c_float * 1)(10.0), None, None, None) == -1      # no batch is held
    still_good()
    nan = d6.copy()
    nan[2, 3, 4] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        solver.run([U], [crf.Term([nan], 10)])
    still_good()
    with pytest.raises(ValueError, match="feature axes"):
        solver.run([U], [crf.Term([np.concatenate([d6, d6[:1]])], 10)])
    still_good()
    with pytest.raises(ValueError, match="terms"):
        solver.run([U], [crf.Term([d6], 2)] * 5)
    still_good()
    with pytest.raises(ValueError, match="float32"):
        solver.run([U], [crf.Term([d6.astype(np.float64)], 10)])
    still_good()
    with pytest.raises(ValueError, match="features are"):                 # (the unary's (K, H, W) fixes the image size)
        solver.run([U.reshape(shape)], [crf.Term([d6[:, :-1]], 10)])
    still_good()
    with pytest.raises(NotImplementedError, match="KL"):
        solver.kl()
    out = (crf.C.c_double * 1)()
    assert solver.lib.pnp_crf_kl(solver.h, 7.0, 10.0, out, None) == -22 and b"not available" in solver.lib.pnp_crf_last_error(solver.h)


# ---- 7. the workspace's history does not matter
def test_solver_reuse_leaves_no_trace(crf, solver):
    import torch
    shape, names, weights = TR.CASES[MIXED]
    first = run_case(crf, solver, shape, names, weights)
    run_case(crf, solver, *TR.CASES[0])
    again = run_case(crf, solver, shape, names, weights)
    assert torch.equal(first[1], again[1]) and torch.equal(first[0], again[0])


# ---- 8. a solver of pnp_crf_create_terms on the two-term path
def test_terms_solver_serves_the_two_term_calls(crf, solver):
    import torch
    K, H, W = 21, 45, 61
    rgb, U = T.inputs(K, H, W)
    two = crf.DenseCRF(1, H * W, H * W, K)
    try:
        lab2, q2 = two.run([U], [rgb], iters=TR.ITERS)
        as_two = crf.DenseCRF.__new__(crf.DenseCRF)                       # DenseCRF's calls on the FeatureCRF's handle
        as_two.lib, as_two.device, as_two.h, as_two.bounds = solver.lib, solver.device, solver.h, solver.bounds
        try:
            lab, q = as_two.run([U], [rgb], iters=TR.ITERS)
            assert torch.equal(q[0], q2[0]) and torch.equal(lab[0], lab2[0])
            # and the terms calls do not serve a two-term batch
            assert solver.lib.pnp_crf_infer_terms(solver.h, 1, (crf.C.c_float * 2)(7.0, 10.0), None, None, None) == -1
            assert solver.lib.pnp_crf_step_terms(solver.h, 1, (crf.C.c_float * 2)(7.0, 10.0), None) == -1
        finally:
            as_two.h = crf.C.c_void_p()                                   # the handle stays the fixture's
    finally:
        two.close()


# ---- 9. pydensecrf's names (pnp-ovss_amd/shims/nd)
def test_nd_shim_end_to_end(crf, solver, monkeypatch):
    import importlib
    import os
    import sys
    import torch
    for m in [m for m in sys.modules if m == "pydensecrf" or m.startswith("pydensecrf.")]:
        monkeypatch.delitem(sys.modules, m)
    monkeypatch.syspath_prepend(os.path.join(T.SHIMS, "nd"))
    importlib.invalidate_caches()
    dcrf = importlib.import_module("pydensecrf.densecrf")
    assert sys.modules["pydensecrf"].__pnp_ovss_shim_nd__ is True
    shape, names, weights = TR.CASES[2]                                   # (3, 13, 17), [d2, d4], weights 3 / 6
    K, H, W = shape
    U, feats = TR.case_inputs(shape, names)
    d = dcrf.DenseCRF(H * W, K)
    d.setUnaryEnergy(U)
    for f, w in zip(feats, weights):
        d.addPairwiseEnergy(np.ascontiguousarray(f.reshape(f.shape[0], -1)), compat=w)
    q_shim = d.inference(TR.ITERS)
    lab, q = run_case(crf, solver, shape, names, weights)
    assert q_shim.shape == (K, H * W) and np.array_equal(q_shim, _np(q).reshape(K, -1))
    assert np.array_equal(d.map(TR.ITERS), _np(lab).reshape(-1))
    Q, t1, t2 = d.startInference()
    for _ in range(TR.ITERS):
        d.stepInference(Q, t1, t2)
    assert np.array_equal(np.array(Q), q_shim)
    # two bilateral scales on one image
    K, H, W = 21, 23, 31
    rgb, U = T.inputs(K, H, W)
    d2 = dcrf.DenseCRF2D(W, H, K)
    d2.setUnaryEnergy(U)
    d2.addPairwiseGaussian(sxy=3, compat=3)
    d2.addPairwiseBilateral(sxy=50, srgb=5, rgbim=rgb, compat=5)
    d2.addPairwiseBilateral(sxy=(20, 25), srgb=(9, 9, 12), rgbim=rgb, compat=4)
    q2 = d2.inference(TR.ITERS)
    terms = [crf.Term(crf.position_features([(H, W)], 3), 3), crf.Term(crf.image_features([rgb], 50, 5), 5),
             crf.Term(crf.image_features([rgb], (20, 25), (9, 9, 12)), 4)]
    _, q_direct = solver.run([U], terms, iters=TR.ITERS)
    assert np.array_equal(q2, _np(q_direct[0]).reshape(K, -1)) and np.isfinite(q2).all() and np.abs(q2.sum(0) - 1).max() < 1e-5
