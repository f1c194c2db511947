"""GPU: the general stand-alone DenseCRF -- label-compatibility vectors / matrices (crf_update_compat_kernel), per-axis kernel
widths, stepwise inference and the KL divergence -- through pnp_ovss.crf and the pydensecrf shim, against the numpy restatement
of tests/_crf_general_ref.py (itself held to the oracle and to a brute force by tests/test_crf_general_cpu.py).

Shapes (K, H, W): the smallest that reach every dispatch of the compatibility kernel (pixels per tile TP by the LDS the three
rows per pixel take; a wave multiplies CRF_CL = 8 labels at a time; 4 / (TP / 64) waves share a pixel set) and of the planes /
rows kernels.  In brackets the tile of the KL form of the kernel (four rows per pixel), where it differs:
  (3, 37, 53)    Kp 4: TP 256, one wave per pixel set, one partial label block; narrow planes kernels; edge tiles both ways
  (8, 19, 23)    Kp 8: TP 256, exactly one full label block
  (9, 19, 23)    Kp 12: TP 256 [128], one full block and one label
  (13, 17, 21)   Kp 16: TP 128, two waves per pixel set, the second with the partial block
  (21, 45, 61)   Kp 24: TP 128, three blocks over two waves
  (33, 29, 41)   Kp 36: TP 64, four waves per pixel set, the fourth idle but for one label; wide planes kernels (Kp >= 32)
  (150, 23, 31)  Kp 152: TP 64 [32], 19 blocks over four waves, a tile above 64 KB of LDS; wave softmax in the Potts kernel
  (203, 9, 13)   Kp 204: TP 32, half the lanes of a wave idle (three rows of 205 floats x 64 pixels pass the CU's LDS)
Marginals are held to _post_refs.Q_ATOL and labels to equality away from the reference's near-ties, with the near-tie cap of
tests/test_crf_op_gpu.py asserted on the reference first; `bit for bit` means torch.equal."""
import functools
import importlib
import os
import sys

import numpy as np
import pytest

import _crf_general_ref as G
import _post_refs as R
import test_crf_op_gpu as T

pytestmark = pytest.mark.gpu

SHAPES = [(3, 37, 53), (8, 19, 23), (9, 19, 23), (13, 17, 21), (21, 45, 61), (33, 29, 41), (150, 23, 31), (203, 9, 13)]
WG, WB = 7.0, 10.0                                           # the Potts weights the matrices are built round
ITERS = 5
ANISO = dict(pos_xy=(2.0, 4.0), bi_xy=(40.0, 70.0), bi_rgb=(4.0, 6.0, 9.0))
# full matrices on both terms at every shape; the other kinds at the two shapes of the CPU checks
KINDS = [(s, "both") for s in SHAPES] + [(s, k) for s in SHAPES[:1] + SHAPES[4:5] for k in ("gauss", "bilat", "diag")]


def matrix(K, w, seed, symmetric=False):
    """w I plus off-diagonal entries drawn in [-0.3 w, 0]: float32, read-only; not symmetric unless asked."""
    rng = np.random.default_rng(seed)
    off = rng.uniform(-0.3 * w, 0.0, (K, K))
    if symmetric:
        off = 0.5 * (off + off.T)
    m = (np.diag(np.full(K, w)) + off * (1 - np.eye(K))).astype(np.float32)
    m.setflags(write=False)
    return m


def compats(K, kind):
    """(pos_w, bi_w, pos_compat, bi_compat) of a case."""
    if kind == "both":
        return WG, WB, matrix(K, WG, 100 + K), matrix(K, WB, 200 + K)
    if kind == "gauss":
        return WG, WB, matrix(K, WG, 100 + K), None
    if kind == "bilat":
        return WG, WB, None, matrix(K, WB, 200 + K)
    if kind == "sym":
        return WG, WB, matrix(K, WG, 100 + K, True), matrix(K, WB, 200 + K, True)
    rng = np.random.default_rng(300 + K)
    return WG, WB, rng.uniform(0.5 * WG, WG, K).astype(np.float32), rng.uniform(0.5 * WB, WB, K).astype(np.float32)


def ref_weights(pos_w, bi_w, pos_c, bi_c):
    return (pos_w if pos_c is None else pos_c), (bi_w if bi_c is None else bi_c)


@functools.lru_cache(maxsize=None)
def model(shape, widths=()):
    K, H, W = shape
    rgb, U = T.inputs(K, H, W)
    return G.MeanField(rgb, U, **dict(widths))


@functools.lru_cache(maxsize=None)
def reference(shape, kind, widths=(), iters=ITERS):
    """-> (labels, marginals) of the numpy reference, read-only, computed once per case."""
    if kind == "potts":
        cg, cb = WG, WB
    else:
        cg, cb = ref_weights(*compats(shape[0], kind))
    q = model(shape, widths).run(iters, cg, cb)
    lab = G.labels_of(q)
    q.setflags(write=False)
    lab.setflags(write=False)
    return lab, q


def _np(t):
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def crf():
    from pnp_ovss import crf as mod
    return mod


@pytest.fixture(scope="module")
def solver(crf):
    plan = crf.plan_batch([s[1:] for s in SHAPES], [s[0] for s in SHAPES])
    s = crf.DenseCRF(3, plan["max_total_pixels"], plan["max_pixels_per_image"], plan["max_labels"])
    yield s
    s.close()


# ---- 1. M = w I and the constant vector reproduce the Potts kernel
@pytest.mark.parametrize("shape", SHAPES, ids=[f"K{s[0]}" for s in SHAPES])
def test_identity_matrix_and_constant_vector_equal_potts_bit_for_bit(solver, shape):
    import torch
    K, H, W = shape
    rgb, U = T.inputs(K, H, W)
    lab_p, q_p = solver.run([U], [rgb], pos_w=WG, bi_w=WB)
    lab_p, q_p = lab_p[0].clone(), q_p[0].clone()
    eye_g, eye_b = np.diag(np.full(K, WG, np.float32)), np.diag(np.full(K, WB, np.float32))
    vec_g, vec_b = np.full(K, WG, np.float32), np.full(K, WB, np.float32)
    for what, cg, cb in (("w I", eye_g, eye_b), ("vector w", vec_g, vec_b), ("w I beside a scalar", eye_g, None)):
        lab, q = solver.run([U], [rgb], pos_w=3.0 if cg is not None else WG, bi_w=WB, pos_compat=cg, bi_compat=cb)
        assert torch.equal(q[0], q_p), f"{shape} {what}: marginals differ from the Potts run"
        assert torch.equal(lab[0], lab_p), f"{shape} {what}: labels differ from the Potts run"


# ---- 2. matrices / vectors against the reference
@pytest.mark.parametrize("shape,kind", KINDS, ids=[f"K{s[0]}-{k}" for s, k in KINDS])
def test_compatibility_matches_reference(solver, shape, kind):
    K, H, W = shape
    rgb, U = T.inputs(K, H, W)
    pos_w, bi_w, cg, cb = compats(K, kind)
    ref_lab, ref_q = reference(shape, kind)
    labels, q = solver.run([U], [rgb], iters=ITERS, pos_w=pos_w, bi_w=bi_w, pos_compat=cg, bi_compat=cb)
    T.check_against_oracle(_np(labels[0]), _np(q[0]), ref_lab, ref_q, f"{shape} {kind}")
    if kind == "both":                                       # not vacuous: the off-diagonal weights move the marginals
        _, q_p = solver.run([U], [rgb], iters=ITERS, pos_w=pos_w, bi_w=bi_w)
        assert float((q_p[0] - q[0]).abs().max()) > 100 * R.Q_ATOL


# ---- 3. per-axis widths
def test_per_axis_widths_match_reference(solver):
    shape = SHAPES[4]
    rgb, U = T.inputs(*shape)
    widths = tuple(sorted(ANISO.items()))
    ref_lab, ref_q = reference(shape, "potts", widths)
    labels, q = solver.run([U], [rgb], iters=ITERS, pos_w=WG, bi_w=WB, **ANISO)
    T.check_against_oracle(_np(labels[0]), _np(q[0]), ref_lab, ref_q, f"{shape} {ANISO}")
    iso_lab, iso_q = reference(shape, "potts")
    assert float(np.abs(iso_q - ref_q).max()) > 100 * R.Q_ATOL           # the widths matter


def test_equal_tuples_equal_the_scalar_call_bit_for_bit(solver):
    import torch
    rgb, U = T.inputs(*SHAPES[4])
    lab_s, q_s = solver.run([U], [rgb], **T.PARAMS[1])
    lab_s, q_s = lab_s[0].clone(), q_s[0].clone()
    p = dict(T.PARAMS[1])
    p.update(pos_xy=(3.0, 3.0), bi_xy=(80.0, 80.0), bi_rgb=(13.0, 13.0, 13.0))
    lab_t, q_t = solver.run([U], [rgb], **p)
    assert torch.equal(q_t[0], q_s) and torch.equal(lab_t[0], lab_s)


def test_gaussian_lattice_cache_keys_on_both_widths(solver):
    """Same image size, (sx, sy) swapped: the kept Gaussian lattice must be rebuilt (result against the reference of the swapped
    widths); the same call again reuses it (result unchanged)."""
    import torch
    shape = SHAPES[4]
    rgb, U = T.inputs(*shape)
    solver.run([U], [rgb], iters=ITERS, pos_w=WG, bi_w=WB, pos_xy=(2.0, 4.0))
    labels, q = solver.run([U], [rgb], iters=ITERS, pos_w=WG, bi_w=WB, pos_xy=(4.0, 2.0))
    first = q[0].clone()
    ref_lab, ref_q = reference(shape, "potts", (("pos_xy", (4.0, 2.0)),))
    T.check_against_oracle(_np(labels[0]), _np(first), ref_lab, ref_q, f"{shape} pos_xy (4, 2) after (2, 4)")
    _, again = solver.run([U], [rgb], iters=ITERS, pos_w=WG, bi_w=WB, pos_xy=(4.0, 2.0))
    assert torch.equal(again[0], first)


# ---- 4. stepwise inference
@pytest.mark.parametrize("kind", ["potts", "both"])
def test_stepwise_equals_one_call_bit_for_bit(solver, kind):
    import torch
    shape = SHAPES[4]
    rgb, U = T.inputs(*shape)
    cg, cb = (None, None) if kind == "potts" else compats(shape[0], kind)[2:]
    lab5, q5 = solver.run([U], [rgb], iters=5, pos_w=WG, bi_w=WB, pos_compat=cg, bi_compat=cb)
    lab5, q5 = lab5[0].clone(), q5[0].clone()
    lab_r, q_r = solver.read()                               # read() after run: the run's result, labels as infer wrote them
    assert torch.equal(q_r[0], q5) and torch.equal(lab_r[0], lab5)
    solver.start()
    solver.step(3)
    solver.step(0)                                           # a no-op
    _, q3 = solver.read(want_labels=False)
    q3 = q3[0].clone()
    solver.step(0)
    assert torch.equal(solver.read()[1][0], q3)
    solver.step(2)
    lab_s, q_s = solver.read()
    assert torch.equal(q_s[0], q5), "start, step(3), step(2) differs from run(iters=5)"
    assert torch.equal(lab_s[0], lab5), "labels of read() differ from the labels infer wrote"
    assert not torch.equal(q3, q5)
    _, q3_run = solver.run([U], [rgb], iters=3, pos_w=WG, bi_w=WB, pos_compat=cg, bi_compat=cb)
    assert torch.equal(q3_run[0], q3)


def test_stepwise_calls_before_start_are_state_errors(crf):
    K, H, W = SHAPES[0]
    rgb, U = T.inputs(K, H, W)
    s = crf.DenseCRF(1, H * W, H * W, K)
    try:
        for call in (s.start, s.step, s.read, s.kl):         # no batch: refused on the host
            with pytest.raises(RuntimeError, match="no batch"):
                call()
        out = (crf.C.c_double * 1)()
        assert s.lib.pnp_crf_start(s.h, None) == -1          # PNP_ERR_STATE: no batch
        d_u, d_rgb, sizes, labels = s._gather([U], [rgb])
        s.set_batch(d_u, d_rgb, sizes, labels)
        assert s.lib.pnp_crf_step(s.h, 1, 7.0, 10.0, None) == -1         # PNP_ERR_STATE: a batch, but no start
        assert b"start" in s.lib.pnp_crf_last_error(s.h)
        assert s.lib.pnp_crf_read(s.h, None, None, None) == -1
        assert s.lib.pnp_crf_kl(s.h, 7.0, 10.0, out, None) == -1
        with pytest.raises(RuntimeError, match="start"):
            s.step()
        s.start()
        s.step(2)
        ref_lab, ref_q = reference(SHAPES[0], "potts", (), 2)
        lab, q = s.read()
        T.check_against_oracle(_np(lab[0]), _np(q[0]), ref_lab, ref_q, "start, step(2) on a fresh solver")
        s.set_batch(d_u, d_rgb, sizes, labels)               # a new batch ends the inference
        assert s.lib.pnp_crf_read(s.h, None, None, None) == -1
    finally:
        s.close()


# ---- 5. KL divergence
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[4], SHAPES[6]], ids=lambda s: f"K{s[0]}")
def test_kl_matches_reference(solver, shape):
    """After 0, 1 and 5 steps, with symmetric matrices on both terms, against the reference's float64 value.  Bound: the
    first-order reach of Q_ATOL, Q_ATOL * sum(|log max(Q, 1e-20)| + 1 + |U| + 2 sum_t |acc_t|), computed from the reference.
    The divergence is asserted not to increase from step 1 to step 5 only where the reference itself does not (parallel
    mean-field updates need not decrease it)."""
    K, H, W = shape
    rgb, U = T.inputs(K, H, W)
    pos_w, bi_w, cg, cb = compats(K, "sym")
    m = model(shape)
    solver.run([U], [rgb], iters=0, pos_w=pos_w, bi_w=bi_w, pos_compat=cg, bi_compat=cb)
    solver.start()
    q_ref = m.start()
    got, want = {}, {}
    for step in range(6):
        if step:
            solver.step(1)
            q_ref = m.step(q_ref, cg, cb)
        if step in (0, 1, 5):
            value, reach = m.kl(q_ref, cg, cb)
            kl = solver.kl()
            assert len(kl) == 1
            print(f"{shape} step {step}: KL {kl[0]:.6f}, reference {value:.6f}, bound {R.Q_ATOL * reach:.3e}")
            assert abs(kl[0] - value) <= R.Q_ATOL * reach
            got[step], want[step] = kl[0], value
    _, q = solver.read(want_labels=False)
    assert float(np.abs(_np(q[0]) - q_ref).max()) <= R.Q_ATOL            # kl() left the marginals alone
    if want[5] <= want[1]:
        assert got[5] <= got[1]
    else:
        print(f"{shape}: the reference's divergence rises from step 1 to step 5 ({want[1]:.6f} -> {want[5]:.6f}): not asserted")


def test_kl_of_a_batch_equals_the_single_runs(solver):
    K = 21
    sizes = [(45, 61), (29, 41)]
    ins = [T.inputs(K, h, w) for h, w in sizes]
    _, _, cg, cb = compats(K, "sym")
    singles = []
    for im, u in ins:
        solver.run([u], [im], iters=2, pos_w=WG, bi_w=WB, pos_compat=cg, bi_compat=cb)
        singles.append(solver.kl()[0])
    solver.run([u for _, u in ins], [im for im, _ in ins], iters=2, pos_w=WG, bi_w=WB, pos_compat=cg, bi_compat=cb)
    both = solver.kl()
    assert both == singles
    assert both == solver.kl()                               # deterministic
    # Potts terms on a mixed-K batch: the divergence needs no matrix from the caller
    mixed = [T.inputs(*SHAPES[0]), T.inputs(*SHAPES[4])]
    solver.run([u for _, u in mixed], [im for im, _ in mixed], iters=1, pos_w=WG, bi_w=WB)
    two = solver.kl()
    for i, s in enumerate((SHAPES[0], SHAPES[4])):
        mf = model(s)
        value, reach = mf.kl(mf.run(1, WG, WB), WG, WB)
        assert abs(two[i] - value) <= R.Q_ATOL * reach


# ---- 6. batches
def test_batch_with_a_matrix_equals_single_runs_bit_for_bit(solver):
    import torch
    K = 21
    ins = [T.inputs(K, h, w) for h, w in [(45, 61), (29, 41), (23, 31)]]
    pos_w, bi_w, cg, cb = compats(K, "both")
    lab_b, q_b = solver.run([u for _, u in ins], [im for im, _ in ins], pos_w=pos_w, bi_w=bi_w, pos_compat=cg, bi_compat=cb)
    for i, (im, u) in enumerate(ins):
        lab_1, q_1 = solver.run([u], [im], pos_w=pos_w, bi_w=bi_w, pos_compat=cg, bi_compat=cb)
        assert torch.equal(q_b[i], q_1[0]), f"image {i}: marginals of the batch differ from the single run"
        assert torch.equal(lab_b[i], lab_1[0]), f"image {i}: labels of the batch differ from the single run"


def test_mixed_label_counts_with_a_matrix_are_refused(solver):
    a, b = T.inputs(*SHAPES[4]), T.inputs(*SHAPES[0])
    _, _, cg, cb = compats(21, "both")
    with pytest.raises(ValueError, match="every image"):
        solver.run([a[1], b[1]], [a[0], b[0]], bi_compat=cb)
    # the C ABI refuses it too: the matrix is held, then a mixed batch arrives
    solver.run([a[1]], [a[0]], iters=1, bi_compat=cb)
    d_u, d_rgb, sizes, labels = solver._gather([a[1], b[1]], [a[0], b[0]])
    solver.set_batch(d_u, d_rgb, sizes, labels)
    with pytest.raises(ValueError, match="every image"):
        solver.infer(iters=1)
    # and the solver goes on: the same batch with Potts terms, then the matrix on a batch it fits
    solver.set_compat(None, None)
    lab, q = solver.infer(iters=ITERS, pos_w=WG, bi_w=WB)
    ref_lab, ref_q = reference(SHAPES[0], "potts")
    T.check_against_oracle(_np(lab[1]), _np(q[1]), ref_lab, ref_q, "mixed batch, Potts, after the refusal")
    lab, q = solver.run([a[1]], [a[0]], iters=ITERS, pos_w=WG, bi_w=WB, pos_compat=cg, bi_compat=cb)
    ref_lab, ref_q = reference(SHAPES[4], "both")
    T.check_against_oracle(_np(lab[0]), _np(q[0]), ref_lab, ref_q, "matrix run after the refusal")


# ---- 7. the shim, on calls the Potts-only shim refused
def test_shim_stepwise_loop_with_vector_and_matrix(crf, monkeypatch):
    import torch
    monkeypatch.syspath_prepend(os.path.join(T.SHIMS, "general"))        # the general shim: a package of its own
    for m in [m for m in sys.modules if m == "pydensecrf" or m.startswith("pydensecrf.")]:
        monkeypatch.delitem(sys.modules, m)
    importlib.invalidate_caches()
    import pydensecrf.densecrf as dcrf
    assert sys.modules["pydensecrf"].__pnp_ovss_shim_general__ is True
    try:
        shape = SHAPES[4]
        K, H, W = shape
        rgb, U = T.inputs(K, H, W)
        pic = np.ascontiguousarray(rgb).copy()
        rng = np.random.default_rng(77)
        cost = rng.uniform(0.0, 3.0, (K, K)).astype(np.float32)          # a label-cost matrix, not symmetric, diagonal and all
        np.fill_diagonal(cost, -10.0)
        d = dcrf.DenseCRF2D(W, H, K)
        d.setUnaryEnergy(np.array(U))
        d.addPairwiseGaussian(sxy=(3, 3), compat=np.full(K, 3, np.float32))
        d.addPairwiseBilateral(sxy=(80, 80), srgb=(13, 13, 13), rgbim=pic, compat=cost)
        # what the shim is documented to hand the solver: diag(-v) and -(m + m^T) / 2
        Mg, Mb = np.diag(np.full(K, -3, np.float32)), (-0.5 * (cost + cost.T)).astype(np.float32)
        mf = G.MeanField(rgb, U, 3.0, 80.0, 13.0)
        q_ref = mf.start()
        Q, tmp1, tmp2 = d.startInference()
        for i in range(5):
            d.stepInference(Q, tmp1, tmp2)
            kl = d.klDivergence(Q)
            q_ref = mf.step(q_ref, Mg, Mb)
            value, reach = mf.kl(q_ref, Mg, Mb)
            print(f"shim step {i + 1}: KL {kl:.6f}, reference {value:.6f}")
            assert isinstance(kl, float) and abs(kl - value) <= R.Q_ATOL * reach
        marg = np.array(Q)
        assert marg.dtype == np.float32 and marg.shape == (K, H * W)
        best = np.argmax(marg, axis=0).reshape(H, W).astype(np.uint8)
        T.check_against_oracle(best, marg.reshape(K, H, W), G.labels_of(q_ref), q_ref, "shim, vector + matrix, five steps")
        # inference(5) and map(5) of a fresh object: the same marginals, bit for bit
        e = dcrf.DenseCRF2D(W, H, K)
        e.setUnaryEnergy(np.array(U))
        e.addPairwiseGaussian(sxy=(3, 3), compat=np.full(K, 3, np.float32))
        e.addPairwiseBilateral(sxy=(80, 80), srgb=(13, 13, 13), rgbim=pic, compat=cost)
        assert np.array_equal(e.inference(5), marg)
        assert np.array_equal(e.map(5), np.argmax(marg, axis=0))
        with pytest.raises(RuntimeError, match="startInference"):        # e's runs took the module's solver over
            d.stepInference(Q, tmp1, tmp2)
        # the reference's own call (numbers throughout) gives what pnp_ovss.crf.densecrf gives: the Potts-only shim's bits
        f = dcrf.DenseCRF2D(W, H, K)
        f.setUnaryEnergy(np.array(U))
        f.addPairwiseGaussian(sxy=3, compat=7)
        f.addPairwiseBilateral(sxy=50, srgb=5, rgbim=pic, compat=10)
        _, q_direct = crf.densecrf(np.array(U), pic)
        assert np.array_equal(f.inference(10), _np(q_direct).reshape(K, H * W))
    finally:
        for m in [m for m in sys.modules if m == "pydensecrf" or m.startswith("pydensecrf.")]:
            monkeypatch.delitem(sys.modules, m, raising=False)
        torch.cuda.synchronize()
