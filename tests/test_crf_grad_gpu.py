"""FeatureCRF.marginals on the GPU (pnp_crf_reserve_grad, pnp_crf_infer_terms_saved, pnp_crf_backward_terms): the forward is
FeatureCRF.run bit for bit; the gradients of the unary energies and of every kind of compatibility agree with the float64
reference of tests/_crf_grad_ref.py within its BOUND, on cases chosen for the dispatches that can go wrong; they are
deterministic to the bit, additive over a batch, honour needs_input_grad, refuse a stale batch and leave the stepwise state
alone."""
import numpy as np
import pytest
import torch

import _crf_grad_ref as R
import _crf_terms_ref as TR

pytestmark = pytest.mark.gpu

CASE_IDS = [f"K{TR.CASES[i][0][0]}-{'+'.join(TR.CASES[i][1])}-{k}" for i, k in R.GRAD_CASES]


@pytest.fixture(scope="module")
def crf():
    from pnp_ovss import crf as mod
    return mod


@pytest.fixture(scope="module")
def solver(crf):
    pix = sorted(c[0][1] * c[0][2] for c in TR.CASES)
    s = crf.FeatureCRF(2, pix[-1] + pix[-2], pix[-1], 150, max_terms=4, max_dims=6)
    yield s
    s.close()


def leaves(shape, names, compats, need_compat=True):
    """Device leaf tensors of a case: (unary (K, H, W), [compat tensors])."""
    U, _ = TR.case_inputs(shape, names)
    u = torch.from_numpy(np.array(U).reshape(shape)).cuda().requires_grad_(True)
    cs = [torch.tensor(c, dtype=torch.float32).cuda().requires_grad_(need_compat) for c in compats]
    return u, cs


def terms_of(crf, shape, names, cs):
    _, feats = TR.case_inputs(shape, names)
    return [crf.Term([f], c) for f, c in zip(feats, cs)]


def grads_of(crf, solver, shape, names, compats, need_compat=True):
    u, cs = leaves(shape, names, compats, need_compat)
    (q,) = solver.marginals([u], terms_of(crf, shape, names, cs), iters=R.ITERS)
    (q * torch.from_numpy(np.array(R.cotangent(shape))).cuda()).sum().backward()
    return q.detach(), u.grad, [c.grad for c in cs]


def measure(crf, solver, index, kinds):
    """-> {tensor name: max |g - g_ref| / max |g_ref|} of one case."""
    shape, names, compats = R.case(index, kinds)
    _, gu, gc = grads_of(crf, solver, shape, names, compats)
    ref_u, ref_c = R.gradients(index, kinds)
    out = {"unary": R.rel_err(gu.cpu().numpy(), ref_u)}
    for t, (a, b) in enumerate(zip(gc, ref_c)):
        assert tuple(a.shape) == tuple(np.shape(b)) and a.is_cuda
        out[f"compat{t}"] = R.rel_err(a.cpu().numpy(), b)
    return out


# ---- forward
@pytest.mark.parametrize("ci", [2, 3])
def test_marginals_equal_run_bit_for_bit(crf, solver, ci):
    shape, names, weights = TR.CASES[ci]
    U, _ = TR.case_inputs(shape, names)
    compats = [float(w) for w in weights]
    _, q_run = solver.run([U], terms_of(crf, shape, names, compats), iters=R.ITERS)
    q_run = q_run[0].clone()
    u, cs = leaves(shape, names, compats)
    (q,) = solver.marginals([u], terms_of(crf, shape, names, cs), iters=R.ITERS)
    assert q.requires_grad and tuple(q.shape) == shape
    assert torch.equal(q.detach(), q_run)


def test_a_solver_without_gradients_allocates_what_it_did(crf):
    shape, names, weights = TR.CASES[2]
    K, H, W = shape
    U, _ = TR.case_inputs(shape, names)
    a = crf.FeatureCRF(1, H * W, H * W, K, max_terms=2, max_dims=4)
    b = crf.FeatureCRF(1, H * W, H * W, K, max_terms=2, max_dims=4)
    try:
        before = a.allocated_bytes()
        assert before == b.allocated_bytes()
        a.run([U], terms_of(crf, shape, names, [float(w) for w in weights]), iters=2)
        assert a.allocated_bytes() == before                       # running reserves nothing
        u, cs = leaves(shape, names, [float(w) for w in weights])
        b.marginals([u], terms_of(crf, shape, names, cs), iters=2)
        grown = b.allocated_bytes()
        assert grown >= before + 4 * 4 * H * W * 4                 # four row arrays of Kp = 4 floats per pixel at least
        b.marginals([u], terms_of(crf, shape, names, cs), iters=2)
        assert b.allocated_bytes() == grown                        # reserved once
    finally:
        a.close()
        b.close()


def test_backward_needs_the_reserved_workspace(crf):
    """The C ABI without pnp_crf_reserve_grad: PNP_ERR_STATE (-1), and on a two-term solver too."""
    import ctypes as C
    shape, names, weights = TR.CASES[0]
    K, H, W = shape
    U, _ = TR.case_inputs(shape, names)
    s = crf.FeatureCRF(1, H * W, H * W, K, max_terms=1, max_dims=1)
    two = crf.DenseCRF(1, H * W, H * W, K)
    try:
        s.run([U], terms_of(crf, shape, names, [5.0]), iters=1)
        buf = torch.zeros(8 * K * H * W, device="cuda")
        w = (C.c_float * 1)(5.0)
        p = C.c_void_p(buf.data_ptr())
        assert s.lib.pnp_crf_backward_terms(s.h, 1, w, p, p, p, None, None) == -1
        assert b"pnp_crf_reserve_grad" in s.lib.pnp_crf_last_error(s.h)
        assert two.lib.pnp_crf_reserve_grad(two.h) == -1
    finally:
        s.close()
        two.close()


# ---- gradients against the float64 reference
@pytest.mark.parametrize("index,kinds", R.GRAD_CASES, ids=CASE_IDS)
def test_gradients_match_the_float64_reference(crf, solver, index, kinds):
    errs = measure(crf, solver, index, kinds)
    for name, e in errs.items():
        print(f"case {index} {kinds} {name}: max|g - g_ref| / max|g_ref| = {e:.3e}")
    assert R.BOUND <= 1e-3
    for name, e in errs.items():
        assert e <= R.BOUND, f"case {index} {kinds} {name}: {e:.3e} > {R.BOUND:.0e}"


def test_two_backward_calls_give_equal_bits(crf, solver):
    shape, names, compats = R.case(3, "smm")
    _, gu1, gc1 = grads_of(crf, solver, shape, names, compats)
    _, gu2, gc2 = grads_of(crf, solver, shape, names, compats)
    assert torch.equal(gu1, gu2)
    for a, b in zip(gc1, gc2):
        assert torch.equal(a, b)


def test_batch_of_two_sizes(crf, solver):
    """(3, 13, 17) d2 + d4 next to a 3-label crop of another size: unary gradients of the batch equal the single runs bit for
    bit; the compatibility gradients are the sums of the singles within the bound."""
    (shape, names, compats) = R.case(2, "sv")
    K = shape[0]
    shapes = [shape, (K, 11, 9)]
    feats, us = [], []
    for sh in shapes:
        U, f = TR.case_inputs(sh, names)
        feats.append(f)
        us.append(np.array(U).reshape(sh))
    cot = [torch.from_numpy(np.array(R.cotangent(shape))).cuda(), torch.from_numpy(np.array(R.cotangent((K + 1, 11, 9))[:K])).cuda()]

    def run(idx):
        u = [torch.from_numpy(us[i]).cuda().requires_grad_(True) for i in idx]
        cs = [torch.tensor(c, dtype=torch.float32).cuda().requires_grad_(True) for c in compats]
        terms = [crf.Term([feats[i][t] for i in idx], c) for t, c in enumerate(cs)]
        qs = solver.marginals(u, terms, iters=R.ITERS)
        sum((q * cot[i]).sum() for q, i in zip(qs, idx)).backward()
        return [x.grad for x in u], [c.grad for c in cs]
    both_u, both_c = run([0, 1])
    singles = [run([0]), run([1])]
    for i in range(2):
        assert torch.equal(both_u[i], singles[i][0][0]), f"image {i}"
    for t in range(len(compats)):
        want = singles[0][1][t].double() + singles[1][1][t].double()
        err = float((both_c[t].double() - want).abs().max() / want.abs().max())
        print(f"batch, compat {t}: |batch - sum of singles| / max = {err:.3e}")
        assert err <= R.BOUND


def test_needs_input_grad(crf, solver):
    shape, names, compats = R.case(3, "smm")
    _, gu_full, _ = grads_of(crf, solver, shape, names, compats)
    _, gu_only, gc = grads_of(crf, solver, shape, names, compats, need_compat=False)
    assert all(g is None for g in gc)
    assert torch.equal(gu_only, gu_full)


def test_stale_batch_raises_and_the_solver_stays_usable(crf, solver):
    shape, names, compats = R.case(2, "sv")
    u, cs = leaves(shape, names, compats)
    (q,) = solver.marginals([u], terms_of(crf, shape, names, cs), iters=2)
    other, onames, oweights = TR.CASES[0]
    U0, _ = TR.case_inputs(other, onames)
    _, q_before = solver.run([U0], terms_of(crf, other, onames, [float(w) for w in oweights]), iters=2)
    q_before = q_before[0].clone()
    with pytest.raises(RuntimeError, match="another batch"):
        q.sum().backward()
    _, q_after = solver.run([U0], terms_of(crf, other, onames, [float(w) for w in oweights]), iters=2)
    assert torch.equal(q_after[0], q_before)
    _, gu, _ = grads_of(crf, solver, shape, names, compats)
    assert gu is not None and bool(torch.isfinite(gu).all())


def test_step_and_read_after_backward(crf, solver):
    shape, names, compats = R.case(2, "sv")
    u, cs = leaves(shape, names, compats)
    (q,) = solver.marginals([u], terms_of(crf, shape, names, cs), iters=3)
    lab0, q0 = solver.read()
    lab0, q0 = lab0[0].clone(), q0[0].clone()
    assert torch.equal(q0, q.detach())
    (q * torch.from_numpy(np.array(R.cotangent(shape))).cuda()).sum().backward()
    lab1, q1 = solver.read()
    assert torch.equal(q1[0], q0) and torch.equal(lab1[0], lab0)
    solver.step(2)
    _, q5 = solver.read()
    u2, cs2 = leaves(shape, names, compats)
    (q_ref,) = solver.marginals([u2], terms_of(crf, shape, names, cs2), iters=5)
    assert torch.equal(q5[0], q_ref.detach())


# ---- compatibilities that are no tensors are constants of the graph
def test_numpy_compatibilities_equal_run_bit_for_bit(crf, solver):
    """A numpy (K,) vector and (K, K) matrix (and a number) given to marginals are what they are to run(); the unary gradient is
    the one of the same values given as tensors."""
    shape, names, compats = R.case(3, "svm")
    U, _ = TR.case_inputs(shape, names)
    assert [np.ndim(c) for c in compats] == [0, 1, 2] and all(isinstance(c, np.ndarray) for c in compats[1:])
    _, q_run = solver.run([U], terms_of(crf, shape, names, compats), iters=R.ITERS)
    q_run = q_run[0].clone()
    u, _ = leaves(shape, names, compats)
    (q,) = solver.marginals([u], terms_of(crf, shape, names, compats), iters=R.ITERS)
    assert torch.equal(q.detach(), q_run)
    (q * torch.from_numpy(np.array(R.cotangent(shape))).cuda()).sum().backward()
    _, gu, _ = grads_of(crf, solver, shape, names, compats)
    assert torch.equal(u.grad, gu)


def test_backward_uses_the_compatibilities_of_its_forward(crf, solver):
    """An in-place update of a compatibility tensor between forward and backward (an optimiser step) does not reach backward."""
    shape, names, compats = R.case(2, "sv")
    _, gu, gc = grads_of(crf, solver, shape, names, compats)
    u, cs = leaves(shape, names, compats)
    (q,) = solver.marginals([u], terms_of(crf, shape, names, cs), iters=R.ITERS)
    with torch.no_grad():
        for c in cs:
            c.mul_(0.5)
    (q * torch.from_numpy(np.array(R.cotangent(shape))).cuda()).sum().backward()
    assert torch.equal(u.grad, gu)
    for a, b in zip([c.grad for c in cs], gc):
        assert torch.equal(a, b)


# ---- more tiles than the partial buffer holds: a 1-D signal
def test_one_dimensional_signal_passes_the_partial_buffer_in_spans(crf):
    """600 samples are 38 tiles of 16 x 16 pixels; a solver sized for them holds the partials of 20, one sized for 16 times the
    pixels holds them all.  Same bits from both, and the float64 reference within the bound."""
    import _crf_general_ref as G
    K, N = 3, 600
    rng = np.random.default_rng(3)
    x = np.arange(N, dtype=np.float32)
    sig = (np.sin(x / 40.0) + rng.normal(0, 0.1, N)).astype(np.float32)
    feats = [np.stack([x / np.float32(6.0)]), np.stack([x / np.float32(25.0), sig / np.float32(0.3)])]
    U = rng.normal(0, 1, (K, N)).astype(np.float32)
    compats = [R._vector(K, 3.0, 31), R._matrix(K, 4.0, 32)]
    cot = rng.normal(size=(K, 1, N)).astype(np.float32)

    def run(solver):
        u = torch.from_numpy(U).cuda().requires_grad_(True)
        cs = [torch.from_numpy(c).cuda().requires_grad_(True) for c in compats]
        (q,) = solver.marginals([u], [crf.Term([f], c) for f, c in zip(feats, cs)], iters=R.ITERS)
        (q * torch.from_numpy(cot).cuda()).sum().backward()
        return [u.grad] + [c.grad for c in cs]
    small = crf.FeatureCRF(1, N, N, K, max_terms=2, max_dims=2)
    large = crf.FeatureCRF(1, 16 * N, N, K, max_terms=2, max_dims=2)
    try:
        got, whole = run(small), run(large)
    finally:
        small.close()
        large.close()
    for a, b in zip(got, whole):
        assert torch.equal(a, b)
    ops = [torch.from_numpy(R._operator(G.Lattice(np.ascontiguousarray(f.T)))) for f in feats]
    Ud = torch.from_numpy(U.astype(np.float64)).requires_grad_(True)
    cd = [torch.from_numpy(c.astype(np.float64)).requires_grad_(True) for c in compats]
    (R.meanfield(Ud, ops, cd) * torch.from_numpy(cot.astype(np.float64).reshape(K, N))).sum().backward()
    for name, a, b in zip(("unary", "compat0", "compat1"), got, [Ud.grad] + [c.grad for c in cd]):
        err = R.rel_err(a.cpu().numpy().reshape(b.shape), b.numpy())
        print(f"1-D signal {name}: max|g - g_ref| / max|g_ref| = {err:.3e}")
        assert err <= R.BOUND
