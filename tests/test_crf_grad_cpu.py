"""CPU: the float64 yardstick of the mean-field gradients (tests/_crf_grad_ref.py) -- its forward against the project's float32
reference, its autograd gradients against central differences, and its sharpness: the gradients of the model with every
operator transposed (a backward pass that kept the forward's blur order) lie far outside the GPU test's bound -- and the
host-side pieces of the gradient entry points that need no device."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _crf_grad_ref as R
import _crf_terms_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "pnp-ovss_amd", "pnp_ovss", "libpnp_hip.so")
CASE_IDS = [f"K{TR.CASES[i][0][0]}-{'+'.join(TR.CASES[i][1])}-{k}" for i, k in R.GRAD_CASES]


def test_bound_follows_the_rule():
    """Ten times the worst error measured on the MI355X, rounded up to a power of ten, and at most 1e-3."""
    assert R.WORST_MEASURED > 0
    import json
    with open(os.path.join(ROOT, "profiles", "crf_grad.json")) as f:
        errors = json.loads(f.read())["errors"]                    # written by tools/crf_bench.py --grad_errors
    assert errors["worst"] <= R.WORST_MEASURED <= 1.1 * errors["worst"]
    assert errors["bound"] == R.BOUND
    assert R.BOUND == 10.0 ** np.ceil(np.log10(10 * R.WORST_MEASURED) - 1e-9)
    assert R.BOUND <= 1e-3


@pytest.mark.parametrize("ci", range(len(TR.CASES)), ids=[f"K{c[0][0]}-" + "+".join(c[1]) for c in TR.CASES])
def test_float64_forward_equals_the_float32_reference(ci):
    shape, names, weights = TR.CASES[ci]
    _, ref_q = TR.reference(shape, names, weights)
    err = float(np.abs(R.forward(shape, names, [float(w) for w in weights]) - ref_q).max())
    print(f"{shape} {names}: float64 forward - float32 reference = {err:.2e}")
    assert err < 1e-5


@pytest.mark.parametrize("index,kinds", [c for c in R.GRAD_CASES if TR.CASES[c[0]][0] == (3, 13, 17)] + [(2, "mm"), (1, "v")],
                         ids=lambda v: str(v))
def test_autograd_agrees_with_central_differences(index, kinds):
    """Directional derivatives of sum(cotangent * Q) along random unit directions of every input, eps = 1e-5 in float64: the
    truncation error is O(eps^2) and the rounding error 1e-16 / eps of the loss, both far below 1e-6 of the derivative."""
    shape, names, compats = R.case(index, kinds)
    grad_u, grad_c = R.gradients(index, kinds)
    U, ops, cs, g = R.loss_inputs(shape, names, compats)
    rng = np.random.default_rng(5)
    inputs, grads = [U] + cs, [grad_u.reshape(shape[0], -1)] + list(grad_c)
    with torch.no_grad():
        for which, (x, gr) in enumerate(zip(inputs, grads)):
            for _ in range(3):
                d = rng.normal(size=tuple(x.shape))
                d = torch.from_numpy(np.asarray(d / np.linalg.norm(d)))
                vals = []
                for sgn in (1.0, -1.0):
                    moved = [t + sgn * 1e-5 * d if i == which else t for i, t in enumerate(inputs)]
                    vals.append(float((R.meanfield(moved[0], ops, moved[1:]) * g).sum()))
                fd = (vals[0] - vals[1]) / 2e-5
                an = float((torch.from_numpy(np.array(gr, np.float64)) * d).sum())
                scale = float(np.abs(gr).max())
                print(f"{shape} {names} {kinds} input {which}: finite difference {fd:.9e}, autograd {an:.9e}")
                assert abs(fd - an) <= 1e-6 * scale + 1e-12


@pytest.mark.parametrize("index,kinds", [c for c in R.GRAD_CASES if any(n != "d1" for n in TR.CASES[c[0]][1])], ids=CASE_IDS[1:])
def test_forward_blur_order_in_the_backward_pass_is_told_apart(index, kinds):
    """With A_t^T in place of A_t (d >= 2: the axis blurs do not commute) every gradient tensor moves by more than ten times
    the bound the GPU test holds the kernels to."""
    grad_u, grad_c = R.gradients(index, kinds)
    wrong_u, wrong_c = R.gradients(index, kinds, True)
    for name, got, ref in [("unary", wrong_u, grad_u)] + [(f"compat {t}", a, b) for t, (a, b) in enumerate(zip(wrong_c, grad_c))]:
        err = R.rel_err(got, ref)
        print(f"case {index} {kinds} {name}: wrong-order discrepancy {err:.3e}")
        assert err > 10 * R.BOUND


def test_commuting_axes_have_a_symmetric_operator():
    shape, names, _ = R.case(0, "s")
    (A,) = R.operators(shape, names)
    assert float((A - A.T).abs().max() / A.abs().max()) < 1e-12
    shape, names, _ = R.case(2, "sv")
    assert min(float((A - A.T).abs().max() / A.abs().max()) for A in R.operators(shape, names)) > 1e-2


def test_plan_terms_q_floats():
    from pnp_ovss import crf
    plan = crf.plan_terms([(13, 17), (9, 13), (23, 31)], [3, 150, 21], [2, 6])
    assert plan["Kp"] == [4, 152, 24]
    assert plan["q_floats"] == 13 * 17 * 4 + 9 * 13 * 152 + 23 * 31 * 24
    assert plan["q_floats"] == plan["qoff"][-1] + 23 * 31 * 24


def test_gradient_entry_points_refuse_a_null_solver():
    lib = ctypes.CDLL(LIB)
    p = ctypes.c_void_p(4096)
    for fn in (lib.pnp_crf_reserve_grad, lib.pnp_crf_infer_terms_saved, lib.pnp_crf_backward_terms):
        fn.restype = ctypes.c_int
    assert lib.pnp_crf_reserve_grad(None) == -22
    assert lib.pnp_crf_infer_terms_saved(None, 5, p, p, p, p, None) == -22
    assert lib.pnp_crf_backward_terms(None, 5, p, p, p, p, None, None) == -22


def test_marginals_needs_a_device():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from pnp_ovss import crf
    with pytest.raises(RuntimeError, match="needs a HIP device"):
        crf.FeatureCRF(1, 64, 64, 3)
    with pytest.raises(RuntimeError, match="marginals needs a HIP device"):
        crf.FeatureCRF.__new__(crf.FeatureCRF).marginals([torch.zeros(3, 8, 8)], [], iters=1)


def test_term_keeps_a_tensor_compatibility():
    from pnp_ovss import crf
    f = np.zeros((2, 4, 4), np.float32)
    w = torch.tensor(3.0, requires_grad=True)
    M = torch.eye(3, requires_grad=True)
    assert crf.Term([f], w).tensor is w and crf.Term([f], w).weight == 3.0 and crf.Term([f], w).kind == crf.COMPAT_SCALAR
    assert crf.Term([f], M).tensor is M and crf.Term([f], M).kind == crf.COMPAT_MATRIX
    assert crf.Term([f], 2.0).tensor is None
