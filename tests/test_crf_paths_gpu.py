"""GPU: the two owners of the DenseCRF host side (csrc/crf_solver.h) -- the engine's post-processing (post.hip) and the
stand-alone solver (crf_op.hip, pnp_ovss.crf.DenseCRF) -- give the same bits on the same problem.

1. Engine and solver.  A batch goes through the engine's merge, threshold / upsample, blur and densecrf(); the unary rows the
   engine computed, de-padded into (K, H * W) planes, and the same RGB go to DenseCRF at the engine's widths 3 / 50 / 5 and
   weights 7 / 10.  Marginals are compared as int32 bit patterns, the solver's labels through the engine's LUT with
   remap_hist(from_crf=True).
       (37,53) K = 3, (45,61) K = 21                 widest row 24 floats: narrow planes <-> rows transpose, narrow update
       ... and (29,41) K = 33                        widest row 36 floats: wide transpose, rows of 4 / 24 / 36 floats in one batch;
                                                     engine crf_chunk 0 (one launch set) and 1 (three, value offsets restarting)
   each with iters = 10 and iters = 0 (the start update alone, which then also emits the solver's labels).
2. The Gaussian lattice cache.  Three batches through one engine / one solver: the second has the sizes of the first (the
   lattice is kept) with other RGB and unaries, the third the same sizes in another order (rebuilt).  After each the results
   equal those of a fresh owner.  The solver also changes pos_xy 3 -> 2 at unchanged sizes.
3. The engine refuses an image beyond the per-image addressing of the iteration kernels (6 * H * W >= 2^24) in its host layout,
   naming the image, and then runs a small batch correctly against the oracle."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import _post_refs as R                               # noqa: E402
from test_post_ops_gpu import _assert_crf_matches, _blurred, _dev, _engine, _maxpix, _total   # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [(37, 53), (45, 61), (29, 41)]
LABELS = [3, 21, 33]


@functools.lru_cache(maxsize=None)
def _case(n_images, seed=71, order=None):
    idx = list(order) if order else list(range(n_images))
    case = R.Case([SIZES[i] for i in idx], [LABELS[i] - 1 for i in idx], [True] * len(idx), seed=seed, n_class=40)
    R.check_crf_input(case, False)
    return case


def _bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy()


def _engine_for(case, chunk):
    return _engine(case.B, _total(case), _maxpix(case), max(case.K), chunk, max_text_len=64)


def _engine_crf(e, case, iters):
    """densecrf(iters) on the blurred maps in place -> (unary planes (K, H * W) per image, concatenated; marginals (K, H * W)
    per image; labels per image), the rows de-padded."""
    e.densecrf(iters=iters)
    labels = [lab.clone() for lab in e.split_labels(e.remap_hist(True))]
    rows, planes, o = e.buffer("unary"), [], 0
    for k, (h, w) in zip(case.K, case.sizes):
        kp = (k + 3) // 4 * 4
        planes.append(rows[o:o + kp * h * w].view(h * w, kp)[:, :k].t().contiguous().reshape(-1))
        o += kp * h * w
    q = [rows_q.t().contiguous() for rows_q in e.post_q()]
    torch.cuda.synchronize()
    return torch.cat(planes), q, labels


def _assert_same(case, q_eng, lab_eng, lab_sol, q_sol, what):
    for b in range(case.B):
        np.testing.assert_array_equal(_bits(q_sol[b].reshape(case.K[b], -1)), _bits(q_eng[b]), err_msg=f"{what}: marginals of image {b}")
        lut = np.asarray(case.luts[b], dtype=np.uint8)
        np.testing.assert_array_equal(lut[lab_sol[b].cpu().numpy()], lab_eng[b].cpu().numpy(), err_msg=f"{what}: labels of image {b}")


@functools.lru_cache(maxsize=None)
def _both_paths(n_images, chunk):
    """{iters: (engine marginals, engine labels, solver labels, solver marginals)} of one batch."""
    from pnp_ovss.crf import DenseCRF
    case = _case(n_images)
    e = _engine_for(case, chunk)
    _blurred(e, case)
    solver = DenseCRF(case.B, _total(case), _maxpix(case), max(case.K))
    d_rgb = _dev(np.concatenate([r.reshape(-1) for r in case.rgb]))
    out = {}
    for iters in (10, 0):
        d_unary, q_eng, lab_eng = _engine_crf(e, case, iters)
        if not out:
            solver.set_batch(d_unary, d_rgb, case.sizes, case.K, pos_xy=3.0, bi_xy=50.0, bi_rgb=5.0)
        lab_sol, q_sol = solver.infer(iters=iters, pos_w=7.0, bi_w=10.0)
        torch.cuda.synchronize()
        out[iters] = (q_eng, lab_eng, [t.clone() for t in lab_sol], [t.clone() for t in q_sol])
    solver.close()
    e.close()
    return out


@pytest.mark.parametrize("iters", [10, 0])
@pytest.mark.parametrize("n_images,chunk", [(2, 0), (3, 0), (3, 1)], ids=["rows24", "rows36", "rows36-chunk1"])
def test_engine_and_solver_give_the_same_bits(n_images, chunk, iters):
    case = _case(n_images)
    assert max((k + 3) // 4 * 4 for k in case.K) == (24 if n_images == 2 else 36)
    _assert_same(case, *_both_paths(n_images, chunk)[iters], what=f"iters {iters}")


# ------------------------------------------------------------------------------------------ 2. the Gaussian lattice cache
def _cache_cases():
    return [_case(2, seed=72), _case(2, seed=73), _case(2, seed=74, order=(1, 0))]


def test_gaussian_cache_in_the_engine():
    cases = _cache_cases()
    e = _engine_for(cases[0], 0)
    for i, case in enumerate(cases):
        _blurred(e, case)
        _, q, lab = _engine_crf(e, case, 10)
        fresh = _engine_for(case, 0)
        _blurred(fresh, case)
        _, q_ref, lab_ref = _engine_crf(fresh, case, 10)
        fresh.close()
        for b in range(case.B):
            np.testing.assert_array_equal(_bits(q[b]), _bits(q_ref[b]), err_msg=f"batch {i}: marginals of image {b}")
            np.testing.assert_array_equal(lab[b].cpu().numpy(), lab_ref[b].cpu().numpy(), err_msg=f"batch {i}: labels of image {b}")
    e.close()


def test_gaussian_cache_in_the_solver():
    from pnp_ovss.crf import DenseCRF
    rng = np.random.default_rng(75)
    cases = _cache_cases()
    bounds = (2, _total(cases[0]), _maxpix(cases[0]), max(cases[0].K))
    solver = DenseCRF(*bounds)
    for i, (case, pos_xy) in enumerate(zip(cases + cases[2:], (3.0, 3.0, 3.0, 2.0))):
        unaries = [rng.uniform(0.1, 4.0, (k, h, w)).astype(np.float32) for k, (h, w) in zip(case.K, case.sizes)]
        lab, q = solver.run(unaries, case.rgb, pos_xy=pos_xy)
        fresh = DenseCRF(*bounds)
        lab_ref, q_ref = fresh.run(unaries, case.rgb, pos_xy=pos_xy)
        torch.cuda.synchronize()
        for b in range(case.B):
            np.testing.assert_array_equal(_bits(q[b]), _bits(q_ref[b]), err_msg=f"batch {i}: marginals of image {b}")
            np.testing.assert_array_equal(lab[b].cpu().numpy(), lab_ref[b].cpu().numpy(), err_msg=f"batch {i}: labels of image {b}")
        fresh.close()
    solver.close()


# ------------------------------------------------------------------------------------------ 3. the unaddressable image
def test_engine_refuses_an_unaddressable_image():
    H, W = 1673, 1672                                # 2 797 256 pixels: 6 n >= 2^24 from n = 2 796 203 on
    assert 6 * (H * W) >= 1 << 24 > 6 * (H * W - 1054)
    e = _engine(1, H * W, H * W, 2, 0)
    rgb = torch.zeros(3 * H * W, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match=r"\(-22\).*image 0"):
        e.post_prepare([(H, W)], [[([0], 1)]], [[0, 1]], [True], rgb=rgb, gt=None, want_crf=True)
    with pytest.raises(RuntimeError):                # nothing is prepared after a refusal
        e.blur_minmax()
    case = R.Case([(33, 45)], [1], [True], seed=76)
    R.check_crf_input(case, False)
    _blurred(e, case)
    e.densecrf()
    _assert_crf_matches(e, case)
    e.close()
