"""CPU: proof that the cases of tests/_post_refs.py discriminate (each proof uses the oracle alone), that every CRF input
passes the input rule, and the argument refusals of the post-processing entry points that sit in front of the first HIP call.

pnp_densecrf's refusal of non-default sigmas needs a prepared engine, so it is checked on the GPU only."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import _post_refs as R                              # noqa: E402
from oracle import pipeline_np as OP                # noqa: E402

ERR_ARG = -22


# ------------------------------------------------------------------------------------------ blur at thin shapes
@pytest.mark.parametrize("shape", R.THIN_SHAPES + [(33, 101)])
def test_oracle_blur_equals_scipy_at_thin_shapes(shape):
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    x = rng.random(shape, dtype=np.float32)
    sigma = 0.05 * max(shape)
    np.testing.assert_array_equal(OP.gaussian_blur(x, sigma), ndi.gaussian_filter(x, sigma))


@pytest.mark.parametrize("shape", [(9, 200), (200, 9), (3, 160), (1, 140), (140, 1)])
def test_single_reflection_differs_at_every_thin_shape(shape):
    """The blur radius int(0.2 * max(H, W) + 0.5) exceeds the short side at each of these shapes: folding the index once (the
    kernel's fast path alone) gives another result than the multi-period reflection.  A length-1 axis holds one sample, so
    there every fold lands on it and only "stays in bounds" is left to go wrong: the two agree."""
    rng = np.random.default_rng(7)
    sigma = 0.05 * max(shape)
    assert OP.gaussian_kernel1d(sigma)[1] >= min(shape)
    x = rng.random(shape, dtype=np.float32)
    if min(shape) == 1:
        np.testing.assert_array_equal(R.blur_single_reflection(x, sigma), OP.gaussian_blur(x, sigma))
    else:
        assert np.abs(R.blur_single_reflection(x, sigma) - OP.gaussian_blur(x, sigma)).max() > 1e-3


def test_single_reflection_equals_oracle_where_one_fold_suffices():
    x = np.random.default_rng(1).random((64, 48), dtype=np.float32)
    np.testing.assert_array_equal(R.blur_single_reflection(x, 0.05 * 64), OP.gaussian_blur(x, 0.05 * 64))


# ------------------------------------------------------------------------------------------ CRF inputs
@pytest.mark.parametrize("case,scale01", [("chunked", True), ("chunked", False), ("wide", True), ("wide", False), ("mixed", True),
                                          ("mixed", False), ("args", False), ("odd_first", True), ("odd_first", False),
                                          ("aligned_first", True), ("aligned_first", False)])
def test_every_crf_input_passes_the_input_rule(case, scale01):
    c = R.case_edge(case) if case in R.EDGE_BATCHES else getattr(R, "case_" + case)()
    R.check_crf_input(c, scale01)
    if case in ("chunked", "wide", "mixed"):
        R.check_crf_input(c, scale01, second=True)


def test_careless_random_maps_break_the_input_rule():
    """What the rule is there for: dense random maps leave no background pixel, the channel blurs to 0 / 0."""
    c = R.Case([(9, 200)], [3], [True], seed=1)
    c.maps[0, 3:6] = np.random.default_rng(0).random((3, 8, 8), dtype=np.float32) + np.float32(0.5)
    with pytest.raises(AssertionError):
        R.check_crf_input(c, False)


def test_edge_batches_hold_the_geometries_they_name():
    odd, ali = R.case_edge("odd_first"), R.case_edge("aligned_first")
    off = np.cumsum([0] + [k * h * w for k, (h, w) in zip(odd.K, odd.sizes)])
    assert odd.sizes[-1] == (32, 64) and off[-2] % 2 == 1            # the aligned shape sits at an odd float offset
    assert ali.sizes[0] == (32, 64)                                   # ... and at offset 0 here
    assert {2, 3, 6} <= set(odd.K) | set(ali.K)
    shapes = set(odd.sizes) | set(ali.sizes)
    assert {(9, 200), (200, 9), (3, 160), (1, 140), (140, 1), (5, 7), (33, 45), (31, 101), (32, 64)} <= shapes


def test_tie_case_leaves_a_tie_to_break():
    """The two tied channels stay bit-equal through the oracle's mean-field and still win pixels after it, in the maps and in
    the marginals; "last maximum wins" labels exactly those pixels differently, and the LUT keeps the two ids apart."""
    c = R.value_case("tie")
    R.check_crf_input(c, False)
    for b in range(c.B):
        pre = c.ref_pre(b, False)
        lab, q, _ = c.ref_crf(b, False)
        for m, first in ((pre, np.argmax(pre, axis=0)), (q, lab)):
            np.testing.assert_array_equal(m[1], m[2])
            last = m.shape[0] - 1 - np.argmax(m[::-1], axis=0)
            assert (first == 1).any() and not (first == 2).any()
            np.testing.assert_array_equal(last != first, first == 1)
            assert (c.remap(b, last.astype(np.float32)) != c.remap(b, first.astype(np.float32))).any()


# ------------------------------------------------------------------------------------------ CRF arguments
def test_crf_arguments_change_labels_and_marginals():
    """Results at iters = k and k + 1, and at each altered weight pair, differ from each other in labels and by more than
    100 x the marginal tolerance somewhere: a kernel that ignored an argument would miss the oracle."""
    c = R.case_args()
    b = 2                                                             # the 64 x 64 image
    res = {}
    for iters in (0, 1, 2, 3, 4, 10):
        res[("it", iters)] = c.ref_crf(b, False, iters=iters)
    for kw in R.CRF_ARGS[3:]:
        res[("w", kw["pos_w"], kw["bi_w"])] = c.ref_crf(b, False, **kw)
    pairs = [(("it", k), ("it", k + 1)) for k in (0, 1, 2, 3)]
    keys = [("it", 10)] + [k for k in res if k[0] == "w"]
    pairs += [(keys[i], keys[j]) for i in range(len(keys)) for j in range(i + 1, len(keys))]
    for a, d in pairs:
        (la, qa, _), (ld, qd, _) = res[a], res[d]
        assert (la != ld).any(), (a, d)
        assert np.abs(qa - qd).max() > 100 * R.Q_ATOL, (a, d)


# ------------------------------------------------------------------------------------------ drop step
def test_drop_reference_equals_the_oracle_drop_loop():
    from pnp_ovss import config as C
    cfg = C.blip_itm_small(128)
    for kind in R.DROP_INPUTS:
        if kind == "nan":
            continue                                                   # (the oracle's loop is the same code path; NaN != NaN below)
        gs = R.drop_maps(kind, cfg.grid, 12)
        it = iter(gs)
        imgs = np.ones((2, 3, cfg.img_size, cfg.img_size), dtype=np.float32)
        g0, agg, picks = OP.drop_loop(None, cfg, imgs, None, None, 3, 7, 9, gradcam_fn=lambda x: next(it))
        r0, ragg, _, rp = R.drop_reference(gs)
        np.testing.assert_array_equal(g0, r0)
        np.testing.assert_array_equal(agg, ragg)
        for i in range(3):
            for b in range(2):
                assert picks[i][b] == list(rp[b, 10 * i:10 * i + 10])


def test_select_topk_nan_rule():
    assert OP.select_topk(np.array([0, np.nan, 3, 3, 0, np.nan, 1], dtype=np.float32), [], 3) == [3, 1, 5]


@pytest.mark.parametrize("P", [8, 21, 48])
@pytest.mark.parametrize("T", [4, 5, 11, 12, 13])
def test_tie_and_nan_cases_discriminate(P, T):
    """Every tie input's picks change under "smaller index wins"; the NaN input's picks change under "NaN smallest"."""
    for kind in ("zeros", "four_cells", "plateaus", "neg_zero"):
        gs = R.drop_maps(kind, P, T)
        ref = R.drop_reference(gs)[3]
        assert (R.drop_reference(gs, topk=R.topk_smaller_index_wins)[3] != ref).any(), kind
    if T > 4:                                                          # T = 4: the salience sum is empty, no NaN reaches it
        gs = R.drop_maps("nan", P, T)
        assert np.isnan(gs[0][1]).sum() == 2 and not np.isnan(gs[0][0]).any()
        ref = R.drop_reference(gs)[3]
        assert (R.drop_reference(gs, topk=R.topk_nan_smallest)[3] != ref).any()
        assert (R.drop_reference(gs, topk=R.topk_smaller_index_wins)[3] != ref).any()


def test_zero_maps_repick_the_last_ten_cells():
    ref = R.drop_reference(R.drop_maps("zeros", 8, 12))[3]
    for it in range(3):
        assert list(ref[0, 10 * it:10 * it + 10]) == list(range(54, 64))


def test_max_picks_truncation_of_the_reference():
    gs = R.drop_maps("plateaus", 8, 12)
    full = R.drop_reference(gs)
    cut = R.drop_reference(gs, max_picks=14)
    np.testing.assert_array_equal(cut[3], full[3][:, :14])           # the same picks while the slots last ...
    assert cut[2].sum() == 2 * 14 and full[2].sum() == 2 * 30        # ... and nothing flagged past them


# ------------------------------------------------------------------------------------------ histogram
@pytest.mark.parametrize("n_class", [21, 60, 64, 65, 91])
def test_histogram_case_discriminates(n_class):
    sizes, K, lut, idx, gts = R.hist_case(n_class, n_class)
    ref = R.hist_reference(gts, idx, lut, n_class)
    allg = np.concatenate([g.ravel() for g in gts])
    for v in (255, -1, n_class, n_class - 1):
        assert (allg == v).any()
    assert sum(1 for v in lut if v >= n_class) == 2
    same = R.hist_reference(gts, idx, lut, n_class, ignore_rule=lambda g, n: (g >= 0) & (g < n))
    np.testing.assert_array_equal(same, ref)
    for rule in (lambda g, n: (g >= 0) & (g <= n), lambda g, n: (g > 0) & (g < n), lambda g, n: (g >= 0) & (g < n - 1),
                 lambda g, n: (g >= -1) & (g < n)):
        assert (R.hist_reference(gts, idx, lut, n_class, ignore_rule=rule) != ref).any()
    # predictions >= n_class are counted (in the next row, as np.bincount does), not dropped
    preds = np.concatenate([np.asarray(lut)[ix].ravel() for ix in idx])
    valid = (allg >= 0) & (allg < n_class)
    assert ref.sum() == valid.sum() and (preds[valid] >= n_class).any()


# ------------------------------------------------------------------------------------------ lattice key range
def test_bilateral_key_extent_rule():
    """The 1 x W image of the range-refusal test leaves the 11-bit packing range, ordinary images stay far inside."""
    assert R.bilateral_key_extent(63, 63, (255, 255, 255)) < R.KEY_LIMIT // 4
    assert R.bilateral_key_extent(199, 8, (255, 255, 255)) < R.KEY_LIMIT // 4
    W = R.RANGE_W
    assert R.bilateral_key_extent(W - 1, 0, (255, 255, 255)) - 2 * 6 >= R.KEY_LIMIT     # whatever the canonical offsets are
    assert int(0.2 * W + 0.5) + 1 <= 4096                                               # blur taps of the image fit one image's share


# ------------------------------------------------------------------------------------------ argument refusals
@pytest.fixture(scope="module")
def lib():
    from pnp_ovss import hip
    return hip.load_library()


@pytest.fixture()
def handle(lib):
    """An engine handle that never touched a device: pnp_create refuses patch != 16 before its first HIP call and leaves
    the handle (for pnp_last_error) to the caller."""
    from pnp_ovss import hip, config as C
    cfg = C.blip_itm_small(128)
    c = hip.PnpConfig(cfg.img_size, 15, cfg.vit_dim, cfg.vit_depth, cfg.vit_heads, cfg.vit_mlp_ratio, cfg.vit_ln_eps,
                      cfg.txt_hidden, cfg.txt_layers, cfg.txt_heads, cfg.txt_inter, cfg.txt_ln_eps, cfg.vocab, cfg.max_pos,
                      cfg.enc_token_id, 2, 32, 7, 0, 0)
    h = ctypes.c_void_p()
    assert lib.pnp_create(ctypes.byref(c), ctypes.byref(h)) == ERR_ARG and h.value
    assert b"patch" in lib.pnp_last_error(h)
    yield h
    lib.pnp_destroy(h)


def test_drop_step_refusals_without_a_gpu(lib, handle):
    buf = ctypes.create_string_buffer(64)
    p, n = ctypes.c_void_p(ctypes.addressof(buf)), None
    ds = lib.pnp_drop_step
    assert ds(n, p, p, p, p, p, 0, 1, 12, 10, 30, n) == ERR_ARG                     # no engine
    assert ds(handle, n, p, p, p, p, 0, 1, 12, 10, 30, n) == ERR_ARG                # no map
    assert ds(handle, p, p, n, p, p, 0, 1, 12, 10, 30, n) == ERR_ARG                # no aggregate
    assert ds(handle, p, p, p, n, p, 0, 1, 12, 10, 30, n) == ERR_ARG                # no dropped mask
    assert ds(handle, p, p, p, p, n, 0, 1, 12, 10, 30, n) == ERR_ARG                # picks wanted, no pick list
    for T in (3, 0, -1):
        assert ds(handle, p, p, p, p, p, 0, 1, T, 10, 30, n) == ERR_ARG
        assert b"too short" in lib.pnp_last_error(handle)


def test_post_reserve_bounds_without_a_gpu(lib, handle):
    pr = lib.pnp_post_reserve
    assert pr(None, 1, 100, 100, 4, 0) == ERR_ARG
    for args in ((0, 100, 100, 4), (65, 100, 100, 4), (-1, 100, 100, 4), (1, 0, 100, 4), (1, 100, 0, 4), (1, 100, 100, 0),
                 (1, 100, 100, 256), (1, -5, 100, 4)):
        assert pr(handle, *args, 0) == ERR_ARG, args
        assert b"bad post-process bounds" in lib.pnp_last_error(handle)
    # the stage calls refuse an engine nobody prepared (PNP_ERR_STATE), again before any HIP call
    assert lib.pnp_blur_minmax(handle, None) not in (0, ERR_ARG)
    assert lib.pnp_densecrf(handle, 10, 7.0, 3.0, 10.0, 50.0, 5.0, None) not in (0, ERR_ARG)
    assert lib.pnp_post_prepare(handle, None, 1, None) == ERR_ARG
