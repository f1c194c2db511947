"""GPU: operator-level tests of the post-processing half -- pipeline_kernels.hip, crf_lattice.hip / crf_meanfield.hip and the post-processing entry points
of post.hip -- against the oracle (oracle/pipeline_np.py), at the chunkings, arguments, geometries and values no other test
runs.  Cases, references and planted faults live in tests/_post_refs.py; tests/test_post_ops_cpu.py proves that they
discriminate.  Everything runs on the 8 x 8 patch grid of blip_itm_small(128) unless stated.

Stages are compared bit for bit (threshold / upsample, blur, labels, histograms, lattice point counts); DenseCRF marginals to
atol = 1e-6, the criterion of test_hip_parity.test_postprocess_stages_bit_exact_vs_oracle.  OP.bilinear_align_corners is pinned
to torch only for H + W > 128; for the smaller shapes below the oracle alone is the reference.

Which kernel branch each shape was chosen to hit:

A. chunked mean-field (crf_iterate_body, xcd_work, PostDesc.voff)
   9 images (24,40) (33,45) (40,24) (17,64) cycling, K = 2 / 3 / 5 / 21 cycling
       crf_chunk = 0: one launch set over nimg = 9 -> one full round of whole images per XCD (nimg >= 8) + one tail image in
                      8 slices; crf_chunk = 4: img0 = 0 / 4 / 8 with nimg = 4 / 4 / 1 (tail slices only), voff restarting at 0
                      in every chunk; crf_chunk = 1: img0 = 0 .. 8, nimg = 1.  Rows of 4 / 4 / 8 / 24 floats in one batch
                      (Kp differs per image), 4 / 8 / 12 / 44 in the paired run.
   2 x (48,64), K = 151      crf_update_kernel<true> (wave softmax, LDS-capped tiles), unary_wide_kernel, crf_splat_kernel<32, *, true>
                             (rows of 152 floats = 38 chunks; paired 304 floats = 76 chunks), chunked against unchunked.
   (48,64) K = 151 + (33,45) K = 3   rows of one batch differ in width: the wide kernels run over an image of one chunk per row.
B. pnp_densecrf arguments: (33,101) (200,9) (64,64), K = 3 / 5 / 2
       iters 0 (the pairwise = 0 update alone) / 1 / 3, weights (0, 10) (7, 0) (3.5, 4.25); refusal of other sigmas;
       1 x 12600 white image: bilateral key coordinate 0.0693 x + 173.7 >= 1018 leaves the 11-bit packing range ->
       lattice_embed_kernel's range flag, pnp_post_prepare's refusal and the reset of the cached Gaussian lattice.
C. edge geometries (blur_axis_kernel, upsample_kernel, lattice build), K among 2 / 3 / 6
   (9,200) (200,9)   blur radius 40 > short side 9: reflect_fast falls through to reflect_idx (up to 5 periods)
   (3,160)           radius 32, axis of 3: more than ten reflection periods
   (1,140) (140,1)   H == 1 / W == 1: sh / sw = 0 in upsample_kernel, a blur axis of one sample, lattice rows of one pixel
   (5,7)             smaller than the 8 x 8 grid (downsampling), tiles under 8 outputs wide and high, radius 1
   (33,45) (31,101)  odd H * W: every later plane / image starts at an odd float offset, W % 4 != 0 -> scalar staging, unaligned
                     row stores of the horizontal pass
   (32,64)           first in its batch: W % 4 == 0, full-width tile, aligned planes -> the 16-byte staging path; last in the
                     other batch behind odd-sized images: same shape, misaligned -> the scalar path must give the same bits
   C == 1 with scale01 (Scale_0_1 skipped on the squeezed map), has_bg False next to True in one batch.
D. value edge cases
   drop_step_kernel  PP = 64 / 441 / 2304 (1 / 2 / 9 passes of the 256-thread loops); T = 4 (empty salience sum) 5 (one row)
                     11 (7 rows: tail loop only) 12 (8 rows: exactly one unrolled block) 13 (block + 1); all-zero maps, four
                     non-zero cells, plateaus wider than npick, -0.0, NaN salience, max_picks < iters * npick
   threshold_kernel  constant non-zero map (0 / 0: all-false mask), +inf cell, NaN cell (den = NaN)
   argmax_kernel     two identical class channels: first maximum, channel-major (maps) and pixel-major (Q); the CRF's fused
                     label output on the same tie (the tied pair covers 4 x 4 grid cells, so that it still wins pixels after
                     the mean-field: test_post_ops_cpu.test_tie_case_leaves_a_tie_to_break)
   hist_kernel       n_class 21 (4 LDS copies) 60 (2) 64 (2, 8192 bins exactly) 65 (1) 91 (global atomics); gt 255 / -1 /
                     n_class / n_class - 1; predictions >= n_class land in the next row as np.bincount puts them

No image fits the range-refusal item at 64 x 64: it uses the 1 x 12600 image (2521 blur taps, below the 4096 per image the
reserve allows)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import _post_refs as R                              # noqa: E402
from pnp_ovss import config as C                    # noqa: E402
from oracle import pipeline_np as OP                # noqa: E402

pytestmark = pytest.mark.gpu

THR = R.THRESHOLD


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def _engine(max_batch, total_pix, max_pix, max_ch, chunk, max_text_len=32, img=128, reserve=True):
    from pnp_ovss.hip import Engine
    e = Engine(C.blip_itm_small(img), max_batch=max_batch, max_text_len=max_text_len, stash_layer=7, mode="f32")
    if reserve:
        e.post_reserve(max_batch, total_pix, max_pix, max_ch, chunk)
    return e


def _prepare(e, case, want_crf=True):
    e.post_prepare(case.sizes, case.plans, case.luts, case.has_bg, rgb=_dev(np.concatenate([r.reshape(-1) for r in case.rgb])),
                   gt=_dev(np.concatenate([g.reshape(-1) for g in case.gts])), want_crf=want_crf)


def _np_list(ts):
    return [t.cpu().numpy().copy() for t in ts]


def _q_single(e, case):
    """Per image (K, H, W) marginals of a single-group run."""
    return [q.cpu().numpy().T.reshape(k, h, w).copy() for q, k, (h, w) in zip(e.post_q(), case.K, case.sizes)]


def _q_pair(e, case):
    """Per image (2, K, H, W) marginals of a paired run: rows hold the two groups back to back, padded to a multiple of 4."""
    flat, out, o = e.buffer("crf_q"), [], 0
    assert flat.numel() >= sum((2 * k + 3) // 4 * 4 * h * w for k, (h, w) in zip(case.K, case.sizes)), "engine reserved one group only"
    for k, (h, w) in zip(case.K, case.sizes):
        kp = (2 * k + 3) // 4 * 4
        rows = flat[o:o + kp * h * w].view(h * w, kp)[:, :2 * k].cpu().numpy()
        out.append(rows.T.reshape(2, k, h, w).copy())
        o += kp * h * w
    return out


def _run_single_and_pair(e, case):
    """postprocess("blur+crf") of the first map set with Scale_0_1, then postprocess_pair of (first | second) map sets."""
    n = case.n_class
    d1, dn = _dev(case.maps), _dev(case.maps_n)
    h, h1, hn = (torch.zeros(n * n, device="cuda", dtype=torch.int64) for _ in range(3))
    lab = e.postprocess(d1, THR, True, "blur+crf", n, h)
    torch.cuda.synchronize()
    out = dict(lab=_np_list(e.split_labels(lab)), hist=h.cpu().numpy().copy(), q=_q_single(e, case))
    l1, ln = e.postprocess_pair(d1, dn, THR, n, h1, hn)
    torch.cuda.synchronize()
    out.update(l1=_np_list(e.split_labels(l1)), ln=_np_list(e.split_labels(ln)), h1=h1.cpu().numpy().copy(),
               hn=hn.cpu().numpy().copy(), qp=_q_pair(e, case))
    return out


def _assert_runs_identical(a, b, images=None, other_images=None):
    """Labels and marginals of run `a` (images `images`) equal those of run `b` (images `other_images`) bit for bit."""
    images = range(len(a["lab"])) if images is None else images
    other_images = images if other_images is None else other_images
    for i, j in zip(images, other_images):
        for key in ("lab", "l1", "ln", "q", "qp"):
            np.testing.assert_array_equal(a[key][i], b[key][j], err_msg=f"{key} image {i}")


def _assert_oracle(case, run, images):
    """Single run and group 0 of the pair = first map set with Scale_0_1; group 1 = second map set without."""
    for b in images:
        lab, q, _ = case.ref_crf(b, True)
        np.testing.assert_array_equal(run["lab"][b].astype(np.float32), case.remap(b, lab))
        np.testing.assert_array_equal(run["l1"][b].astype(np.float32), case.remap(b, lab))
        np.testing.assert_allclose(run["q"][b], q, rtol=0, atol=R.Q_ATOL)
        np.testing.assert_allclose(run["qp"][b][0], q, rtol=0, atol=R.Q_ATOL)
        labn, qn, _ = case.ref_crf(b, False, second=True)
        np.testing.assert_array_equal(run["ln"][b].astype(np.float32), case.remap(b, labn))
        np.testing.assert_allclose(run["qp"][b][1], qn, rtol=0, atol=R.Q_ATOL)


def _total(case):
    return sum(h * w for h, w in case.sizes)


def _maxpix(case):
    return max(h * w for h, w in case.sizes)


# ------------------------------------------------------------------------------------------ A. chunked mean-field
@pytest.fixture(scope="module")
def chunked_runs():
    case = R.case_chunked()
    R.check_crf_input(case, True)
    R.check_crf_input(case, False, second=True)
    runs = {}
    for chunk in (0, 4, 1):
        e = _engine(case.B, _total(case), _maxpix(case), max(case.K), chunk)
        _prepare(e, case)
        runs[chunk] = _run_single_and_pair(e, case)
        if chunk == 0:                               # the same engine, one image per prepared batch
            singles = []
            for b in range(case.B):
                sub = case.sub(b)
                _prepare(e, sub)
                singles.append(_run_single_and_pair(e, sub))
            runs["single"] = singles
        e.close()
    return case, runs


def test_chunked_meanfield_is_bit_identical_to_unchunked(chunked_runs):
    case, runs = chunked_runs
    for chunk in (4, 1):
        _assert_runs_identical(runs[chunk], runs[0])
        for key in ("hist", "h1", "hn"):
            np.testing.assert_array_equal(runs[chunk][key], runs[0][key], err_msg=f"{key} chunk {chunk}")
    assert runs[0]["hist"].sum() == _total(case)
    np.testing.assert_array_equal(runs[0]["hist"], runs[0]["h1"])
    assert (runs[0]["h1"] != runs[0]["hn"]).any()                     # the two groups are different problems


def test_chunked_meanfield_equals_single_image_runs(chunked_runs):
    case, runs = chunked_runs
    for chunk in (0, 4, 1):
        for b in range(case.B):
            _assert_runs_identical(runs[chunk], runs["single"][b], images=[b], other_images=[0])
    for key in ("hist", "h1", "hn"):
        np.testing.assert_array_equal(sum(s[key] for s in runs["single"]), runs[0][key])


def test_chunked_meanfield_equals_oracle(chunked_runs):
    case, runs = chunked_runs
    for chunk in (0, 4, 1):
        _assert_oracle(case, runs[chunk], range(4))


def test_chunked_meanfield_at_151_channels():
    """ade768's dispatch (crf_chunk = 1, K = 151) at 48 x 64: chunked against unchunked, single and paired, and the oracle."""
    case = R.case_wide()
    R.check_crf_input(case, True)
    R.check_crf_input(case, False, second=True)
    runs = {}
    for chunk in (0, 1):
        e = _engine(2, _total(case), _maxpix(case), 151, chunk, max_text_len=192)
        _prepare(e, case)
        runs[chunk] = _run_single_and_pair(e, case)
        e.close()
    _assert_runs_identical(runs[1], runs[0])
    for key in ("hist", "h1", "hn"):
        np.testing.assert_array_equal(runs[1][key], runs[0][key])
    _assert_oracle(case, runs[1], range(2))


def test_mixed_width_batch():
    """K = 151 next to K = 3 in one prepared batch, against single-image runs and the oracle."""
    case = R.case_mixed()
    R.check_crf_input(case, True)
    R.check_crf_input(case, False, second=True)
    e = _engine(2, _total(case), _maxpix(case), 151, 0, max_text_len=192)
    _prepare(e, case)
    run = _run_single_and_pair(e, case)
    for b in range(case.B):
        sub = case.sub(b)
        _prepare(e, sub)
        _assert_runs_identical(run, _run_single_and_pair(e, sub), images=[b], other_images=[0])
    e.close()
    _assert_oracle(case, run, range(2))


# ------------------------------------------------------------------------------------------ B. pnp_densecrf arguments
@pytest.fixture(scope="module")
def args_engine():
    case = R.case_args()
    e = _engine(3, max(_total(case), R.RANGE_W), max(_maxpix(case), R.RANGE_W), 8, 0)
    yield e
    e.close()


def _blurred(e, case, scale01=False):
    _prepare(e, case)
    e.merge_tokens(_dev(case.maps))
    e.threshold_upsample(THR, scale01)
    e.blur_minmax()


def _assert_crf_matches(e, case, scale01=False, **kw):
    labels = e.split_labels(e.remap_hist(True))
    torch.cuda.synchronize()
    qs = _q_single(e, case)
    for b in range(case.B):
        lab, q, _ = case.ref_crf(b, scale01, **kw)
        np.testing.assert_array_equal(labels[b].cpu().numpy().astype(np.float32), case.remap(b, lab), err_msg=f"image {b} {kw}")
        np.testing.assert_allclose(qs[b], q, rtol=0, atol=R.Q_ATOL, err_msg=f"image {b} {kw}")


@pytest.mark.parametrize("kw", R.CRF_ARGS, ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_densecrf_arguments_vs_oracle(args_engine, kw):
    case = R.case_args()
    R.check_crf_input(case, False)
    _blurred(args_engine, case)
    args_engine.densecrf(**kw)
    _assert_crf_matches(args_engine, case, **kw)


def test_densecrf_refuses_other_sigmas(args_engine):
    case = R.case_args()
    _blurred(args_engine, case)
    for kw in (dict(pos_xy=2.0), dict(bi_xy=40.0), dict(bi_rgb=4.0)):
        with pytest.raises(RuntimeError, match=r"\(-22\)"):
            args_engine.densecrf(**kw)
    args_engine.densecrf()
    _assert_crf_matches(args_engine, case)


def test_lattice_key_range_refusal_drops_the_gaussian_cache(args_engine):
    """A prepare that is refused for a key out of the packing range has already rebuilt the Gaussian lattice for ITS sizes.
    The next batch has the sizes of the batch prepared before the refusal: a cache that still named those sizes would skip
    the rebuild and run on the refused batch's lattice."""
    e = args_engine
    case = R.case_args()
    _blurred(e, case)
    e.densecrf()
    _assert_crf_matches(e, case)
    bad = R.Case([(1, R.RANGE_W)], [1], [True], seed=3)
    bad.rgb = [np.full((1, R.RANGE_W, 3), 255, dtype=np.uint8)]
    assert R.bilateral_key_extent(R.RANGE_W - 1, 0, (255, 255, 255)) - 12 >= R.KEY_LIMIT
    with pytest.raises(RuntimeError, match="packing range"):
        _prepare(e, bad)
    with pytest.raises(RuntimeError):                # nothing is prepared after a refusal
        e.blur_minmax()
    again = R.Case(case.sizes, case.n_cls, case.has_bg, seed=41)
    R.check_crf_input(again, False)
    _blurred(e, again)
    e.densecrf()
    _assert_crf_matches(e, again)


# ------------------------------------------------------------------------------------------ C. edge geometries
@pytest.fixture(scope="module")
def edge_engine():
    cases = [R.case_edge(n) for n in R.EDGE_BATCHES]
    e = _engine(5, max(_total(c) for c in cases), max(_maxpix(c) for c in cases), 8, 0)
    yield e
    e.close()


@pytest.mark.parametrize("scale01", [True, False])
@pytest.mark.parametrize("name", sorted(R.EDGE_BATCHES))
def test_edge_geometries_every_stage_vs_oracle(edge_engine, name, scale01):
    e, case = edge_engine, R.case_edge(name)
    R.check_crf_input(case, scale01)
    _prepare(e, case)
    e.merge_tokens(_dev(case.maps))
    e.threshold_upsample(THR, scale01)
    torch.cuda.synchronize()
    pre = _np_list(e.post_maps("maps_pre_blur"))
    for b in range(case.B):
        np.testing.assert_array_equal(pre[b], case.ref_pre(b, scale01), err_msg=f"pre-blur {case.sizes[b]}")
    e.blur_minmax()
    torch.cuda.synchronize()
    blurred = _np_list(e.post_maps("maps"))
    for b in range(case.B):
        np.testing.assert_array_equal(blurred[b], case.ref_blur(b, scale01), err_msg=f"blur {case.sizes[b]}")
    hist = torch.zeros(21 * 21, device="cuda", dtype=torch.int64)
    labels = e.split_labels(e.remap_hist(False, 21, hist))
    torch.cuda.synchronize()
    ref_labels = [case.remap(b, np.argmax(case.ref_blur(b, scale01), axis=0).astype(np.float32)) for b in range(case.B)]
    for b in range(case.B):
        np.testing.assert_array_equal(labels[b].cpu().numpy().astype(np.float32), ref_labels[b], err_msg=f"labels {case.sizes[b]}")
    np.testing.assert_array_equal(hist.cpu().numpy().reshape(21, 21), OP.scores(case.gts, ref_labels, 21)[1].astype(np.int64))
    e.densecrf()
    _assert_crf_matches(e, case, scale01)
    idg = e.buffer("crf_idbase_gauss", torch.int32)[: case.B + 1].cpu().numpy()
    idb = e.buffer("crf_idbase_bilateral", torch.int32)[: case.B + 1].cpu().numpy()
    for b in range(case.B):
        stats = case.ref_crf(b, scale01)[2]
        assert (idg[b + 1] - idg[b], idb[b + 1] - idb[b]) == (stats[0], stats[1]), case.sizes[b]


# ------------------------------------------------------------------------------------------ D. drop step
@pytest.fixture(scope="module", params=[128, 336, 768])
def drop_engine(request):
    e = _engine(2, 0, 0, 0, 0, img=request.param, reserve=False)
    yield e
    e.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _drive_drop_step(e, gs, max_picks, npick=10):
    B, T, P, _ = gs[0].shape
    g0 = torch.full((B, T, P, P), 7.0, device="cuda")
    agg = torch.full((B, T, P, P), 7.0, device="cuda")
    dropped = torch.zeros(B, P * P, device="cuda", dtype=torch.uint8)
    guard = torch.full((64 + B * max_picks + 64,), -7, device="cuda", dtype=torch.int32)
    picks = guard[64:64 + B * max_picks].view(B, max_picks)
    picks.fill_(-1)
    for it, g in enumerate(gs):
        e.drop_step(_dev(g), g0, agg, dropped, picks, it, npick)
    torch.cuda.synchronize()
    guard = guard.cpu().numpy()
    assert (guard[:64] == -7).all() and (guard[64 + B * max_picks:] == -7).all()
    return g0.cpu().numpy(), agg.cpu().numpy(), dropped.cpu().numpy(), picks.cpu().numpy()


@pytest.mark.parametrize("T", [4, 5, 11, 12, 13])
def test_drop_step_value_edges_vs_oracle(drop_engine, T):
    e = drop_engine
    P = e.grid
    for kind in R.DROP_INPUTS:
        gs = R.drop_maps(kind, P, T)
        for max_picks in (30, 14):                   # 14 < 3 * 10: slots past it are neither written nor flagged
            ref = R.drop_reference(gs, max_picks=max_picks)
            got = _drive_drop_step(e, gs, max_picks)
            for name, g, r in zip(("g0", "agg", "dropped", "picks"), got, ref):
                if kind == "nan" or g.dtype != np.float32:
                    np.testing.assert_array_equal(g, r, err_msg=f"{name} {kind} PP={P * P} T={T} max_picks={max_picks}")
                else:                                # -0.0 and 0.0 told apart
                    assert np.array_equal(_bits(g), _bits(r)), f"{name} {kind} PP={P * P} T={T} max_picks={max_picks}"


# ------------------------------------------------------------------------------------------ D. threshold / minmax / background / argmax
@pytest.fixture(scope="module")
def value_engine():
    e = _engine(2, 33 * 45 + 17 * 64, 33 * 45, 8, 0)
    yield e
    e.close()


@pytest.mark.parametrize("kind", ["constant", "inf", "nan"])
def test_threshold_value_edges_vs_oracle(value_engine, kind):
    """A constant class map thresholds to all-false (0 / 0), +inf and NaN cells poison their own channel: maps with equal NaN
    positions, and the labels of the blur-free and the "blur" mode equal to the oracle's."""
    e, case = value_engine, R.value_case(kind)
    _prepare(e, case, want_crf=False)
    e.merge_tokens(_dev(case.maps))
    e.threshold_upsample(THR, False)
    torch.cuda.synchronize()
    pre = _np_list(e.post_maps("maps_pre_blur"))
    with np.errstate(all="ignore"):
        for b in range(case.B):
            ref = case.ref_pre(b, False)
            np.testing.assert_array_equal(np.isnan(pre[b]), np.isnan(ref))
            np.testing.assert_array_equal(pre[b], ref)
        if kind != "constant":
            assert np.isnan(case.ref_pre(0, False)).any() and not np.isnan(case.ref_pre(1, False)).any()
        else:
            assert (case.ref_pre(0, False)[1] == 0).all()
        for mode in (None, "blur"):
            labels = e.split_labels(e.postprocess(_dev(case.maps), THR, False, mode))
            torch.cuda.synchronize()
            for b in range(case.B):
                lab = OP.postprocess(mode, case.ref_pre(b, False), None, case.sizes[b])
                np.testing.assert_array_equal(labels[b].cpu().numpy().astype(np.float32), case.remap(b, lab), err_msg=f"{mode} {b}")


def test_argmax_ties_take_the_first_maximum(value_engine):
    """Two identical class channels tie exactly in the maps and in the CRF marginals: channel-major argmax (remap_hist(False)),
    pixel-major argmax (remap_hist(True)) and the label output fused into the last CRF update all take the first."""
    e, case = value_engine, R.value_case("tie")
    R.check_crf_input(case, False)
    _prepare(e, case)
    labels = e.split_labels(e.postprocess(_dev(case.maps), THR, False, None))
    torch.cuda.synchronize()
    for b in range(case.B):
        pre = case.ref_pre(b, False)
        np.testing.assert_array_equal(pre[1], pre[2])
        assert (pre[1] > 0).any()
        lab = np.argmax(pre, axis=0).astype(np.float32)
        assert not (lab == 2).any()
        np.testing.assert_array_equal(labels[b].cpu().numpy().astype(np.float32), case.remap(b, lab))
    d = _dev(case.maps)
    sep = _np_list(e.split_labels(e.postprocess(d, THR, False, "blur+crf")))          # pnp_densecrf + a separate argmax over Q
    torch.cuda.synchronize()
    qs = _q_single(e, case)
    f1, fn = e.postprocess_pair(d, d, THR, scale01=(False, False))                      # labels written by the last update
    torch.cuda.synchronize()
    f1, fn = _np_list(e.split_labels(f1)), _np_list(e.split_labels(fn))
    for b in range(case.B):
        lab, q, _ = case.ref_crf(b, False)
        np.testing.assert_array_equal(qs[b][1], qs[b][2])                             # the tie survives the mean-field
        assert (lab == 1).any() and not (lab == 2).any()
        for got in (sep[b], f1[b], fn[b]):
            np.testing.assert_array_equal(got.astype(np.float32), case.remap(b, lab))


# ------------------------------------------------------------------------------------------ D. confusion histogram
@pytest.mark.parametrize("n_class", [21, 60, 64, 65, 91])
def test_confusion_hist_bin_layouts_and_ignore_labels(value_engine, n_class):
    e = value_engine
    sizes, K, lut, idx, gts = R.hist_case(n_class, n_class)
    case = R.Case(sizes, [K, K], [False, False], seed=61)
    case.luts, case.gts = [lut, lut], gts
    _prepare(e, case, want_crf=False)
    e.merge_tokens(_dev(case.maps))
    e.threshold_upsample(THR, False)                 # the maps now live in "maps_pre_blur": overwrite them with one-hot planes
    onehot = np.concatenate([(np.arange(K)[:, None, None] == ix[None]).astype(np.float32).reshape(-1) for ix in idx])
    e.buffer("maps_pre_blur")[: onehot.size].copy_(_dev(onehot))
    hist = torch.zeros(n_class * n_class, device="cuda", dtype=torch.int64)
    ref = R.hist_reference(gts, idx, lut, n_class)
    for rep in (1, 2):                               # accumulated over two calls into the same buffer
        labels = e.split_labels(e.remap_hist(False, n_class, hist))
        torch.cuda.synchronize()
        for b in range(2):
            np.testing.assert_array_equal(labels[b].cpu().numpy(), np.asarray(lut, dtype=np.uint8)[idx[b]])
        np.testing.assert_array_equal(hist.cpu().numpy().reshape(n_class, n_class), rep * ref)
