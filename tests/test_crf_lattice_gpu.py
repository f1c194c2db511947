"""GPU: the DenseCRF lattice stage by stage (tests/_crf_lattice_checks.py; inputs and checkers are proven in
test_crf_lattice_cpu.py).  What a lattice build leaves on the device -- barycentric weights, ids, neighbour tables, two-axis
neighbour records, contributor lists, numbering, normaliser (pnp_crf_lattice_view_get) -- and the value rows after the splat, the
forward blur, the reverse blur and the slice of one filter pass on seeded rows (pnp_crf_probe_filter: the mean-field's own
kernels and dispatch) equal tests/_crf_general_ref.Lattice, the numpy restatement of oracle/densecrf_ref.c, BIT FOR BIT, through
the id bijection the first check establishes.  Equality is the contract: the kernels' comments state the order of every
operation (contributors in ascending pixel order, one rounding per axis element, vertices in order in the slice).

  feature path  D = 1 .. 6 (keys of 16 / 16 / 16 / 16 / 12 / 10 bits per coordinate, no image bits), one batch of four images:
                the runs image twice (identical keys in adjacent images), the smooth image (negative keys), a line of 7 pixels
  three terms   2, 6 and 3 axes in one solver: lattices allocated for the widest term, value buffers shared in turn
  dispatch      the same batch at K = 59, 100, 151: splat with 16 / 32 lanes per point and the multi-pass form (38 chunks)
  limit         keys within 8 of the edge of the 12- and 10-bit fields
  two terms     the nine images of tests/_crf_rows.py on the Gaussian (D = 2) and bilateral (D = 5) lattices, keys with image bits
  independence  an image of a batch, made local, equals the image prepared alone
  sort          the radix sort over 16, 48, 60 and all 64 key bits (the D = 4 key uses all 64)"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import _crf_general_ref as G                       # noqa: E402
import _crf_lattice_checks as LC                   # noqa: E402
import _crf_rows as CR                             # noqa: E402
from _gpu_guard import Guarded                     # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
PNP_ERR_STATE, PNP_ERR_ARG = -1, -22
SIZES = [LC.RUNS_SIZE, LC.RUNS_SIZE, LC.SMOOTH_SIZE, LC.LINE_SIZE]
BUILD = ("embed", "neighbours", "nbr8", "lists", "numbering", "norm")
FILTER = ("splat", "forward", "reverse", "slice")


def _feature_solver(feats, K, *more):
    """A FeatureCRF with one term over `feats` -- per image (D, H, W) -- and one over each of `more`, and zero unary energies of K
    labels; the batch is set."""
    from pnp_ovss import crf
    terms = [feats] + list(more)
    dims, sizes = [t[0].shape[0] for t in terms], [f.shape[1:] for f in feats]
    pix = [h * w for h, w in sizes]
    solver = crf.FeatureCRF(len(feats), sum(pix), max(pix), K, max_terms=len(terms), max_dims=max(dims))
    d_unary = torch.zeros(K * sum(pix), dtype=torch.float32, device=solver.device)
    d_feat = [torch.from_numpy(np.concatenate([np.ascontiguousarray(f).reshape(-1) for f in t])).to(solver.device) for t in terms]
    solver.set_batch(d_unary, d_feat, dims, sizes, [K] * len(feats))
    return solver


def _probe(solver, term, stage, planes, idbase, tag):
    """pnp_crf_probe_filter into a guarded buffer of exactly the floats the stage writes: NaN before, guards intact and no NaN
    after.  -> per image (M_b, K) rows, or (K, H * W) planes for the slice."""
    K = planes[0].shape[0]
    counts = np.diff(idbase.astype(np.int64))
    need = sum(p.size for p in planes) if stage == "slice" else int(counts.sum()) * K
    out = Guarded((need,), torch.float32, guard=4 * K)
    d_in = torch.from_numpy(np.concatenate([p.reshape(-1) for p in planes])).to(solver.device)
    solver.probe_filter(term, stage, d_in, out=out.live)
    torch.cuda.synchronize()
    flat = out.check(f"{tag}/{stage}").numpy()
    cuts = np.cumsum([p.size for p in planes] if stage == "slice" else counts * K)[:-1]
    return [part.reshape(K, -1) if stage == "slice" else part.reshape(-1, K) for part in np.split(flat, cuts)]


def _check_term(solver, term, refs, sizes, K, seed, tag, build=BUILD, stages=FILTER):
    """The build stages `build` and the filter stages `stages` of one term of the batch that is set."""
    dev = solver.lattice_arrays(term)
    points = int(solver.lib.pnp_crf_lattice_points(solver.h, term))
    assert dev["points"] == points and dev["D1"] == refs[0].d + 1
    maps = LC.check_build(dev, refs, sizes, points=points, stages=build)
    if not stages:
        return dev
    planes = LC.probe_rows(sizes, K, seed)
    want = [LC.reference_stages(r, p) for r, p in zip(refs, planes)]
    for stage in stages:
        got = _probe(solver, term, stage, planes, dev["idbase"], tag)
        LC.check_rows(stage, got, [w[stage] for w in want], maps)
    return dev


@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 6])
def test_feature_path_every_stage_equals_the_reference(D):
    solver = _feature_solver(LC.batch_images(D), 5)
    try:
        dev = _check_term(solver, 0, LC.batch_lattices(D), SIZES, 5, seed=10 + D, tag=f"features D={D}")
        # identical images side by side: the same lattice twice, apart from the ids' base
        a, b = LC.image_local(dev, SIZES, 0), LC.image_local(dev, SIZES, 1)
        for k in a:
            np.testing.assert_array_equal(np.asarray(a[k]), np.asarray(b[k]), err_msg=f"images 0 and 1 differ in {k}")
    finally:
        solver.close()


def test_terms_of_different_dimensions_in_one_solver():
    """Three terms of 2, 6 and 3 axes: every lattice is allocated for the widest term's 7 points per pixel (the stride of the
    axis tables) while each runs with its own d + 1, and the terms take turns in one pair of value buffers."""
    dims = (2, 6, 3)
    solver = _feature_solver(LC.batch_images(2), 5, LC.batch_images(6), LC.batch_images(3))
    try:
        assert solver.lattice_points() == [sum(r.M for r in LC.batch_lattices(D)) for D in dims]
        for term, D in enumerate(dims):
            dev = _check_term(solver, term, LC.batch_lattices(D), SIZES, 5, seed=40 + term, tag=f"three terms, term {term} D={D}")
            assert dev["cap"] == 7 * sum(h * w for h, w in SIZES)
    finally:
        solver.close()


@pytest.mark.parametrize("K", [59, 100, 151])
@pytest.mark.parametrize("D", [1, 3, 6])
def test_every_splat_dispatch_equals_the_reference(D, K):
    solver = _feature_solver(LC.batch_images(D), K)
    try:
        _check_term(solver, 0, LC.batch_lattices(D), SIZES, K, seed=100 * D + K, tag=f"dispatch D={D} K={K}", build=("embed",),
                    stages=("splat", "forward", "slice"))
    finally:
        solver.close()


@pytest.mark.parametrize("D", [5, 6])
def test_keys_at_the_edge_of_the_key_field(D):
    solver = _feature_solver([LC.limit_image(D)], 2)
    try:
        _check_term(solver, 0, [LC._lattice("limit", D)], [LC.RUNS_SIZE], 2, 0, f"limit D={D}", build=("embed", "neighbours", "lists"),
                    stages=())
    finally:
        solver.close()


_TWO_TERM_REFS = {}


def _two_term_refs():
    if not _TWO_TERM_REFS:
        pairs = [G.features(rgb, 3, 50, 5) for rgb in CR.case(3).rgb]
        _TWO_TERM_REFS[0] = [G.Lattice(fg) for fg, _ in pairs]
        _TWO_TERM_REFS[1] = [G.Lattice(fb) for _, fb in pairs]
    return _TWO_TERM_REFS


@pytest.mark.parametrize("K", [3, 59])
def test_two_term_solver_every_stage_equals_the_reference(K):
    """The Gaussian (D = 2) and bilateral (D = 5) lattices of pnp_crf_set_batch, keys with the image index above the coordinates,
    on nine images: one round of whole images per XCD and a tail image in eight slices."""
    from pnp_ovss import crf
    case, refs = CR.case(K), _two_term_refs()
    sizes = [tuple(s) for s in case.sizes]
    pix = [h * w for h, w in sizes]
    solver = crf.DenseCRF(len(sizes), sum(pix), max(pix), K)
    try:
        unaries = [np.zeros((K, h, w), F32) for h, w in sizes]
        d_unary, d_rgb, _, labels = solver._gather(unaries, case.rgb)
        solver.set_batch(d_unary, d_rgb, sizes, labels, pos_xy=3.0, bi_xy=50.0, bi_rgb=5.0)
        before = solver.allocated_bytes()
        for term in (0, 1):
            _check_term(solver, term, refs[term], sizes, K, seed=7 * K + term, tag=f"two-term K={K} term={term}")
        assert 0 < solver.allocated_bytes() - before <= 64 * 1024      # the descriptors of the bilateral probe, once
    finally:
        solver.close()


def test_an_image_of_a_batch_equals_the_image_prepared_alone():
    D = 4                                                     # the key that uses all 64 bits
    batch = _feature_solver(LC.batch_images(D), 5)
    alone = _feature_solver([LC.smooth_image(D)], 5)
    try:
        a = LC.image_local(batch.lattice_arrays(0), SIZES, 2)
        b = LC.image_local(alone.lattice_arrays(0), [LC.SMOOTH_SIZE], 0)
        assert len(a["seg_lo"]) == LC._lattice("smooth", D).M
        for k in a:
            np.testing.assert_array_equal(np.asarray(a[k]), np.asarray(b[k]), err_msg=k)
    finally:
        batch.close()
        alone.close()


def test_state_and_argument_errors_and_what_a_probe_leaves():
    """No batch: PNP_ERR_STATE.  A term or stage out of range, null pointers: PNP_ERR_ARG, nothing written.  A probe drops the
    stepwise state and leaves the batch as it was: the same inference gives the same bits before and after."""
    from pnp_ovss import crf, hip
    D, K = 3, 5
    feats = LC.batch_images(D)
    pix = [h * w for h, w in SIZES]
    solver = crf.FeatureCRF(4, sum(pix), max(pix), K, max_terms=2, max_dims=D)
    try:
        lib, view = solver.lib, hip.PnpCrfLatticeView()
        buf = Guarded((64,), torch.float32, guard=64)
        assert lib.pnp_crf_lattice_view_get(solver.h, 0, ctypes.byref(view)) == PNP_ERR_STATE
        assert lib.pnp_crf_probe_filter(solver.h, 0, 0, buf.ptr, buf.ptr, None) == PNP_ERR_STATE
        d_unary = torch.from_numpy(np.random.default_rng(0).random(K * sum(pix), dtype=F32)).to(solver.device)
        d_feat = torch.from_numpy(np.concatenate([f.reshape(-1) for f in feats])).to(solver.device)
        solver.set_batch(d_unary, [d_feat], [D], SIZES, [K] * 4)
        for term in (-1, 1, 8):                               # the batch has one term
            assert lib.pnp_crf_lattice_view_get(solver.h, term, ctypes.byref(view)) == PNP_ERR_ARG
            assert lib.pnp_crf_probe_filter(solver.h, term, 0, buf.ptr, buf.ptr, None) == PNP_ERR_ARG
        assert lib.pnp_crf_lattice_view_get(solver.h, 0, None) == PNP_ERR_ARG
        for stage in (-1, 4):
            assert lib.pnp_crf_probe_filter(solver.h, 0, stage, buf.ptr, buf.ptr, None) == PNP_ERR_ARG
        assert lib.pnp_crf_probe_filter(solver.h, 0, 0, None, buf.ptr, None) == PNP_ERR_ARG
        assert lib.pnp_crf_probe_filter(solver.h, 0, 0, buf.ptr, None, None) == PNP_ERR_ARG
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf.check("refused probe", written=0)).all())      # refused calls wrote nothing
        _, q0 = solver.infer(iters=2, weights=[4.0])
        q0 = [q.cpu().numpy() for q in q0]
        idbase = solver.lattice_arrays(0)["idbase"]
        _probe(solver, 0, "slice", LC.probe_rows(SIZES, K, 1), idbase, "state")
        with pytest.raises(RuntimeError, match="no inference was started"):
            solver.step(1)
        _, q1 = solver.infer(iters=2, weights=[4.0])
        for a, b in zip(q0, q1):
            np.testing.assert_array_equal(a.view(np.int32), b.cpu().numpy().view(np.int32))
    finally:
        solver.close()


@pytest.mark.parametrize("n", [4097, 70001])
@pytest.mark.parametrize("bits", [16, 48, 60, 64])
def test_sort_pairs_over_the_widths_of_the_feature_keys(n, bits):
    """pnp_op_sort_pairs over key bits [0, bits) against np.argsort(kind="stable"): random keys and keys with many ties; the
    D = 4 feature key uses all 64 bits, D = 1 / 3 / 5 / 6 use 16 / 48 / 60 / 60."""
    from pnp_ovss import hip
    lib = hip.load_library()
    rng = np.random.default_rng(1000 * bits + n)
    mask = np.uint64((1 << bits) - 1)
    for kind in ("random", "ties"):
        keys = rng.integers(0, 2 ** 64, size=n, dtype=np.uint64, endpoint=False)
        if kind == "ties":
            keys &= np.uint64(0x8000000000000003) | (np.uint64(3) << np.uint64(bits - 2))
        sel = keys & mask
        order = np.argsort(sel, kind="stable")
        vals = np.arange(n, dtype=np.uint32)
        kin = torch.from_numpy(keys.view(np.int64).copy()).cuda()
        vin = torch.from_numpy(vals.view(np.int32).copy()).cuda()
        kout, vout = Guarded((n,), torch.float64, guard=256), Guarded((n,), torch.float32, guard=256)
        assert lib.pnp_op_sort_pairs(kin.data_ptr(), kout.ptr, vin.data_ptr(), vout.ptr, n, 0, bits, None, 0, None) == 0
        torch.cuda.synchronize()
        # (sorted keys may look like NaN as float64: the guards are checked here, every element against the reference below)
        got_k = kout.check(f"sort keys {kind} n={n} bits={bits}", written=0).numpy().view(np.uint64)
        got_v = vout.check(f"sort values {kind} n={n} bits={bits}", written=0).numpy().view(np.uint32)
        np.testing.assert_array_equal(got_v, vals[order], err_msg=f"{kind} n={n} bits={bits}")
        np.testing.assert_array_equal(got_k, keys[order], err_msg=f"{kind} n={n} bits={bits}")
