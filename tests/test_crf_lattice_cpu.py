"""CPU: the inputs and the checkers of the per-stage DenseCRF lattice tests (tests/_crf_lattice_checks.py), proven without a
device.  The images really hold what test_crf_lattice_gpu.py relies on -- contributor lists of every length class of the splat,
absent and present neighbours, negative keys, keys at the edge of the 12- and 10-bit fields --; the checkers pass arrays derived
from the reference and name the right stage for every fault planted in them; the split of _crf_general_ref.Lattice.compute into
splat, blur and slice leaves its bits; and the two new entry points refuse bad arguments before any HIP call."""
import ctypes
import os

import numpy as np
import pytest

import _crf_general_ref as G
import _crf_lattice_checks as LC

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "pnp-ovss_amd", "pnp_ovss", "libpnp_hip.so")
PNP_ERR_ARG = -22
DIMS = (1, 2, 3, 4, 5, 6)
SIZES = [LC.RUNS_SIZE, LC.RUNS_SIZE, LC.SMOOTH_SIZE, LC.LINE_SIZE]


def _compute_before_the_split(L, x):
    """Lattice.compute as it stood before splat / blur / slice were split out of it."""
    x = np.ascontiguousarray(x, dtype=F32)
    N, d, M, vs = L.N, L.d, L.M, x.shape[1]
    values = np.zeros((M + 1, vs), F32)
    o = (L.offset + 1).reshape(-1)
    np.add.at(values, o, L.bary.reshape(-1, 1) * np.repeat(x, d + 1, axis=0))
    for j in range(d + 1):
        t = values[L.n1[j] + 1] + values[L.n2[j] + 1]
        new = np.zeros_like(values)
        new[1:] = (values[1:].astype(np.float64) + 0.5 * t.astype(np.float64)).astype(F32)
        values = new
    alpha = F32(1.0) / (F32(1.0) + F32(2.0 ** -d))
    out = np.zeros((N, vs), F32)
    for j in range(d + 1):
        out = out + L.bary[:, j, None] * values[L.offset[:, j] + 1] * alpha
    return out


@pytest.mark.parametrize("D", DIMS)
def test_compute_keeps_its_bits_and_its_parts_are_reachable(D):
    L = LC._lattice("smooth", D)
    x = np.random.default_rng(D).standard_normal((L.N, 3)).astype(F32)
    want = _compute_before_the_split(L, x)
    np.testing.assert_array_equal(L.compute(x).view(np.int32), want.view(np.int32))
    np.testing.assert_array_equal(L.slice(L.blur(L.splat(x), range(D + 1))).view(np.int32), want.view(np.int32))
    if D >= 2:                                              # the axis blurs do not commute in float32: the reverse order is another result
        assert not np.array_equal(L.blur(L.splat(x), range(D, -1, -1)), L.blur(L.splat(x)))


@pytest.mark.parametrize("D", DIMS)
def test_runs_image_holds_every_list_length_of_the_splat(D):
    """Lists of exactly 1, G, G + 1, LPP, LPP + 1 for LPP = 8, 16, 32, 40 and 70 (beyond 2 LPP: the continuation loop) and the
    background's 1199, on 10 (D + 1) points, for every D; the keys stay inside the feature key."""
    L = LC._lattice("runs", D)
    assert sorted(set(LC.list_lengths(L).tolist())) == sorted(LC.RUNS + [1199])
    assert L.M == 10 * (D + 1)
    assert int(np.abs(L.keys).max()) == {1: 63, 2: 150, 3: 203, 4: 255, 5: 309, 6: 366}[D] < LC.KEY_LIMIT[D]
    assert LC.runs_image(D).shape == (D,) + LC.RUNS_SIZE and float(LC.runs_image(D).min()) < 0


@pytest.mark.parametrize("D", DIMS)
def test_smooth_image_has_absent_and_present_neighbours_and_negative_keys(D):
    L = LC._lattice("smooth", D)
    absent = float((L.n1 < 0).mean())
    negative = float((L.keys < 0).mean())
    print(f"[measured] smooth image D={D}: {L.M} points, absent n1 share {absent:.2f}, negative key share {negative:.2f}")
    assert 0.05 <= absent <= 0.95
    assert negative >= 0.30
    assert int(np.abs(L.keys).max()) < LC.KEY_LIMIT[D]


@pytest.mark.parametrize("D,limit", [(5, 2042), (6, 505)])
def test_limit_image_reaches_the_edge_of_the_key_field(D, limit):
    assert LC.KEY_LIMIT[D] == limit == (1 << (64 // D - 1)) - D - 1
    L = LC._lattice("limit", D)
    top = int(np.abs(L.keys).max())
    print(f"[measured] limit image D={D}: factor {LC.LIMIT_FACTOR[D]}, largest |key| {top}")
    assert limit - 8 <= top <= limit - 1
    assert sorted(set(LC.list_lengths(L).tolist())) == sorted(LC.RUNS + [1199])


def test_every_image_is_small_and_the_batch_has_identical_neighbours():
    assert all(h * w < 2000 for h, w in SIZES)
    for D in DIMS:
        imgs = LC.batch_images(D)
        assert [f.shape for f in imgs] == [(D,) + s for s in SIZES]
        assert np.array_equal(imgs[0], imgs[1])              # identical keys in adjacent images


@pytest.mark.parametrize("K,dispatch", [(5, "8"), (59, "16"), (100, "32"), (151, "multi")])
def test_label_counts_cover_every_splat_dispatch(K, dispatch):
    """crf_splat's rule on the chunks of the widest row; K = 151 is MULTI with 38 chunks."""
    k4 = ((K + 3) // 4 * 4 + 3) // 4
    assert ("8" if k4 <= 8 else "16" if k4 <= 16 else "32" if k4 <= 32 else "multi") == dispatch
    assert K != 151 or k4 == 38


@pytest.fixture(scope="module", params=DIMS, ids=lambda D: f"D{D}")
def derived(request):
    D = request.param
    refs = LC.batch_lattices(D)
    dev, order = LC.device_like(refs, SIZES)
    return D, refs, dev, order


def test_arrays_derived_from_the_reference_pass_every_stage(derived):
    D, refs, dev, order = derived
    maps = LC.check_build(dev, refs, SIZES, points=dev["points"])
    for (d2r, _), o in zip(maps, order):
        np.testing.assert_array_equal(d2r, o)
    assert any(not np.array_equal(o, np.arange(len(o))) for o in order)       # the numbering really is another one
    planes = LC.probe_rows(SIZES, 5, seed=D)
    want = [LC.reference_stages(r, p) for r, p in zip(refs, planes)]
    for stage in ("splat", "forward", "reverse"):
        LC.check_rows(stage, [w[stage][o] for w, o in zip(want, order)], [w[stage] for w in want], maps)
    LC.check_rows("slice", [w["slice"].reshape(5, h, wd) for w, (h, wd) in zip(want, SIZES)], [w["slice"] for w in want])
    for ref, w, p in zip(refs, want, planes):                # the slice stage is compute() between the normalisers
        nrm = LC.norm_of(ref)[:, None]
        np.testing.assert_array_equal(w["slice"].T, ref.compute(p.T * nrm) * nrm)


@pytest.fixture(scope="module")
def d3():
    refs = LC.batch_lattices(3)
    dev, order = LC.device_like(refs, SIZES)
    return refs, dev, order


@pytest.mark.parametrize("fault", LC.BUILD_FAULTS)
def test_a_planted_build_fault_fails_in_its_stage(d3, fault):
    refs, dev, _ = d3
    bad, stage = LC.plant(dev, fault, SIZES)
    with pytest.raises(LC.StageError) as e:
        LC.check_build(bad, refs, SIZES, points=dev["points"])
    assert e.value.stage == stage and str(e.value).startswith(stage + ": "), str(e.value)
    LC.check_build(dev, refs, SIZES, points=dev["points"])    # (the arrays the fault was planted in are untouched)


def test_a_wrong_point_count_fails_in_embed(d3):
    refs, dev, _ = d3
    with pytest.raises(LC.StageError) as e:
        LC.check_embed(dev, refs, SIZES, points=dev["points"] + 1)
    assert e.value.stage == "embed"


@pytest.mark.parametrize("fault", ["splat in descending pixel order", "forward with two axes exchanged", "reverse handed in as forward"])
def test_a_planted_filter_fault_fails_in_its_stage(d3, fault):
    refs, dev, order = d3
    maps = LC.check_embed(dev, refs, SIZES)
    planes = LC.probe_rows(SIZES, 5, seed=3)
    want = [LC.reference_stages(r, p) for r, p in zip(refs, planes)]
    if fault.startswith("splat"):
        stage, rows = "splat", [LC.splat_descending(r, p) for r, p in zip(refs, planes)]
    elif fault.startswith("forward"):
        stage = "forward"
        rows = [r.blur(np.concatenate([np.zeros((1, 5), F32), w["splat"]]), [1, 0, 2, 3])[1:] for r, w in zip(refs, want)]
    else:
        stage, rows = "forward", [w["reverse"] for w in want]
    with pytest.raises(LC.StageError) as e:
        LC.check_rows(stage, [r[o] for r, o in zip(rows, order)], [w[stage] for w in want], maps)
    assert e.value.stage == stage and str(e.value).startswith(stage + ": "), str(e.value)


def test_an_image_of_a_batch_made_local_equals_the_image_alone(d3):
    """LC.image_local, on which the batch-independence test of the GPU rests: image 2 of the derived batch, ids and pixels made
    local, is what the same image derives alone."""
    refs, dev, _ = d3
    alone, _ = LC.device_like([refs[2]], [SIZES[2]])
    local = LC.image_local(dev, SIZES, 2)
    for k, v in LC.image_local(alone, [SIZES[2]], 0).items():
        np.testing.assert_array_equal(np.asarray(local[k]), np.asarray(v), err_msg=k)


def test_new_entry_points_refuse_bad_arguments_without_a_device():
    """pnp_crf_lattice_view_get and pnp_crf_probe_filter return PNP_ERR_ARG before any HIP call for a null solver, whatever else
    they are given (a null view, a term or stage out of range, null buffers), as the neighbouring entry points do; the state
    errors of a solver without a batch need a solver, hence a device: test_crf_lattice_gpu.py."""
    if not os.path.exists(LIB):
        import subprocess
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "pnp-ovss_amd", "csrc"), "-j8"])
    lib = ctypes.CDLL(LIB)
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    lib.pnp_crf_lattice_view_get.argtypes = [vp, i32, vp]
    lib.pnp_crf_probe_filter.argtypes = [vp, i32, i32, vp, vp, vp]
    lib.pnp_crf_lattice_points.argtypes = [vp, i32]
    lib.pnp_crf_lattice_points.restype = ctypes.c_int64
    view = (ctypes.c_char * 256)()
    for term in (-1, 0, 1, 8):
        assert lib.pnp_crf_lattice_view_get(None, term, view) == PNP_ERR_ARG
        assert lib.pnp_crf_lattice_view_get(None, term, None) == PNP_ERR_ARG
        assert lib.pnp_crf_lattice_points(None, term) == -1
        for stage in (-1, 0, 3, 4):
            assert lib.pnp_crf_probe_filter(None, term, stage, None, None, None) == PNP_ERR_ARG
            assert lib.pnp_crf_probe_filter(None, term, stage, vp(4096), vp(4096), None) == PNP_ERR_ARG
    assert bytes(view) == bytes(256)                          # nothing was written


def test_view_structure_matches_the_header():
    """pnp_ovss.hip.PnpCrfLatticeView has the fields of include/pnp_hip.h's pnp_crf_lattice_view, in order."""
    import re
    from pnp_ovss import hip
    src = open(os.path.join(ROOT, "include", "pnp_hip.h")).read()
    body = re.search(r"typedef struct pnp_crf_lattice_view \{(.*?)\} pnp_crf_lattice_view;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.search(r"(\w+)\s*$", decl.strip()).group(1) for decl in body.split(";") if decl.strip()]
    assert names == [n for n, _ in hip.PnpCrfLatticeView._fields_]
    assert ctypes.sizeof(hip.PnpCrfLatticeView) == 4 + 4 + 3 * 8 + 11 * 8
