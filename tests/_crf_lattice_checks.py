"""Per-stage checks of the DenseCRF lattice (test_crf_lattice_cpu.py, test_crf_lattice_gpu.py): what a lattice build leaves on
the device -- barycentric weights, lattice ids, neighbour tables, two-axis neighbour records, contributor lists, normaliser --
and the value rows after the splat, the forward and reverse axis blurs and the slice, each against tests/_crf_general_ref.Lattice
(the numpy restatement of oracle/densecrf_ref.c), bit for bit.  Pure numpy.

Every checker takes the arrays of ONE term over a batch as pnp_ovss.crf._Solver.lattice_arrays returns them (`dev`: global lattice
ids and global pixel indices, images back to back) and the per-image references, and raises StageError with the name of the stage
in front.  Lattice ids are internal -- the device numbers the points of an image along a Z-order curve of their first
contributor, the reference by np.unique of the keys -- so everything is compared through the id bijection check_embed
establishes (`maps`).

Also here: the images of the tests (their properties are proven in test_crf_lattice_cpu.py) and, for that test, device-like arrays
derived from the reference alone with faults planted in them."""
import copy
import functools

import numpy as np

import _crf_general_ref as G

F32 = np.float32
ENT = np.dtype([("pixel", "<u4"), ("w", "<f4"), ("nr", "<f4"), ("pad", "<u4")])
STAGES = ("embed", "neighbours", "nbr8", "lists", "numbering", "norm", "splat", "forward", "reverse", "slice")


class StageError(AssertionError):
    def __init__(self, stage, text):
        super().__init__(f"{stage}: {text}")
        self.stage = stage


def _need(ok, stage, text):
    if not ok:
        raise StageError(stage, text() if callable(text) else text)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


def _first_bad(mask):
    return tuple(int(i) for i in np.argwhere(mask)[0])


# ------------------------------------------------------------------------------------------ images
RUNS = [1, 8, 9, 16, 17, 32, 33, 40, 70]
RUNS_SIZE, SMOOTH_SIZE, LINE_SIZE = (19, 75), (23, 31), (1, 7)
KEY_LIMIT = {1: 32000, 2: 32000, 3: 32000, 4: 32000, 5: 2042, 6: 505}       # crf_feature_key_limit(D): |key| stays below it
# the runs image times this factor has its largest |key| in [limit - 8, limit - 1]: 2034 and 497 (proven in test_crf_lattice_cpu.py)
LIMIT_FACTOR = {5: 6.6217, 6: 1.3614}


def runs_image(D, factor=1.0):
    """(D, 19, 75) float32, piecewise constant: background vector 0.37 (-1)^i (i + 1); run r of RUNS on row 2 r + 1 from column
    2 with the vector (-1)^(r + i) (6 (r + 1) + 1.3 i).  Every run is far from everything else in every feature, so its lattice
    points are its own: contributor lists of exactly the lengths RUNS, and one of 1199 for the background, per simplex vertex."""
    H, W = RUNS_SIZE
    f = np.empty((D, H, W), np.float64)
    for i in range(D):
        f[i] = 0.37 * (-1) ** i * (i + 1)
        for r, n in enumerate(RUNS):
            f[i, 2 * r + 1, 2:2 + n] = (-1) ** (r + i) * (6 * (r + 1) + 1.3 * i)
    f = (f * factor).astype(F32)
    f.setflags(write=False)
    return f


def smooth_image(D, size=SMOOTH_SIZE):
    """(D, H, W) float32: (x - W // 2) / 3, (y - H // 2) / 3, then planes of seeded integers (0 .. 255) / 40 - 3; D = 1 takes the
    first of those alone.  Negative and positive coordinates, neighbours present and absent."""
    H, W = size
    rng = np.random.default_rng(1000 * H + W)
    yy, xx = np.mgrid[0:H, 0:W]
    noise = [rng.integers(0, 256, (H, W)).astype(F32) / F32(40) - F32(3) for _ in range(4)]
    planes = [(xx - W // 2).astype(F32) / F32(3), (yy - H // 2).astype(F32) / F32(3)] + noise
    f = np.stack(planes[2:3] if D == 1 else planes[:D]).astype(F32)
    f.setflags(write=False)
    return f


def batch_images(D):
    """The batch of the feature-path tests: the runs image, the same again (identical keys in adjacent images), the smooth image
    and a single pixel line of 7.  -> [(D, H, W) float32]"""
    return [runs_image(D), runs_image(D), smooth_image(D), smooth_image(D, LINE_SIZE)]


def limit_image(D):
    return runs_image(D, LIMIT_FACTOR[D])


@functools.lru_cache(maxsize=None)
def _lattice(kind, D):
    f = {"runs": runs_image, "smooth": smooth_image, "line": lambda d: smooth_image(d, LINE_SIZE), "limit": limit_image}[kind](D)
    return lattice_of(f)


def lattice_of(f):
    """The reference lattice of (d, H, W) or (d, N) features."""
    f = np.asarray(f)
    return G.Lattice(np.ascontiguousarray(f.reshape(f.shape[0], -1).T))


def batch_lattices(D):
    return [_lattice(k, D) for k in ("runs", "runs", "smooth", "line")]


def norm_of(ref):
    """ref.norm() as (N,) float32, computed once per reference."""
    if not hasattr(ref, "_norm1"):
        ref._norm1 = np.ascontiguousarray(ref.norm().reshape(-1))
    return ref._norm1


def list_lengths(ref):
    return np.bincount(ref.offset.reshape(-1), minlength=ref.M)


def probe_rows(sizes, K, seed):
    """Per image the (K, H * W) float32 probe input: seeded uniform in (0, 1), never zero."""
    rng = np.random.default_rng(seed)
    return [np.maximum(rng.random((K, h * w), dtype=F32), F32(2.0 ** -24)) for h, w in sizes]


def reference_stages(ref, planes):
    """One filter pass of the reference on planes (K, N): rows of every stage.  splat / forward / reverse (M, K) in the reference's
    id order, slice (K, N): the message norm * alpha * slice(forward)."""
    nrm = norm_of(ref)[:, None]
    x = np.ascontiguousarray(planes.T, dtype=F32) * nrm
    sp = ref.splat(x)
    fw = ref.blur(sp)
    rv = ref.blur(sp, range(ref.d, -1, -1))
    msg = np.zeros((ref.N, x.shape[1]), F32) + ref.slice(fw) * nrm
    return dict(splat=sp[1:], forward=fw[1:], reverse=rv[1:], slice=np.ascontiguousarray(msg.T))


# ------------------------------------------------------------------------------------------ Z-order
def _spread(v):
    v = v.astype(np.uint64)
    v = (v | (v << np.uint64(8))) & np.uint64(0x00FF00FF)
    v = (v | (v << np.uint64(4))) & np.uint64(0x0F0F0F0F)
    v = (v | (v << np.uint64(2))) & np.uint64(0x33333333)
    v = (v | (v << np.uint64(1))) & np.uint64(0x55555555)
    return v


def zorder_key(local_pixel, vertex, W):
    """first_contrib_kernel's sort key inside an image: (Morton position of the pixel) << 3 | vertex."""
    y, x = local_pixel // W, local_pixel % W
    return ((_spread(x) | (_spread(y) << np.uint64(1))) << np.uint64(3)) | vertex.astype(np.uint64)


def _pix0(sizes):
    return np.concatenate([[0], np.cumsum([h * w for h, w in sizes])]).astype(np.int64)


# ------------------------------------------------------------------------------------------ the checkers
def check_embed(dev, refs, sizes, points=None):
    """bary bit for bit; per image the pairing of device and reference ids over all (pixel, vertex) is a bijection onto
    0 .. M_b - 1; idbase counts the reference's points.  -> maps: per image (d2r, r2d) local id arrays."""
    D1, pix0, idbase = dev["D1"], _pix0(sizes), dev["idbase"].astype(np.int64)
    want = np.concatenate([_bits(r.bary).reshape(-1) for r in refs])
    _need(dev["bary"].shape == want.shape, "embed", lambda: f"bary has {dev['bary'].shape} entries, the references {want.shape}")
    bad = _bits(dev["bary"]) != want
    _need(not bad.any(), "embed", lambda: f"bary differs from the reference in {int(bad.sum())} of {bad.size} entries, first at "
          f"(pixel, vertex) {divmod(_first_bad(bad)[0], D1)}: {dev['bary'][bad][0]!r} != {want.view(F32)[bad][0]!r}")
    _need(idbase[0] == 0, "embed", f"idbase[0] = {idbase[0]}")
    counts = [int(r.M) for r in refs]
    _need(list(np.diff(idbase)) == counts, "embed", lambda: f"points per image {list(np.diff(idbase))}, the references have {counts}")
    if points is not None:
        _need(int(idbase[-1]) == int(points), "embed", f"idbase[B] = {idbase[-1]}, pnp_crf_lattice_points = {points}")
    maps = []
    for b, ref in enumerate(refs):
        dl = dev["offset"][pix0[b] * D1:pix0[b + 1] * D1].astype(np.int64) - idbase[b]
        rl = ref.offset.reshape(-1)
        _need(dl.shape == rl.shape and dl.min() >= 0 and dl.max() < ref.M, "embed",
              lambda: f"image {b}: lattice ids {dl.min() + idbase[b]} .. {dl.max() + idbase[b]} leave the image's range "
              f"[{idbase[b]}, {idbase[b + 1]})")
        pairs = np.unique(np.stack([dl, rl], 1), axis=0)
        _need(len(pairs) == ref.M and len(np.unique(pairs[:, 0])) == ref.M and len(np.unique(pairs[:, 1])) == ref.M, "embed",
              lambda: f"image {b}: device and reference ids do not pair one to one ({len(pairs)} distinct pairs, "
              f"{len(np.unique(pairs[:, 0]))} device ids, {len(np.unique(pairs[:, 1]))} reference ids, {ref.M} points)")
        d2r = np.empty(ref.M, np.int64)
        d2r[pairs[:, 0]] = pairs[:, 1]
        r2d = np.empty(ref.M, np.int64)
        r2d[d2r] = np.arange(ref.M)
        maps.append((d2r, r2d))
    return maps


def check_neighbours(dev, refs, maps):
    """n1 / n2 of every axis equal the reference's under the bijection, -1 to -1; no id leaves the point's image."""
    idbase = dev["idbase"].astype(np.int64)
    for b, (ref, (d2r, r2d)) in enumerate(zip(refs, maps)):
        lo, hi = idbase[b], idbase[b + 1]
        for name in ("n1", "n2"):
            got = dev[name][:, lo:hi].astype(np.int64)
            out = (got != -1) & ((got < lo) | (got >= hi))
            _need(not out.any(), "neighbours", lambda: f"image {b}: {name}[axis, point] = {got[out][0]} at {_first_bad(out)} is outside "
                  f"the image's ids [{lo}, {hi})")
            r = getattr(ref, name)[:, d2r]
            want = np.where(r >= 0, r2d[np.maximum(r, 0)] + lo, -1)
            bad = got != want
            _need(not bad.any(), "neighbours", lambda: f"image {b}: {name} differs in {int(bad.sum())} entries, first at (axis, local "
                  f"point) {_first_bad(bad)}: {got[bad][0]} != {want[bad][0]}")


def nbr8_from(n1, n2, idbase):
    """What nbr8_kernel documents, from global-id tables n1 / n2 (D1, M): (D1 // 2, M, 8) image-local ids in the order ia, id,
    pa, pd, aa, ad, da, dd; an absent second-axis neighbour has absent first-axis neighbours."""
    D1, M = n1.shape
    n1, n2 = n1.astype(np.int64), n2.astype(np.int64)
    lo = np.repeat(idbase[:-1].astype(np.int64), np.diff(idbase))

    def via(table, at):
        return np.where(at >= 0, table[np.maximum(at, 0)], -1)
    out = np.empty((D1 // 2, M, 8), np.int64)
    for p in range(D1 // 2):
        a1, a2, b1, b2 = n1[2 * p], n2[2 * p], n1[2 * p + 1], n2[2 * p + 1]
        rec = np.stack([a1, a2, b1, b2, via(a1, b1), via(a2, b1), via(a1, b2), via(a2, b2)], 1)
        out[p] = np.where(rec >= 0, rec - lo[:, None], -1)
    return out


def check_nbr8(dev):
    want = nbr8_from(dev["n1"], dev["n2"], dev["idbase"])
    got = dev["nbr8"].astype(np.int64)
    _need(got.shape == want.shape, "nbr8", lambda: f"shape {got.shape}, expected {want.shape}")
    bad = got != want
    names = ("ia", "id", "pa", "pd", "aa", "ad", "da", "dd")
    _need(not bad.any(), "nbr8", lambda: f"{int(bad.sum())} fields differ from n1 / n2, first at (pair, point) {_first_bad(bad)[:2]} "
          f"field {names[_first_bad(bad)[2]]}: {got[bad][0]} != {want[bad][0]}")


def check_lists(dev):
    """The contributor lists: ranges tile [0, E) in id order, (pixel, vertex) indices strictly ascending inside a range, records
    agree with bary / norm bit for bit, and a point's range holds exactly the (pixel, vertex) pairs whose offset is the point."""
    D1, lo, hi, vals, ent = dev["D1"], dev["seg_lo"].astype(np.int64), dev["seg_hi"].astype(np.int64), dev["vals"].astype(np.int64), dev["ent"]
    E, M = len(dev["offset"]), len(lo)
    _need(len(vals) == E and len(ent) == E, "lists", lambda: f"{len(vals)} list entries / {len(ent)} records for {E} (pixel, vertex) pairs")
    _need(M > 0 and lo[0] == 0 and hi[-1] == E and (lo[1:] == hi[:-1]).all() and (hi > lo).all(), "lists",
          lambda: f"the ranges [seg_lo, seg_hi) do not tile [0, {E}) in id order: starts at {lo[0]}, ends at {hi[-1]}, "
          f"{int((lo[1:] != hi[:-1]).sum())} gaps or overlaps, {int((hi <= lo).sum())} empty ranges; first at point "
          f"{int(np.argmax(np.concatenate([lo[1:] != hi[:-1], [True]]) | (hi <= lo)))}")
    inner = np.ones(E, bool)
    inner[lo] = False
    bad = inner[1:] & (np.diff(vals) <= 0)
    _need(not bad.any(), "lists", lambda: f"vals is not strictly ascending inside a list: entries {_first_bad(bad)[0]} and the next "
          f"hold {vals[_first_bad(bad)[0]]}, {vals[_first_bad(bad)[0] + 1]}")
    _need(vals.min() >= 0 and vals.max() < E, "lists", "a list entry is no (pixel, vertex) index of the batch")
    bad = vals // D1 != ent["pixel"].astype(np.int64)
    _need(not bad.any(), "lists", lambda: f"ent.pixel != vals // D1 at entry {_first_bad(bad)[0]}")
    bad = ent["w"].view(np.int32) != _bits(dev["bary"])[vals]
    _need(not bad.any(), "lists", lambda: f"ent.w is not bary[vals] at entry {_first_bad(bad)[0]}")
    bad = ent["nr"].view(np.int32) != _bits(dev["norm"])[vals // D1]
    _need(not bad.any(), "lists", lambda: f"ent.nr is not norm[ent.pixel] at entry {_first_bad(bad)[0]} (pixel {vals[bad][0] // D1}): "
          f"{ent['nr'][bad][0]!r} != {dev['norm'][vals[bad][0] // D1]!r}")
    owner = np.repeat(np.arange(M), hi - lo)
    bad = dev["offset"].astype(np.int64)[vals] != owner
    _need(not bad.any(), "lists", lambda: f"entry {_first_bad(bad)[0]} sits in the list of point {owner[bad][0]} but its offset is "
          f"{dev['offset'][vals[bad][0]]}")
    _need(np.array_equal(np.sort(vals), np.arange(E)), "lists", "the lists do not hold every (pixel, vertex) pair exactly once")


def check_numbering(dev, sizes):
    """first_contrib_kernel's contract: inside an image ids ascend strictly in (Morton position of the first contributor pixel,
    its vertex)."""
    D1, pix0, idbase = dev["D1"], _pix0(sizes), dev["idbase"].astype(np.int64)
    first = dev["vals"].astype(np.int64)[dev["seg_lo"]]
    for b, (h, w) in enumerate(sizes):
        pv = first[idbase[b]:idbase[b + 1]]
        local = pv // D1 - pix0[b]
        _need(local.min() >= 0 and local.max() < h * w, "numbering", f"image {b}: a first contributor lies in another image")
        key = zorder_key(local, pv % D1, w)
        bad = np.diff(key.astype(np.int64)) <= 0
        _need(not bad.any(), "numbering", lambda: f"image {b}: ids {idbase[b] + _first_bad(bad)[0]} and the next are not in Z-order of "
              f"their first contributors (pixel, vertex) {divmod(int(pv[_first_bad(bad)[0]]), D1)}, "
              f"{divmod(int(pv[_first_bad(bad)[0] + 1]), D1)}")


def check_norm(dev, refs):
    want = np.concatenate([_bits(norm_of(r)) for r in refs])
    bad = _bits(dev["norm"]) != want
    _need(not bad.any(), "norm", lambda: f"{int(bad.sum())} of {bad.size} normalisers differ, first at pixel {_first_bad(bad)[0]}: "
          f"{dev['norm'][bad][0]!r} != {want.view(F32)[bad][0]!r}")


def check_rows(stage, got, want, maps=None):
    """A filter stage bit for bit.  got: per image the device rows -- (M_b, K) in device id order, compared with the reference's
    rows through the bijection; for "slice" (K, ...) planes, compared directly.  want: per image reference_stages(...)[stage]."""
    for b, (g, w) in enumerate(zip(got, want)):
        g = np.asarray(g, dtype=F32)
        if stage != "slice":
            w = w[maps[b][0]]
        g = g.reshape(w.shape) if g.size == w.size else g
        _need(g.shape == w.shape, stage, lambda: f"image {b}: shape {g.shape}, the reference has {w.shape}")
        bad = _bits(g) != _bits(w)
        _need(not bad.any(), stage, lambda: f"image {b}: {int(bad.sum())} of {bad.size} values differ from the reference, largest "
              f"difference {np.abs(g.astype(np.float64) - w)[bad].max():.3e}, first at {_first_bad(bad)}: {g[bad][0]!r} != {w[bad][0]!r}")


def check_build(dev, refs, sizes, points=None, stages=("embed", "neighbours", "nbr8", "lists", "numbering", "norm")):
    """The build stages in order.  -> maps"""
    maps = check_embed(dev, refs, sizes, points)
    if "neighbours" in stages:
        check_neighbours(dev, refs, maps)
    if "nbr8" in stages:
        check_nbr8(dev)
    if "lists" in stages:
        check_lists(dev)
    if "numbering" in stages:
        check_numbering(dev, sizes)
    if "norm" in stages:
        check_norm(dev, refs)
    return maps


def image_local(dev, sizes, b):
    """The arrays of image b of a batch with ids, pixels and list positions made local to the image: what the same image
    prepared alone must give."""
    D1, pix0, idbase = dev["D1"], _pix0(sizes), dev["idbase"].astype(np.int64)
    lo, hi, e0, e1 = idbase[b], idbase[b + 1], pix0[b] * D1, pix0[b + 1] * D1

    def ids(a):
        a = a.astype(np.int64)
        return np.where(a >= 0, a - lo, -1)
    s0 = int(dev["seg_lo"][lo])
    ent = dev["ent"][s0:s0 + (e1 - e0)].copy()
    ent["pixel"] -= np.uint32(pix0[b])
    return dict(D1=D1, bary=dev["bary"][e0:e1], offset=ids(dev["offset"][e0:e1]), norm=dev["norm"][pix0[b]:pix0[b + 1]],
                seg_lo=dev["seg_lo"][lo:hi].astype(np.int64) - s0, seg_hi=dev["seg_hi"][lo:hi].astype(np.int64) - s0,
                vals=dev["vals"][s0:s0 + (e1 - e0)].astype(np.int64) - e0, ent=ent, n1=ids(dev["n1"][:, lo:hi]),
                n2=ids(dev["n2"][:, lo:hi]), nbr8=dev["nbr8"][:, lo:hi].astype(np.int64))


# ------------------------------------------------------------------------------------------ device-like arrays from the reference
def device_like(refs, sizes):
    """What a correct build would leave for these references, derived from them alone: per image the points renumbered by the
    Z-order of their first contributor (a permutation of the reference's np.unique order), lists, records and two-axis
    neighbour records built from that numbering.  -> (dev, order): order[b][i] = reference id of device point i of image b."""
    D1 = refs[0].d + 1
    pix0 = _pix0(sizes)
    offset, n1, n2, vals, seg_len, order_all, idbase = [], [], [], [], [], [], [0]
    for b, (ref, (h, w)) in enumerate(zip(refs, sizes)):
        rid = ref.offset.reshape(-1)
        pv = np.arange(rid.size)
        first = np.full(ref.M, rid.size, np.int64)
        np.minimum.at(first, rid, pv)
        order = np.argsort(zorder_key(first // D1, first % D1, w), kind="stable")
        r2d = np.empty(ref.M, np.int64)
        r2d[order] = np.arange(ref.M)
        lo = idbase[-1]
        did = r2d[rid]
        offset.append(did + lo)
        by_point = np.argsort(did, kind="stable")
        vals.append(pv[by_point] + pix0[b] * D1)
        seg_len.append(np.bincount(did, minlength=ref.M))
        for src, dst in ((ref.n1, n1), (ref.n2, n2)):
            t = src[:, order]
            dst.append(np.where(t >= 0, r2d[np.maximum(t, 0)] + lo, -1))
        order_all.append(order)
        idbase.append(lo + ref.M)
    vals = np.concatenate(vals)
    hi = np.cumsum(np.concatenate(seg_len))
    dev = dict(D1=D1, cap=int(idbase[-1]), points=int(idbase[-1]), idbase=np.array(idbase, np.int32),
               bary=np.concatenate([r.bary.reshape(-1) for r in refs]).astype(F32), offset=np.concatenate(offset).astype(np.int32),
               vals=vals.astype(np.uint32), seg_lo=(hi - np.concatenate(seg_len)).astype(np.int32), seg_hi=hi.astype(np.int32),
               n1=np.concatenate(n1, 1).astype(np.int32), n2=np.concatenate(n2, 1).astype(np.int32),
               norm=np.concatenate([norm_of(r) for r in refs]))
    ent = np.zeros(len(vals), ENT)
    ent["pixel"] = vals // D1
    ent["w"] = dev["bary"][vals]
    ent["nr"] = dev["norm"][vals // D1]
    dev["ent"] = ent
    dev["nbr8"] = nbr8_from(dev["n1"], dev["n2"], dev["idbase"]).astype(np.int32)
    return dev, order_all


def _swap(a, i, j):
    a[i], a[j] = copy.copy(a[j]), copy.copy(a[i])


def _renumber(dev, i, j):
    """Device ids i and j exchange their points, consistently in every array (lists stay in id order)."""
    perm = np.arange(dev["points"])
    perm[[i, j]] = [j, i]                                     # new id of old id
    old_of_new = np.argsort(perm)
    lens = (dev["seg_hi"] - dev["seg_lo"]).astype(np.int64)
    pieces = [np.arange(dev["seg_lo"][o], dev["seg_hi"][o]) for o in old_of_new]
    move = np.concatenate(pieces)
    for k in ("vals", "ent"):
        dev[k] = dev[k][move]
    hi = np.cumsum(lens[old_of_new])
    dev["seg_hi"], dev["seg_lo"] = hi.astype(np.int32), (hi - lens[old_of_new]).astype(np.int32)
    dev["offset"] = perm[dev["offset"]].astype(np.int32)
    for k in ("n1", "n2"):
        t = dev[k][:, old_of_new].astype(np.int64)
        dev[k] = np.where(t >= 0, perm[np.maximum(t, 0)], -1).astype(np.int32)
    dev["nbr8"] = nbr8_from(dev["n1"], dev["n2"], dev["idbase"]).astype(np.int32)


def plant(dev, fault, sizes):
    """A copy of device-like arrays with one fault.  -> (dev, the stage that has to name it)"""
    d = copy.deepcopy(dev)
    D1, idbase = d["D1"], d["idbase"].astype(np.int64)
    both = np.argwhere((d["n1"] >= 0) & (d["n2"] >= 0) & (d["n1"] != d["n2"]))
    if fault == "neighbours swapped":
        j, p = both[len(both) // 2]
        d["n1"][j, p], d["n2"][j, p] = d["n2"][j, p], d["n1"][j, p]
        d["nbr8"] = nbr8_from(d["n1"], d["n2"], d["idbase"]).astype(np.int32)
        return d, "neighbours"
    if fault == "neighbour in the next image":
        j, p = 1, int(idbase[1]) // 2                        # a point of image 0; image 1 holds the same keys
        d["n1"][j, p] = idbase[1] + (d["n1"][j, p] if d["n1"][j, p] >= 0 else p)
        d["nbr8"] = nbr8_from(d["n1"], d["n2"], d["idbase"]).astype(np.int32)
        return d, "neighbours"
    if fault == "absent neighbour present":
        j, p = np.argwhere(d["n1"] < 0)[0]
        d["n1"][j, p] = p
        d["nbr8"] = nbr8_from(d["n1"], d["n2"], d["idbase"]).astype(np.int32)
        return d, "neighbours"
    long_ = int(np.argmax(d["seg_hi"] - d["seg_lo"] >= 8))    # a point with a list of eight or more
    if fault == "contributor dropped":
        e = int(d["seg_lo"][long_]) + 3
        d["vals"], d["ent"] = np.delete(d["vals"], e), np.delete(d["ent"], e)
        d["seg_hi"][long_:] -= 1
        d["seg_lo"][long_ + 1:] -= 1
        return d, "lists"
    if fault == "contributors exchanged":
        e = int(d["seg_lo"][long_]) + 2
        _swap(d["vals"], e, e + 1)
        _swap(d["ent"], e, e + 1)
        return d, "lists"
    if fault == "seg_hi off by one":
        d["seg_hi"][long_] += 1
        return d, "lists"
    if fault == "normaliser of the neighbouring pixel":
        nxt = np.minimum(d["ent"]["pixel"].astype(np.int64) + 1, len(d["norm"]) - 1)
        e = int(np.argmax(d["norm"][d["ent"]["pixel"]] != d["norm"][nxt]))
        d["ent"]["nr"][e] = d["norm"][nxt[e]]
        return d, "lists"
    if fault == "nbr8.dd along the wrong axis":
        # dd = the second-axis n2 neighbour's n2 along the pair's FIRST axis; planted: along its second axis
        n2 = d["n2"].astype(np.int64)
        pd = n2[1]
        wrong = np.where(pd >= 0, n2[1][np.maximum(pd, 0)], -1)
        lo = np.repeat(idbase[:-1], np.diff(idbase))
        wrong = np.where(wrong >= 0, wrong - lo, -1)
        p = int(np.argmax(wrong != d["nbr8"][0, :, 7]))
        assert wrong[p] != d["nbr8"][0, p, 7]
        d["nbr8"][0, p, 7] = wrong[p]
        return d, "nbr8"
    if fault == "ids against the Z-order":
        _renumber(d, int(idbase[2]) + 3, int(idbase[2]) + 4)
        return d, "numbering"
    if fault == "bary one ulp off":
        e = len(d["bary"]) // 2
        d["bary"][e] = np.nextafter(d["bary"][e], F32(2))
        return d, "embed"
    raise ValueError(fault)


BUILD_FAULTS = ("neighbours swapped", "neighbour in the next image", "absent neighbour present", "contributor dropped",
                "contributors exchanged", "seg_hi off by one", "normaliser of the neighbouring pixel", "nbr8.dd along the wrong axis",
                "ids against the Z-order", "bary one ulp off")


def splat_descending(ref, planes):
    """reference_stages' splat with every list summed in DESCENDING (pixel, vertex) order."""
    x = np.ascontiguousarray(planes.T, dtype=F32) * norm_of(ref)[:, None]
    values = np.zeros((ref.M + 1, x.shape[1]), F32)
    o = (ref.offset + 1).reshape(-1)
    np.add.at(values, o[::-1], (ref.bary.reshape(-1, 1) * np.repeat(x, ref.d + 1, axis=0))[::-1])
    return values[1:]
