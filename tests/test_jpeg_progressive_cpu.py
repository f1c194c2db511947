"""CPU: the host half of the progressive JPEG decoder (pnp_ovss.jpeg.parse_progressive / pack_scans) and the test writer it is
checked with (_jpeg_progressive.py).  Pillow is the reference: the writer's files decode, in Pillow, to the pixels of the
baseline stream their coefficients came from; the packed descriptors, decoded by the pure-Python reference decoder, give those
coefficients back; and what the device does not restate is refused with UnsupportedJpeg."""
import numpy as np
import pytest

import _jpeg_progressive as P
import _jpeg_streams as S
from oracle import jpeg_np as J
from pnp_ovss import jpeg as PJ


def _check_packed(files, sources):
    """decode_packed(pack_scans(files)) against the quantised coefficients of `sources`: everything on the blocks a
    one-component scan covers, the DC everywhere an interleaved DC scan reaches."""
    data, imgs, tabs, scans, segs, groups, sizes, tot = PJ.pack_scans(files)
    got = P.decode_packed(data, imgs, tabs, scans, segs)
    for i, (f, src) in enumerate(zip(files, sources)):
        j, q = S.quantised(src)
        cov = P.covered(j["frame"])
        interleaved_dc = any(sc.image == i and sc.kind in (0, 1) and sc.ncomp > 1 for sc in scans) or len(q) == 1
        assert sizes[i] == (j["frame"]["H"], j["frame"]["W"])
        for c, qc in enumerate(q):
            assert got[i][c].shape == qc.shape
            assert np.array_equal(got[i][c][cov[c]], qc[cov[c]]), f"image {i} component {c}: covered blocks differ"
            if interleaved_dc:
                assert np.array_equal(got[i][c][..., 0], qc[..., 0]), f"image {i} component {c}: DC of the padded grid differs"
            if PJ.is_progressive(f):
                assert not got[i][c][~cov[c]][:, 1:].any(), f"image {i} component {c}: AC written outside the scan's blocks"
    return data, imgs, tabs, scans, segs, groups, tot


# ------------------------------------------------------------------------------------------ the writer against libjpeg
def test_writer_files_decode_to_the_source_pixels_in_pillow():
    for name, src, data in P.script_cases() + P.restart_cases():
        assert np.array_equal(S.pillow_rgb(data), S.pillow_rgb(src)), name
    src, a, b = P.dense_case()
    assert np.array_equal(S.pillow_rgb(a), S.pillow_rgb(src)) and np.array_equal(S.pillow_rgb(b), S.pillow_rgb(src))


@pytest.mark.parametrize("sampling,h,w", [("420", 37, 53), ("422", 33, 70), ("444", 16, 24), ("gray", 27, 43)])
def test_pillow_progressive_equals_its_baseline(sampling, h, w):
    """Pillow's progressive file holds the coefficients of its baseline file (same quality, same subsampling): same pixels, and
    the baseline's coefficients out of the packed progressive scans."""
    img = S.noisy_image(h, w, 7)
    kw = dict(quality=80) if sampling == "gray" else dict(quality=80, subsampling={"444": 0, "422": 1, "420": 2}[sampling])
    base, prog = P.pillow_pair(img[..., 1] if sampling == "gray" else img, **kw)
    assert np.array_equal(S.pillow_rgb(prog), S.pillow_rgb(base))
    j = PJ.parse_progressive(prog)
    assert len(j["scans"]) == (6 if sampling == "gray" else 10)
    got = [(tuple(s["comps"]), s["Ss"], s["Se"], s["Ah"], s["Al"]) for s in j["scans"]]
    assert got == P.pillow_script(len(j["comps"]))
    _check_packed([prog], [base])


# ------------------------------------------------------------------------------------------ the host half
def test_packed_scans_hold_the_source_coefficients():
    cases = P.script_cases()
    _check_packed([d for _, _, d in cases], [s for _, s, _ in cases])
    for k in (0, 7, 20, len(cases) - 4, len(cases) - 3):
        _check_packed([cases[k][2]], [cases[k][1]])


def test_packed_restart_intervals():
    cases = P.restart_cases()
    data, imgs, tabs, scans, segs, groups, tot = _check_packed([d for _, _, d in cases], [s for _, s, _ in cases])
    # 40 x 24 at 4:2:0, DRI 1: 2 x 3 MCUs in the interleaved DC scans, 3 x 5 real luma blocks of the 4 x 6 the plane holds
    per_scan = {}
    for g in segs:
        if g.image == 0:
            per_scan[scans[g.scan].ordinal] = per_scan.get(scans[g.scan].ordinal, 0) + 1
    assert per_scan == {0: 6, 1: 15, 2: 6, 3: 6, 4: 15, 5: 15, 6: 6, 7: 6, 8: 6, 9: 15}
    luma_ac = [sc for sc in scans if sc.image == 0 and sc.ordinal == 1][0]
    assert (luma_ac.bw, luma_ac.bh, imgs[0].bx[0], imgs[0].by[0]) == (3, 5, 4, 6)


def test_mixed_batch_layout():
    """Baseline, progressive, grey and restart files in one batch: baseline segments first, then groups by scan ordinal; image
    descriptors and totals as pack_batch lays them out."""
    base = S.table_case("unary", "luma1", "422")[1]
    rst = S.restart_cases()["dri7"][1]
    cases = P.script_cases()
    files = [cases[3][2], base, cases[30][2], rst, P.restart_cases()[0][2]]
    sources = [cases[3][1], S.table_case("unary", "luma1", "422")[0], cases[30][1], S.restart_cases()["dri7"][0], P.restart_cases()[0][1]]
    data, imgs, tabs, scans, segs, groups, tot = _check_packed(files, sources)
    nb = tot["base_segments"]
    assert nb == 1 + 4 and all(scans[g.scan].kind == 0 for g in segs[:nb]) and all(scans[g.scan].kind for g in segs[nb:])
    d1, i1, t1, s1, z1, tot1 = PJ.pack_batch([base, rst])
    for a, b in ((imgs[1], i1[0]), (imgs[3], i1[1])):
        assert (a.H, a.W, a.ncomp, list(a.bx), list(a.by), a.data_len) == (b.H, b.W, b.ncomp, list(b.bx), list(b.by), b.data_len)
    end = 0
    for k, (first, count, kind, ordinal) in enumerate(groups.tolist()):
        assert first == (nb if k == 0 else end) and count > 0
        assert all(scans[g.scan].kind == kind and scans[g.scan].ordinal == ordinal for g in segs[first:first + count])
        end = first + count
    assert end == len(segs)
    assert [g[3] for g in groups.tolist()] == sorted(g[3] for g in groups.tolist())
    off = 0
    for im, (h, w) in zip(imgs, [S.pillow_rgb(f).shape[:2] for f in files]):
        assert im.rgb_off == off
        off += h * w * 3
    assert off == tot["rgb_bytes"]


def test_dense_history_streams():
    src, a, b = P.dense_case()
    _check_packed([a, b], [src, src])


def test_run_that_outlasts_the_bits_of_its_segment():
    """The refinement scan of aligned_run_case ends on a byte boundary inside an end-of-band run: its last eight blocks have
    no bit at all."""
    src, data = P.aligned_run_case()
    assert P.PAD_BITS[data][-1] == 0 and np.array_equal(S.pillow_rgb(data), S.pillow_rgb(src))
    j, q = S.quantised(src)
    assert not q[0][2:, :, 1:].any() and q[0][:2, :, 1:].any()
    _check_packed([data], [src])


# ------------------------------------------------------------------------------------------ refusals
def _sos_offsets(data):
    """Offsets of every SOS marker of a file this module's writer produced (walks the marker segments)."""
    out, pos = [], 2
    while pos < len(data):
        assert data[pos] == 0xFF
        m = data[pos + 1]
        if m == 0xD9:
            break
        L = (data[pos + 2] << 8) | data[pos + 3]
        if m == 0xDA:
            out.append(pos)
            pos += 2 + L
            while not (data[pos] == 0xFF and data[pos + 1] != 0 and not 0xD0 <= data[pos + 1] <= 0xD7):
                pos += 1
        else:
            pos += 2 + L
    return out


def _refusal_cases():
    src = P.small_source("420", 24, 40)
    good = P.recode_progressive(src, P.pillow_script(3))
    sos = _sos_offsets(good)
    assert len(sos) == 10
    cut = good[:sos[-1] - len(P.PROG_AC[1]) - 21]             # the last scan and the DHT segment in front of it
    assert cut[-2:] != b"\xff\xd9" and good[len(cut):len(cut) + 2] == b"\xff\xc4"
    bad_ah = P.recode_progressive(src, [((0, 1, 2), 0, 0, 0, 2), ((0, 1, 2), 0, 0, 1, 0)] + [((c,), 1, 63, 0, 0) for c in range(3)])
    two = bytearray(P.recode_progressive(src, P.spectral_script(3)))
    p = _sos_offsets(bytes(two))[1]                           # the first AC scan: claim two components in its header
    hdr = bytes((0xFF, 0xDA, 0, 10, 2, 1, 0x00, 2, 0x11, 1, 5, 0))
    two_comp = bytes(two[:p]) + hdr + bytes(two[p + 10:])
    many = P.recode_progressive(src, [((0, 1, 2), 0, 0, 0, 0)] + [((c,), k, k, 0, 0) for c in range(3) for k in range(1, 22)] +
                                [((c,), 22, 63, 0, 0) for c in range(3)])
    three = P.recode_progressive(src, P.pillow_script(3), table_ids=((0, 1, 2), (0, 1, 1)))
    return {"last refinement scan removed": cut + b"\xff\xd9", "Ah is not the previous Al": bad_ah, "AC scan of two components": two_comp,
            "more than MAX_SCANS scans": many, "three DC tables in one scan": three}


@pytest.mark.parametrize("name", ["last refinement scan removed", "Ah is not the previous Al", "AC scan of two components",
                                  "more than MAX_SCANS scans", "three DC tables in one scan"])
def test_refusals(name):
    data = _refusal_cases()[name]
    assert PJ.MAX_SCANS == 64
    with pytest.raises(PJ.UnsupportedJpeg):
        PJ.parse_progressive(data)
    with pytest.raises(PJ.UnsupportedJpeg):
        PJ.pack_scans([data])


def test_more_refusals():
    src = P.small_source("420", 24, 40)
    for script in ([((0,), 1, 63, 0, 0), ((0, 1, 2), 0, 0, 0, 0), ((1,), 1, 63, 0, 0), ((2,), 1, 63, 0, 0)],      # AC before its DC
                   [((0, 1, 2), 0, 0, 0, 0), ((0,), 1, 63, 1, 0), ((1,), 1, 63, 0, 0), ((2,), 1, 63, 0, 0)],      # a band's first scan with Ah != 0
                   [((0, 1, 2), 0, 0, 0, 0), ((0,), 1, 63, 0, 0), ((1,), 1, 63, 0, 0)],                           # a component without AC
                   [((0, 1, 2), 0, 0, 0, 0), ((0,), 1, 63, 0, 0), ((0,), 5, 9, 0, 0), ((1,), 1, 63, 0, 0), ((2,), 1, 63, 0, 0)]):
        with pytest.raises(PJ.UnsupportedJpeg):
            PJ.parse_progressive(P.recode_progressive(src, script))
    good = P.recode_progressive(src, P.pillow_script(3))
    for bad in (good[:40], b"", good[:2] + b"\x00" + good[3:], S.table_source("420")):
        with pytest.raises(PJ.UnsupportedJpeg):
            PJ.parse_progressive(bad)


def test_exactly_max_scans_is_accepted():
    src = P.small_source("gray", 17, 17)
    script = [((0,), 0, 0, 0, 0)] + [((0,), k, k, 0, 0) for k in range(1, 63)] + [((0,), 63, 63, 0, 0)]
    assert len(script) == PJ.MAX_SCANS
    _check_packed([P.recode_progressive(src, script)], [src])


# ------------------------------------------------------------------------------------------ the existing parsers
def test_parse_and_pack_batch_still_refuse_progressive():
    _, prog = P.pillow_pair(S.noisy_image(16, 24, 1), quality=75)
    assert PJ.is_progressive(prog) and not PJ.is_progressive(S.table_source("420"))
    with pytest.raises(PJ.UnsupportedJpeg, match="SOF2"):
        PJ.parse(prog)
    with pytest.raises(PJ.UnsupportedJpeg, match="SOF2"):
        PJ.pack_batch([S.table_source("444"), prog])
    with pytest.raises(J.JpegError):
        J.parse_jpeg(prog)
