"""CPU: the JPEG input path on streams Pillow's encoder never writes -- the test stream writer itself (_jpeg_streams.py)
against Pillow, the host packer (pnp_ovss.jpeg.parse / pack_batch) against the oracle's parser, and the oracle
(oracle/jpeg_np.py) against Pillow on the narrow images where libjpeg leaves its fancy chroma upsampling."""
import re

import numpy as np
import pytest

import _jpeg_streams as S
from oracle import jpeg_np as J
from pnp_ovss import jpeg as PJ


def _roundtrip(name, src, data):
    ref = S.pillow_rgb(data)
    assert np.array_equal(ref, S.pillow_rgb(src)), f"{name}: Pillow decodes the re-coded stream to other pixels than its source"
    assert np.array_equal(J.decode(data), ref), f"{name}: oracle != Pillow"


# ------------------------------------------------------------------------------------------ the writer
def test_table_sets_are_legal_and_as_described():
    for dc, ac in S.TABLE_SETS.values():
        S.check_tables_legal(*dc)
        S.check_tables_legal(*ac)
        assert sorted(dc[1]) == list(range(12)) and sorted(ac[1]) == sorted(S.STD_AC[1]) and len(ac[1]) == 162
    assert S.UNARY_DC[0] == [1] * 12 + [0] * 4                                   # two codes longer than 10 bits
    assert S.SKEWED_AC[0] == [1] * 8 + [0] * 7 + [154]
    assert S.FLAT_DC[0][3] == 12 and sum(S.FLAT_DC[0]) == 12 and S.FLAT_AC[0][7] == 162 and sum(S.FLAT_AC[0]) == 162


@pytest.mark.parametrize("sampling", S.SAMPLINGS)
def test_writer_roundtrip_table_cases(sampling):
    for tset, assign, s in S.TABLE_CASES:
        if s == sampling:
            src, data = S.table_case(tset, assign, s)
            _roundtrip((tset, assign, s), src, data)
            assert data.count(b"\xff\xc4") >= (1 if assign == "one_dht" else 2)


def test_writer_roundtrip_restart_dressing_geometry():
    for name, (src, data) in S.restart_cases().items():
        _roundtrip(name, src, data)
    for name, (src, data) in S.dressing_cases().items():
        _roundtrip(name, src, data)
    for name, data in S.geometry_cases():
        assert np.array_equal(J.decode(data), S.pillow_rgb(data)), f"{name}: oracle != Pillow"
        if name.endswith("gray2x2"):
            h, w = (int(v) for v in name.split()[0].split("x"))
            _roundtrip(name, S.source(h, w, "gray", 92, seed=20 + S.GEOMETRY_SIZES.index((h, w))), data)


def test_writer_roundtrip_long_streams():
    for name, (src, data) in S.long_streams().items():
        _roundtrip(name, src, data)
    src, data = S.flat_stream()
    _roundtrip("flat", src, data)


def test_long_stream_input_conditions():
    """Conditions on the INPUT of the all-sub-sequences-live GPU case, not measurements: see S.long_streams."""
    props = {name: S.stream_properties(data) for name, (_, data) in S.long_streams().items()}
    print("[measured] jpeg long streams:", props)
    for name in ("skewed_19k", "skewed_4k"):                # a stuffed FF at the end of a 16-byte slice and of a 4096-byte chunk
        p = props[name]
        assert p["segments"] == 1 and p["stuffed_mod16_15"] >= 2 and p["stuffed_mod4096_4095"] >= 1, (name, p)
    p = props["skewed_19k"]
    assert p["sub_bits"] > 128 and p["live"] > 14 * 64 and 19000 <= p["raw_len"] <= 20480, p
    p = props["skewed_4k"]
    assert 4096 < p["raw_len"] < 4500 and p["live"] < 1024 and p["sub_bits"] == 128, p
    p = props["all_live"]
    assert p["live"] == 1024 and p["sub_bits"] > 128 and p["segments"] == 1, p
    src, data = S.flat_stream()
    p = S.stream_properties(data)
    assert p["segments"] == 1 and p["live"] >= 64, p


def test_undefined_code_stream_differs_in_one_byte():
    """The corrupt input of the GPU error test: the flat-table stream with one scan byte changed; the packer still takes it
    (the markers are intact), the oracle refuses it."""
    _, data = S.flat_stream()
    bad = S.undefined_ac_code_stream()
    j = J.parse_jpeg(data)
    diff = [i for i in range(len(data)) if data[i] != bad[i]]
    assert len(bad) == len(data) and len(diff) == 1 and data.index(j["scan"]) <= diff[0] < data.index(j["scan"]) + len(j["scan"])
    assert bad[diff[0]] == 0xA2 > 161                       # as an aligned 8-bit AC code: above the 162 codes the table defines
    with pytest.raises(J.JpegError):
        J.decode(bad)
    _, _, _, segs, _, _ = PJ.pack_batch([bad])
    assert len(segs) == 1 and segs[0].raw_len == len(j["scan"])


# ------------------------------------------------------------------------------------------ the host packer
def _rst_split(scan, dri, nmcu):
    """Independent restatement of the segment list: (offset, length, first MCU, MCU count) per restart interval."""
    if not dri:
        return [(0, len(scan), 0, nmcu)]
    marks = [m.start() for m in re.finditer(rb"\xff[\xd0-\xd7]", scan)]
    nseg = -(-nmcu // dri)
    out = []
    for k in range(nseg):
        s0 = 0 if k == 0 else marks[k - 1] + 2
        s1 = marks[k] if k < len(marks) else len(scan)
        if k:
            assert scan[s0 - 1] == 0xD0 + ((k - 1) & 7), "RSTn out of sequence in the test stream"
        out.append((s0, s1 - s0, k * dri, min(dri, nmcu - k * dri)))
    return out


def check_pack(files):
    """pack_batch against the oracle's parser: geometry, quantisation and Huffman tables by the ids the scan names, the scan
    bytes and the restart segments."""
    data, imgs, tabs, segs, sizes, tot = PJ.pack_batch(files)
    assert len(imgs) == len(files) == len(sizes)
    seg_i, coef, plane, rgb, clean = 0, 0, 0, 0, 0
    for i, f in enumerate(files):
        j = J.parse_jpeg(f)
        hmax, vmax, mcux, mcuy = J.geometry(j["frame"])
        im, comps = imgs[i], j["frame"]["comps"]
        assert (im.H, im.W, im.ncomp, im.hmax, im.vmax, im.mcux, im.mcuy) == (j["frame"]["H"], j["frame"]["W"], len(comps), hmax, vmax, mcux, mcuy)
        assert sizes[i] == (im.H, im.W) and im.data_off % 16 == 0 and im.data_len == len(j["scan"]) and im.rgb_off == rgb
        assert bytes(data[im.data_off:im.data_off + im.data_len]) == j["scan"]
        t = tabs[im.tab]
        for ci, c in enumerate(comps):
            assert (im.h[ci], im.v[ci], im.bx[ci], im.by[ci]) == (c["h"], c["v"], mcux * c["h"], mcuy * c["v"])
            assert (im.coef_off[ci], im.plane_off[ci]) == (coef, plane)
            coef += im.bx[ci] * im.by[ci] * 64
            plane += im.bx[ci] * im.by[ci] * 64
            np.testing.assert_array_equal(np.array(t.quant[im.tq[ci]][:]), j["qt"][c["tq"]])
            for cls, tid in ((0, im.td[ci]), (1, im.ta[ci])):
                assert tid == (c["td"], c["ta"])[cls] and tid in (0, 1)
                counts, symbols = j["ht"][(cls, tid)]
                assert list(t.counts[cls * 2 + tid]) == list(counts) and list(t.vals[cls * 2 + tid][:len(symbols)]) == list(symbols)
        rgb += im.H * im.W * 3
        want = _rst_split(j["scan"], j["dri"], mcux * mcuy)
        for k, (off, raw, m0, nm) in enumerate(want):
            s = segs[seg_i + k]
            assert (s.image, s.byte_off, s.raw_len, s.mcu0, s.nmcu) == (i, off, raw, m0, nm), (i, k)
            assert s.clean_off == clean and s.clean_off % 16 == 0 and s.clean_cap >= s.raw_len + 32 and s.clean_cap % 16 == 0
            assert s.sub_bits % 32 == 0 and s.sub_bits >= 128 and s.sub_bits * PJ.SUBSEQUENCES >= s.raw_len * 8
            clean += s.clean_cap
        seg_i += len(want)
        assert sum(nm for _, _, _, nm in want) == mcux * mcuy
    assert seg_i == len(segs)
    assert (tot["coef_elems"], tot["plane_bytes"], tot["rgb_bytes"], tot["clean_bytes"]) == (coef, plane, rgb, clean)
    return imgs, segs


def test_packer_gray_with_2x2_factors_is_one_block_per_mcu():
    data = S.recode(S.source(37, 53, "gray", 80, seed=1), gray_factors=(2, 2))
    assert PJ.parse(data)["comps"][0]["h"] == PJ.parse(data)["comps"][0]["v"] == 1
    imgs, segs = check_pack([data])
    assert (imgs[0].mcux, imgs[0].mcuy, imgs[0].hmax, imgs[0].vmax, imgs[0].bx[0], imgs[0].by[0]) == (7, 5, 1, 1, 7, 5)
    assert segs[0].nmcu == 35


def test_packer_dressed_streams():
    cases = S.dressing_cases()
    imgs, segs = check_pack([d for _, d in cases.values()])
    names = list(cases)
    nseg = {n: sum(1 for s in segs if s.image == i) for i, n in enumerate(names)}
    nmcu = imgs[0].mcux * imgs[0].mcuy
    assert nmcu == 12
    # an appended file's RST markers open no segment: exactly the MCUs of the first file, by its own DRI
    assert nseg["second"] == nseg["second_dri_first_plain"] == nseg["junk"] == 1 and nseg["second_dri"] == 6
    for i, n in enumerate(names):
        assert sum(s.nmcu for s in segs if s.image == i) == nmcu, n
    src, junk = cases["junk"]
    assert PJ.parse(junk)["scan_end"] == PJ.parse(S.recode(src))["scan_end"]             # nothing behind EOI is scan data
    assert PJ.parse(cases["sof1_dqt16"][1])["qt"][0].max() <= 255 and b"\xff\xc1" in cases["sof1_dqt16"][1]
    assert [c["id"] for c in PJ.parse(cases["ids012"][1])["comps"]] == [0, 1, 2]
    assert cases["one_dht"][1].count(b"\xff\xc4") == 1 and len(PJ.parse(cases["one_dht"][1])["ht"]) == 4
    assert cases["fill"][1].count(b"\xff\xff\xff\xff") >= 6


def test_packer_adobe_transform():
    src = S.source(16, 16, "420", 80, seed=2)
    assert PJ.parse(S.recode(src, jfif=False, adobe=1))["W"] == 16
    for jfif in (False, True):                    # transform 0 = stored RGB; with a JFIF marker too, still refused (the safe side)
        with pytest.raises(PJ.UnsupportedJpeg):
            PJ.parse(S.recode(src, jfif=jfif, adobe=0))
        with pytest.raises(PJ.UnsupportedJpeg):
            PJ.pack_batch([src, S.recode(src, jfif=jfif, adobe=0)])


def test_packer_restart_intervals():
    cases = S.restart_cases()
    names = list(cases)
    imgs, segs = check_pack([d for _, d in cases.values()])
    nseg = {n: sum(1 for s in segs if s.image == i) for i, n in enumerate(names)}
    assert nseg == {"dri1": 25, "dri1_420": 15, "dri7": 4, "dri_row": 5, "dri_row_420": 3, "dri_all": 1, "dri_more": 1, "dri0": 1}
    one = [s for s in segs if s.image == names.index("dri1")]
    assert all(s.nmcu == 1 for s in one) and [s.mcu0 for s in one] == list(range(25))          # RSTn wrapped three times
    assert max(s.raw_len for s in one) < 16 < max(s.raw_len for s in segs if s.image == names.index("dri1_420"))
    assert [s.nmcu for s in segs if s.image == names.index("dri7")] == [7, 7, 7, 4]
    assert [s.nmcu for s in segs if s.image == names.index("dri_more")] == [15]


def test_packer_table_cases_share_tables_by_content():
    files = [S.table_case(*c)[1] for c in S.TABLE_CASES]
    imgs, _ = check_pack(files)
    keys = {}
    for c, im, f in zip(S.TABLE_CASES, imgs, files):
        j = J.parse_jpeg(f)
        key = (tuple(sorted((k, tuple(a), tuple(b)) for k, (a, b) in j["ht"].items())), tuple(sorted((k, q.tobytes()) for k, q in j["qt"].items())))
        assert keys.setdefault(key, im.tab) == im.tab, c
    assert len(set(keys.values())) == len(keys) == len({im.tab for im in imgs})
    check_pack([d for _, d in S.geometry_cases()])


# ------------------------------------------------------------------------------------------ the narrow-image rule
@pytest.mark.parametrize("ss", (0, 1, 2))
def test_oracle_matches_pillow_on_narrow_images(ss):
    """libjpeg upsamples the chroma planes with its fancy triangle filters only when their downsampled width exceeds 2
    (jdsample.c); up to width 4 it replicates.  Oracle against Pillow, every H x W here."""
    rng = np.random.default_rng(100 + ss)
    bad = []
    for H in (1, 2, 3, 12, 17):
        for W in (1, 2, 3, 4, 5, 6, 9):
            data = S.pillow_jpeg(rng.integers(0, 256, (H, W, 3), dtype=np.uint8), quality=95, subsampling=ss)
            ref = S.pillow_rgb(data)
            got = J.decode(data)
            if not np.array_equal(got, ref):
                bad.append((H, W, int(np.abs(got.astype(int) - ref).max())))
    assert not bad, f"subsampling {ss}: (H, W, max |oracle - Pillow|) = {bad}"
