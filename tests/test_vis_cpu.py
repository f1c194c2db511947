"""CPU: the semantics of the output side, pinned without a device -- the numpy restatement of libjpeg's baseline encoder
(_vis_refs.py) equals Pillow's bytes on every image the GPU tests use, three planted faults each break that equality, the
overlay restatement has the properties the kernel documents, and the host halves (markers, argument checks, command line)
behave."""
import os
import sys

import numpy as np
import pytest

import _vis_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("quality", (30, 75, 95))
def test_encoder_restatement_equals_pillow(quality):
    bad = []
    for (H, W) in R.SIZES:
        for kind in R.CONTENTS:
            img = R.test_image(kind, H, W)
            if R.jpeg_encode_ref(img, quality) != R.pillow_jpeg(img, quality):
                bad.append((kind, H, W))
    assert not bad, bad


def _zrl_runs(Z):
    n = 0
    for b in Z:
        nz = np.flatnonzero(b[1:] != 0) + 1
        n += int((np.diff(np.concatenate([[0], nz])) - 1 >= 16).sum())
    return n


def test_test_images_reach_the_hard_cases():
    """The contents promise stuffed bytes, ZRL runs, DC-only blocks and the largest categories a Pillow file can hold: check
    that they deliver (size 10 for AC; size 10 for DC too -- at quality <= 95 the DC quantiser is >= 2, |difference| <= 1020)."""
    Z, _, _ = R.jpeg_coefficients_ref(R.test_image("noise", 37, 29), 95)
    raw, stuffed = R.entropy_code_ref(Z)
    assert raw.count(b"\xff") == len(stuffed) - len(raw) >= 3
    assert _zrl_runs(R.jpeg_coefficients_ref(R.test_image("noise", 37, 29), 30)[0]) >= 1
    assert _zrl_runs(R.jpeg_coefficients_ref(R.test_image("smooth", 17, 33), 75)[0]) >= 1
    Z, _, _ = R.jpeg_coefficients_ref(R.test_image("checker", 16, 16), 95)
    assert 512 <= np.abs(Z[:, 1:]).max() < 1024, "no size-10 AC coefficient"
    assert abs(int(Z[1, 0]) - int(Z[0, 0])) == 512, "no size-10 DC difference"
    for kind in ("white", "black"):
        Zf, _, _ = R.jpeg_coefficients_ref(R.test_image(kind, 16, 16), 75)
        assert Zf[0, 0] != 0 and not Zf[:, 1:].any()                # DC-only blocks


@pytest.mark.parametrize("fault,sizes", [("fault_bias", ((16, 16), (375, 500))),           # constant bias instead of 1, 2, 1, 2
                                         ("fault_rows", ((24, 40), (40, 24))),             # pad full-resolution rows (H % 16 == 8)
                                         ("fault_dummy", ((37, 29), (9, 50), (1, 1)))])    # dummy blocks with DC 0
def test_planted_faults_break_the_equality(fault, sizes):
    for (H, W) in sizes:
        img = R.test_image("smooth", H, W)
        assert R.jpeg_encode_ref(img, 75) == R.pillow_jpeg(img, 75)
        assert R.jpeg_encode_ref(img, 75, **{fault: True}) != R.pillow_jpeg(img, 75), (fault, H, W)


def test_host_markers_and_tables_equal_the_restatement():
    from pnp_ovss import jpeg as J
    for q in (1, 30, 49, 50, 75, 95):
        t = J.quality_tables(q)
        assert t.dtype == np.uint16 and t.shape == (2, 64) and t.min() >= 1 and t.max() <= 255
        np.testing.assert_array_equal(t[0], R.quant_table(R.STD_LUMA_Q, q))
        np.testing.assert_array_equal(t[1], R.quant_table(R.STD_CHROMA_Q, q))
        assert J.encode_headers(375, 500, t) == R.jpeg_headers_ref(375, 500, t[0], t[1])
    img = R.test_image("smooth", 17, 33)
    Z, ql, qc = R.jpeg_coefficients_ref(img, 75)
    scan = R.entropy_code_ref(Z)[1]
    assert J.encode_headers(17, 33, J.quality_tables(75)) + scan + b"\xff\xd9" == R.pillow_jpeg(img, 75)
    for q in (0, 96):
        with pytest.raises(ValueError):
            J.quality_tables(q)
    with pytest.raises(ValueError):
        J.encode_headers(0, 5, J.quality_tables(75))
    # the worst-case capacity really bounds the longest block: 20 + 63 * 26 bits, every byte stuffed
    assert J.scan_capacity(16, 16, worst=True) >= 2 * 6 * ((20 + 63 * 26 + 7) // 8)
    assert J.scan_capacity(375, 500) >= 375 * 500 * 3 // 2


def test_overlay_restatement_properties():
    from pnp_ovss import vis
    pal = vis.default_palette()
    np.testing.assert_array_equal(pal, R.default_palette_ref())
    assert tuple(pal[1]) == (255, 0, 0) and tuple(pal[2]) == (0, 0, 255) and tuple(pal[5]) == (0, 128, 0)
    assert tuple(pal[10]) == (154, 205, 50) and tuple(pal[11]) == (255, 0, 0) and tuple(pal[255]) == tuple(pal[(255 - 1) % 10 + 1])
    rng = np.random.default_rng(3)
    rgb = rng.integers(0, 256, (6, 9, 3), dtype=np.uint8)
    rgb[0, 0] = R.TRUNCATION_WITNESS_RGB
    lab = rng.integers(0, 12, (6, 9), dtype=np.uint8)
    lab[0, 0] = 0
    out = R.overlay_ref(lab, rgb)
    bg = lab == 0
    assert (out[bg][:, 0] == out[bg][:, 1]).all() and (out[bg][:, 1] == out[bg][:, 2]).all()      # label 0: grey
    # truncation, not rounding: grey of (255, 255, 0) is 236.6145
    g = (0.2125 * 255 + 0.7154 * 255) / 255 * 255
    assert int(g) == 236 and round(g) == 237 and tuple(out[0, 0]) == (236, 236, 236)
    # palette indexing: on a black image a label's pixel is its colour times alpha, truncated
    black = np.zeros((1, 255, 3), dtype=np.uint8)
    labs = np.arange(1, 256, dtype=np.uint8)[None, :]
    o = R.overlay_ref(labs, black)
    want = ((pal[1:].astype(np.float64) / 255 * 0.3 + 0.0 * (1 - 0.3)) * 255).astype(np.uint8)
    np.testing.assert_array_equal(o[0], want)
    assert tuple(o[0, 0]) == (76, 0, 0)                           # 0.3 * 255 = 76.5 -> 76
    # a class keeps its colour whatever else the image holds (the reference ranks the labels present)
    a = R.overlay_ref(np.array([[7, 0]], dtype=np.uint8), rgb[:1, :2])
    b = R.overlay_ref(np.array([[7, 3]], dtype=np.uint8), rgb[:1, :2])
    assert tuple(a[0, 0]) == tuple(b[0, 0])


def test_segment_in_the_wild_refuses_bad_lists_without_a_device():
    from pnp_ovss import wild
    img = np.zeros((8, 8, 3), dtype=np.uint8)
    with pytest.raises(ValueError, match="one list per image"):
        wild.segment_in_the_wild(None, None, [img, img], [["cat"]])
    with pytest.raises(ValueError, match="non-empty list"):
        wild.segment_in_the_wild(None, None, [img, img], [["cat"], []])
    with pytest.raises(ValueError, match="non-empty list"):
        wild.segment_in_the_wild(None, None, [img], ["cat"])
    with pytest.raises(ValueError, match="ids"):
        wild.segment_in_the_wild(None, None, [img], [["cat"]], ids=["a", "b"])
    with pytest.raises(ValueError, match="at most 255"):
        wild.segment_in_the_wild(None, None, [img], [[f"c{i}" for i in range(256)]])
    assert wild.captions_of([["eiffeltower", "merrygoround"]]) == ["A picture of eiffeltower merrygoround"]
    assert wild.vis_file_name("out", "N_drop", "paris", "blur+crf") == "out/0519_Segmentation/BLIP_N_drop_paris_blur+crf.jpeg"


def test_cli_parser_and_wild_class_table(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "pnp-ovss_amd"))
    import PnP_OVSS_0514_updated_segmentation as cli
    from pnp_ovss import wild
    a = cli.get_args_parser().parse_args([])
    assert a.in_the_wild is False and a.wild_classes is None and a.save_vis is False          # everything off unless asked for
    a = cli.get_args_parser().parse_args(["--in_the_wild", "--wild_classes", "names.json", "--save_vis"])
    assert a.in_the_wild and a.wild_classes == "names.json" and a.save_vis
    (tmp_path / "In_the_wild").mkdir()
    for n in ("b.jpg", "a.jpeg", "c.png"):
        (tmp_path / "In_the_wild" / n).write_bytes(b"")
    found = wild.list_wild_images(str(tmp_path))
    assert [i for i, _ in found] == ["a", "b"]
    (tmp_path / "names.json").write_text('{"a": ["dog", "grass"]}')
    with pytest.raises(SystemExit, match=r"\['b'\]"):
        wild.load_wild_classes(str(tmp_path / "names.json"), ["a", "b"])
    with pytest.raises(SystemExit, match="--wild_classes"):
        wild.load_wild_classes(None, ["a"])
    assert wild.load_wild_classes(str(tmp_path / "names.json"), ["a"]) == [["dog", "grass"]]
