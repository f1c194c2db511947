"""CPU: the host half of the label-map PNG files (pnp_ovss.png) and the reference encoder the GPU test compares the device's
bytes against (_png_refs.py, written from the format's description): zlib and Pillow read what the reference writes, the
package's chunk writer agrees with it, the capacity bound is the token layer's worst case, the C ABI refuses bad arguments
without a device, and the command line writes a PNG only when asked."""
import ctypes
import io
import os
import sys
import zlib

import numpy as np
import pytest

import _png_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _maps():
    rng = np.random.default_rng(5)
    two = np.zeros((2, 40), dtype=np.uint8)
    two[0, 10:] = 3
    two[1, 10:] = 3
    two[1, 25:] = 7
    return {
        "1x1": np.array([[5]], dtype=np.uint8),
        "3x7 random": rng.integers(0, 256, (3, 7), dtype=np.uint8),
        "constant 5x600": np.full((5, 600), 9, dtype=np.uint8),
        "two rows, Up wins": two,
        "high labels": np.array([[143, 144, 255, 255, 255, 255, 143]] * 3, dtype=np.uint8),
        "blob 60x80": R.blob_map(60, 80, 5, 1),
        "noise 33x65": rng.integers(0, 256, (33, 65), dtype=np.uint8),
    }


MAPS = _maps()


@pytest.mark.parametrize("name", sorted(MAPS))
def test_reference_stream_is_a_zlib_stream_of_the_filtered_rows(name):
    """zlib inflates the reference's stream to its filtered stream (which also checks the Adler-32), the stream starts 78 01,
    and un-filtering the rows gives the labels back."""
    lab = MAPS[name]
    H, W = lab.shape
    stream, filt, toks = R.zlib_stream(lab)
    assert stream[:2] == b"\x78\x01" and len(filt) == H * (W + 1)
    assert zlib.decompress(stream) == filt
    rows = np.frombuffer(filt, dtype=np.uint8).reshape(H, W + 1)
    assert set(rows[:, 0].tolist()) <= {0, 2} and rows[0, 0] == 0, "row 0 always gets filter 0"
    back = np.zeros((H, W), dtype=np.uint8)
    for y in range(H):
        back[y] = rows[y, 1:] if rows[y, 0] == 0 else rows[y, 1:] + (back[y - 1] if y else 0)
    assert np.array_equal(back, lab)
    assert sum(1 if k == "lit" else v for k, v in toks) == len(filt)
    assert all(3 <= v <= 258 for k, v in toks if k == "match")
    assert len(stream) <= R.stream_capacity_ref(H, W)


def test_reference_filter_choice_and_token_rules():
    lab = MAPS["two rows, Up wins"]
    _, filters = R.filtered_stream(lab)
    assert filters == [0, 2]                       # row 1: raw changes twice, its Up difference once
    # a run of length r: literal, (r - 1) // 258 full matches, then a match of t >= 3 or t literals
    for r, want in ((1, [("lit", 7)]), (2, [("lit", 7)] * 2), (3, [("lit", 7)] * 3), (4, [("lit", 7), ("match", 3)]),
                    (259, [("lit", 7), ("match", 258)]), (260, [("lit", 7), ("match", 258), ("lit", 7)]),
                    (262, [("lit", 7), ("match", 258), ("match", 3)]), (775, [("lit", 7)] + [("match", 258)] * 3)):
        assert R.tokens_of(bytes([7] * r), 1, r - 1) == want, r
    # runs never cross a row
    assert R.tokens_of(bytes([0] * 8), 2, 3) == [("lit", 0), ("match", 3)] * 2


@pytest.mark.parametrize("palette", ["voc", "overlay", "random", None])
def test_reference_files_open_in_pillow_and_chunk_writer_agrees(palette):
    from PIL import Image
    from pnp_ovss import png, vis
    pal = {"voc": R.voc_palette_ref(), "overlay": vis.default_palette(), None: None,
           "random": np.random.default_rng(3).integers(0, 256, (256, 3), dtype=np.uint8)}[palette]
    np.testing.assert_array_equal(png.voc_palette(), R.voc_palette_ref())
    assert [tuple(v) for v in png.voc_palette()[:4]] == [(0, 0, 0), (128, 0, 0), (0, 128, 0), (128, 128, 0)]
    for name, lab in MAPS.items():
        H, W = lab.shape
        filt, toks, data = R.encode(lab, pal)
        Image.open(io.BytesIO(data)).verify()
        im = Image.open(io.BytesIO(data))
        assert im.size == (W, H) and im.mode == ("L" if pal is None else "P"), name
        assert np.array_equal(np.asarray(im), lab), name
        if pal is not None:
            assert np.array_equal(np.asarray(im.getpalette(), dtype=np.uint8).reshape(-1, 3), pal), name
        stream = R.zlib_stream(lab)[0]
        arg = pal if palette in ("random", None) else palette
        assert png.encode_chunks(H, W, stream, arg) == data, name
    assert png.encode_chunks(1, 1, R.zlib_stream(MAPS["1x1"])[0], "grey") == R.encode(MAPS["1x1"], None)[2]
    with pytest.raises(ValueError):
        png.encode_chunks(1, 1, b"", "rainbow")
    with pytest.raises(ValueError):
        png.encode_chunks(1, 1, b"", np.zeros((16, 3), dtype=np.uint8))
    with pytest.raises(ValueError):
        png.encode_chunks(0, 1, b"", None)


@pytest.mark.parametrize("H,W", [(1, 1), (3, 7), (5, 64), (33, 65)])
def test_stream_capacity_is_the_all_literal_length(H, W):
    """A stream of H (W + 1) bytes, no two neighbours equal, every byte >= 144, costs 9 bits per byte: exactly the bound."""
    from pnp_ovss import png
    filt = R.all_literal_stream(H, W)
    assert min(filt) >= 144 and all(a != b for a, b in zip(filt, filt[1:]))
    stream = R.stream_of_filtered(filt, H, W)
    assert zlib.decompress(stream) == filt
    assert png.stream_capacity(H, W) == len(stream) == R.stream_capacity_ref(H, W) == 2 + -(-(10 + 9 * H * (W + 1)) // 8) + 4


class _Img(ctypes.Structure):
    _fields_ = [("labels_off", ctypes.c_int64), ("out_off", ctypes.c_int64), ("H", ctypes.c_int32), ("W", ctypes.c_int32),
                ("out_cap", ctypes.c_int32), ("pad", ctypes.c_int32)]


def test_c_abi_refusals_and_workspace_query_without_a_device():
    """pnp_png_encode's argument checks sit in front of any HIP call: PNP_ERR_ARG = -22 for a null pointer, H or W outside
    1..65535, a negative capacity or offset and more than 2^31 / 9 filtered bytes in a call; d_ws = NULL answers ws_need."""
    from pnp_ovss import hip, png
    lib = hip.load_library()
    f = lib.pnp_png_encode
    assert ctypes.sizeof(hip.PnpPngImage) == ctypes.sizeof(_Img) == 32
    assert [n for n, _ in hip.PnpPngImage._fields_] == [n for n, _ in _Img._fields_]
    need = ctypes.c_int64(-1)
    p = ctypes.c_void_p(4096)                      # never dereferenced: every call below is answered on the host

    def query(*imgs):
        arr = (_Img * len(imgs))(*[_Img(*i) for i in imgs])
        return f(None, arr, len(imgs), None, None, None, None, 0, ctypes.byref(need), None)

    assert query((0, 0, 375, 500, png.stream_capacity(375, 500), 0)) == 0
    one = need.value
    assert one > 375 * 501 + png.stream_capacity(375, 500) and one % 256 == 0
    assert query((0, 0, 375, 500, 0, 0), (375 * 500, 0, 375, 500, 0, 0)) == 0 and one < need.value <= 2 * one
    assert query((0, 0, 65535, 3639, 0, 0)) == 0                                  # 238 547 400 filtered bytes: just inside
    assert png.MAX_STREAM_BYTES == (1 << 31) // 9 and 65535 * 3640 <= png.MAX_STREAM_BYTES < 65535 * 3641
    for bad in ((0, 0, 0, 5, 10, 0), (0, 0, 5, 0, 10, 0), (0, 0, 65536, 5, 10, 0), (0, 0, 5, 65536, 10, 0), (0, 0, -1, 5, 10, 0),
                (0, 0, 5, 5, -1, 0), (-1, 0, 5, 5, 10, 0), (0, -1, 5, 5, 10, 0), (0, 0, 65535, 3640, 10, 0)):
        assert query(bad) == -22, bad
        assert query((0, 0, 4, 4, 64, 0), bad) == -22, bad
    assert query((0, 0, 65535, 1820, 0, 0), (0, 0, 65535, 1820, 0, 0)) == -22      # the sum counts, not the single image
    arr = (_Img * 1)(_Img(0, 0, 4, 4, 64, 0))
    assert f(None, None, 1, None, None, None, None, 0, ctypes.byref(need), None) == -22       # no descriptors
    assert f(None, arr, 0, None, None, None, None, 0, ctypes.byref(need), None) == -22        # no images
    assert f(None, arr, 1, None, None, None, None, 0, None, None) == -22                      # neither a workspace nor a question
    assert query((0, 0, 4, 4, 64, 0)) == 0
    ws = need.value
    for args in ((None, arr, 1, p, p, p, p, ws, None, None), (p, arr, 1, None, p, p, p, ws, None, None),
                 (p, arr, 1, p, None, p, p, ws, None, None), (p, arr, 1, p, p, None, p, ws, None, None),
                 (p, arr, 1, p, p, p, p, ws - 1, None, None)):
        assert f(*args) == -22, args


def test_cli_flags_and_png_only_when_asked(tmp_path, monkeypatch):
    """--save_png / --png_palette parse on both drivers' parser (default off, palette voc); wild.run_cli writes {id}.png beside
    {id}.npy only with the flag, with the palette asked for (the segmentation itself is stubbed: no device here)."""
    sys.path.insert(0, os.path.join(ROOT, "pnp-ovss_amd"))
    import PnP_OVSS_0514_updated_segmentation as cli
    import lavis.models
    import torch
    from pnp_ovss import wild
    a = cli.get_args_parser().parse_args([])
    assert a.save_png is False and a.png_palette == "voc"
    a = cli.get_args_parser().parse_args(["--save_png", "--png_palette", "grey"])
    assert a.save_png and a.png_palette == "grey"
    assert cli.get_args_parser().parse_args(["--png_palette", "overlay"]).png_palette == "overlay"
    with pytest.raises(SystemExit):
        cli.get_args_parser().parse_args(["--png_palette", "rainbow"])
    assert wild.WildResult("a", None, None, "N_drop").png is None

    (tmp_path / "In_the_wild").mkdir()
    (tmp_path / "In_the_wild" / "a.jpg").write_bytes(b"")
    (tmp_path / "names.json").write_text('{"a": ["dog"]}')
    lab = np.array([[0, 1], [1, 1]], dtype=np.uint8)
    seen = []

    def fake_segment(model, args, images, class_names, ids=None, overlays=True, png=False, png_palette="voc"):
        seen.append((png, png_palette))
        return [wild.WildResult(ids[0], lab, b"jpeg bytes", "N_drop", R.encode(lab, R.voc_palette_ref())[2] if png else None)]

    monkeypatch.setattr(wild, "segment_in_the_wild", fake_segment)
    monkeypatch.setattr(lavis.models, "load_model_and_preprocess", lambda *a, **k: (None, None, None))
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    for flags, want in (([], ["BLIP_N_drop_a_blur.jpeg", "a.npy"]), (["--save_png"], ["BLIP_N_drop_a_blur.jpeg", "a.npy", "a.png"]),
                        (["--png_palette", "grey"], ["BLIP_N_drop_a_blur.jpeg", "a.npy"])):
        save = tmp_path / ("out" + "_".join(flags))
        args = cli.get_args_parser().parse_args(["--in_the_wild", "--wild_classes", str(tmp_path / "names.json"), "--home_dir", str(tmp_path),
                                                 "--save_path", str(save), "--prune_att_head", "9", "--postprocess", "blur"] + flags)
        wild.run_cli(0, 1, args)
        assert sorted(os.listdir(save)) == ["0519_Segmentation"]
        assert sorted(os.listdir(save / "0519_Segmentation")) == want, flags
        assert seen[-1] == (bool(args.save_png), args.png_palette)
        if args.save_png:
            from PIL import Image
            assert np.array_equal(np.asarray(Image.open(save / "0519_Segmentation" / "a.png")), np.load(save / "0519_Segmentation" / "a.npy"))
