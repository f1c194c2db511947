"""GPU: the device JPEG decoder (csrc/jpeg.hip, `pnp_jpeg_decode`) stage by stage -- byte un-stuffing, Huffman entropy decode,
inverse DCT, upsampling + colour -- each against its own bit-exact reference, on the streams of _jpeg_streams.py that Pillow's
encoder never writes.  A failure names the stage: `unstuff`, `coef`, `planes` or `rgb`.

References: unstuff = the segment's bytes with every FF 00 replaced by FF; coef = the quantised coefficients the stream was
written from (or the oracle's entropy decode divided by the quantisation table); planes = oracle/jpeg_np.py's islow IDCT of
them; rgb = Pillow's `Image.open(...).convert('RGB')` of the same bytes.  Every comparison is exact equality."""
import time

import numpy as np
import pytest
import torch

import _jpeg_streams as S
from oracle import jpeg_np as J
from pnp_ovss import hip, jpeg as PJ

pytestmark = pytest.mark.gpu

POISON, SENTINEL, GUARD = 0xA5, 0x3C, 4096


class _Bytes:
    """`n` device bytes filled with `fill` between two guard blocks of SENTINEL bytes (the manner of _gpu_guard.Guarded)."""

    def __init__(self, n, fill):
        self.n = int(n)
        self.buf = torch.full((2 * GUARD + self.n,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.live = self.buf[GUARD:GUARD + self.n]
        self.live.fill_(fill)
        assert self.live.data_ptr() % 16 == 0

    def check(self, tag):
        raw = self.buf.cpu().numpy()
        assert (raw[:GUARD] == SENTINEL).all(), f"{tag}: front guard written"
        assert (raw[GUARD + self.n:] == SENTINEL).all(), f"{tag}: back guard written"
        return raw[GUARD:GUARD + self.n].copy()


def run_stages(files):
    """pnp_jpeg_decode on pack_batch(files) with buffers of its own, as hip.jpeg_decode_batch allocates them -> dict of every
    intermediate on the host (clean, seg_bits, coef, planes, rgb, err, seconds) plus the descriptors.  clean / planes / rgb
    start as POISON bytes, so nothing can lean on stale memory; all five buffers sit between guard blocks."""
    lib = hip.load_library()
    data, imgs, tabs, segs, sizes, tot = PJ.pack_batch(files)

    def up(buf):
        return torch.frombuffer(bytearray(bytes(buf)), dtype=torch.uint8).cuda()
    d_data, d_imgs, d_tabs, d_segs = torch.from_numpy(data).cuda(), up(imgs), up(tabs), up(segs)
    bufs = dict(clean=_Bytes(tot["clean_bytes"], POISON), seg_bits=_Bytes(4 * len(segs), POISON), coef=_Bytes(2 * tot["coef_elems"], POISON),
                planes=_Bytes(tot["plane_bytes"], POISON), rgb=_Bytes(tot["rgb_bytes"], POISON))
    d_err = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = lib.pnp_jpeg_decode(d_data.data_ptr(), d_imgs.data_ptr(), d_tabs.data_ptr(), d_segs.data_ptr(), len(files), len(segs),
                            bufs["clean"].live.data_ptr(), bufs["seg_bits"].live.data_ptr(), bufs["coef"].live.data_ptr(),
                            tot["coef_elems"], bufs["planes"].live.data_ptr(), bufs["rgb"].live.data_ptr(), tot["max_blocks"],
                            tot["max_pixels"], d_err.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    assert r == 0, f"pnp_jpeg_decode returned {r}"
    out = {k: b.check(k) for k, b in bufs.items()}
    out["seg_bits"] = out["seg_bits"].view(np.int32)
    out["coef"] = out["coef"].view(np.int16)
    out.update(err=int(d_err.item()), seconds=seconds, imgs=imgs, segs=segs, sizes=sizes, tot=tot, data=data)
    return out


_REF = {}


def reference(data):
    """-> (quantised coefficients per component, planes per component, Pillow's pixels), computed once per stream."""
    if data not in _REF:
        j, q = S.quantised(data)
        planes = [J._plane(qc * j["qt"][c["tq"]]) for c, qc in zip(j["frame"]["comps"], q)]
        _REF[data] = (q, planes, S.pillow_rgb(data))
    return _REF[data]


def check_stages(files, names, out=None):
    """Every stage of every image of the batch against its reference; the first differing stage is the one reported."""
    out = run_stages(files) if out is None else out
    imgs, segs, data = out["imgs"], out["segs"], out["data"]
    end = 0
    for k, s in enumerate(segs):                                   # ---- unstuff
        im = imgs[s.image]
        raw = bytes(data[im.data_off + s.byte_off:im.data_off + s.byte_off + s.raw_len])
        want = S.unstuff(raw)
        tag = f"unstuff: {names[s.image]} segment {k}"
        assert out["seg_bits"][k] == 8 * len(want), f"{tag}: {out['seg_bits'][k]} bits, expected {8 * len(want)}"
        got = out["clean"][s.clean_off:s.clean_off + s.clean_cap]
        assert bytes(got[:len(want)]) == want, f"{tag}: bytes differ, first at {_first_diff(got[:len(want)], want)} of {len(want)}"
        assert not got[len(want):].any(), f"{tag}: bytes behind the data up to clean_cap are not zero"
        assert s.clean_off == end
        end = s.clean_off + s.clean_cap
    assert end == out["tot"]["clean_bytes"]
    assert out["err"] == 0, f"coef: the entropy decoder reported corrupt data in a batch of valid streams ({names[0]} ...)"
    coef_end = 0
    for i, f in enumerate(files):
        q, planes, rgb = reference(f)
        im = imgs[i]
        assert im.ncomp == len(q)
        for c in range(im.ncomp):                                  # ---- coefficients, natural order, block (by, bx) of the plane
            nb = im.bx[c] * im.by[c]
            assert q[c].shape == (im.by[c], im.bx[c], 64) and im.coef_off[c] == coef_end
            got = out["coef"][im.coef_off[c]:im.coef_off[c] + nb * 64].reshape(im.by[c], im.bx[c], 64)
            bad = np.argwhere(got != q[c])
            assert not len(bad), f"coef: {names[i]} component {c}: {len(bad)} differ, first (by, bx, k) = {bad[0]}: {got[tuple(bad[0])]} != {q[c][tuple(bad[0])]}"
            coef_end += nb * 64
        for c in range(im.ncomp):                                  # ---- planes
            nb = im.bx[c] * im.by[c]
            got = out["planes"][im.plane_off[c]:im.plane_off[c] + nb * 64].reshape(im.by[c] * 8, im.bx[c] * 8)
            bad = np.argwhere(got != planes[c])
            assert not len(bad), f"planes: {names[i]} component {c}: {len(bad)} differ, first (y, x) = {bad[0]}"
        H, W = out["sizes"][i]                                     # ---- pixels
        got = out["rgb"][im.rgb_off:im.rgb_off + H * W * 3].reshape(H, W, 3)
        bad = np.argwhere(got != rgb)
        assert not len(bad), f"rgb: {names[i]}: {len(bad)} differ, first (y, x, ch) = {bad[0]}: {got[tuple(bad[0])]} != {rgb[tuple(bad[0])]}"
    assert coef_end == out["tot"]["coef_elems"]
    return out


def _first_diff(a, b):
    n = min(len(a), len(b))
    return next((i for i in range(n) if a[i] != b[i]), n)


# ------------------------------------------------------------------------------------------ 1. table shapes
def test_table_shapes_one_batch_and_alone():
    """Unary / skewed / flat tables x (chroma shares table 0, luma on table 1, one DHT segment) x 4:4:4, 4:2:2, 4:2:0 and
    grayscale in ONE batch (coef_off, plane_off, clean_off, the table index and the sharing of tables by content), and a
    sample of them alone."""
    files = [S.table_case(*c)[1] for c in S.TABLE_CASES]
    names = [" ".join(c) for c in S.TABLE_CASES]
    out = check_stages(files, names)
    assert len({im.tab for im in out["imgs"]}) > 12                # (4 samplings x 3 sets x >= 2 distinct table contents)
    for k in (0, 5, 10, 15, 22, 27, 31, 32):
        check_stages([files[k]], [names[k]])


# ------------------------------------------------------------------------------------------ 2. all sub-sequences live
@pytest.mark.parametrize("name", ("skewed_19k", "skewed_4k", "all_live"))
def test_long_streams(name):
    """Streams whose input conditions test_jpeg_streams_cpu.py::test_long_stream_input_conditions asserts: more than 128 bits
    per sub-sequence, every one of the 1024 threads live, stuffed FF bytes at the last byte of a 16-byte slice and of a
    4096-byte chunk of the un-stuffing kernel, the long-code path in nearly every symbol."""
    _, data = S.long_streams()[name]
    p = S.stream_properties(data)
    out = check_stages([data], [name])
    s = out["segs"][0]
    assert (s.raw_len, s.sub_bits, int(out["seg_bits"][0])) == (p["raw_len"], p["sub_bits"], 8 * p["clean_len"])
    if name == "all_live":
        assert -(-int(out["seg_bits"][0]) // s.sub_bits) == PJ.SUBSEQUENCES and s.sub_bits > 128
    else:
        assert p["stuffed_mod16_15"] >= 2 and p["stuffed_mod4096_4095"] >= 1


# ------------------------------------------------------------------------------------------ 3. no self-synchronisation
def test_flat_tables_do_not_self_synchronise():
    """Fixed-length codes never re-align a sub-sequence that started at the wrong bit: the result is right only if the round
    loop carries thread 0's state down the whole chain.  Exact coefficients and pixels, in bounded time."""
    src, data = S.flat_stream()
    p = S.stream_properties(data)
    assert p["segments"] == 1 and p["live"] >= 64
    out = check_stages([data], ["flat 4:4:4"])
    assert out["seconds"] < 5.0, f"{out['seconds']:.2f} s for one {p['raw_len']}-byte segment"
    out = check_stages([data, S.long_streams()["all_live"][1]], ["flat 4:4:4", "all_live"])
    assert out["seconds"] < 5.0


# ------------------------------------------------------------------------------------------ 4. restart segments
def test_restart_segments():
    """DRI 1 (one MCU and fewer than 16 bytes per segment, RSTn wrapping), DRI 7 on 25 MCUs, one MCU row per segment, DRI >= the
    MCU count, and files without DRI in the same batch."""
    cases = S.restart_cases()
    names = list(cases)
    out = check_stages([d for _, d in cases.values()], names)
    nseg = [sum(1 for s in out["segs"] if s.image == i) for i in range(len(names))]
    assert nseg == [25, 15, 4, 5, 3, 1, 1, 1]
    assert max(s.raw_len for s in out["segs"] if s.image == 0) < 16
    check_stages([cases["dri1"][1]], ["dri1"])
    check_stages([cases["dri7"][1], cases["dri0"][1]], ["dri7", "dri0"])


# ------------------------------------------------------------------------------------------ 5. geometry
def test_geometry():
    """1 x 1 to 17 x 17, single rows and columns, every sampling, grayscale written with 2 x 2 factors; includes the widths
    up to 4 where libjpeg replicates the chroma samples instead of its fancy upsampling."""
    cases = S.geometry_cases()
    assert len(cases) == len(S.GEOMETRY_SIZES) * 5
    check_stages([d for _, d in cases], [n for n, _ in cases])
    for k in (0, 2, 13, 31, 59):
        check_stages([cases[k][1]], [cases[k][0]])


@pytest.mark.parametrize("ss", (1, 2))
def test_narrow_images_replicate_chroma(ss):
    """jdsample.c: fancy upsampling only when the downsampled chroma width exceeds 2.  Widths 1..6 and 9, heights 1..17."""
    rng = np.random.default_rng(200 + ss)
    files, names = [], []
    for H in (1, 2, 3, 12, 17):
        for W in (1, 2, 3, 4, 5, 6, 9):
            files.append(S.pillow_jpeg(rng.integers(0, 256, (H, W, 3), dtype=np.uint8), quality=95, subsampling=ss))
            names.append(f"{H}x{W} subsampling {ss}")
    check_stages(files, names)


# ------------------------------------------------------------------------------------------ 6. stream dressing
def test_stream_dressing():
    """Fill bytes, COM / APPn, bytes and whole files behind EOI, no JFIF, Adobe transform 1, component ids 0,1,2, SOF1 with
    16-bit DQT, one DHT segment: Pillow's pixels for each, alone and in one batch."""
    cases = S.dressing_cases()
    check_stages([d for _, d in cases.values()], list(cases))
    for name, (_, d) in cases.items():
        check_stages([d], [name])
        got = hip.jpeg_decode_batch([d])[0].cpu().numpy()
        assert np.array_equal(got, S.pillow_rgb(d)), name


# ------------------------------------------------------------------------------------------ 7. error reporting
@pytest.mark.parametrize("kind", ("undefined_ac_code", "truncated"))
def test_corrupt_streams_are_reported(kind):
    """An undefined Huffman code and a scan cut in the middle: err is set, hip.jpeg_decode_batch raises RuntimeError, and the
    guard blocks around all five buffers are intact (run_stages checks them)."""
    if kind == "undefined_ac_code":
        data = S.undefined_ac_code_stream()
    else:
        data = S.long_streams()["skewed_4k"][1]
        data = data[:len(data) // 2] + b"\xff\xd9"
    out = run_stages([data])
    assert out["err"] == 1
    with pytest.raises(RuntimeError):
        hip.jpeg_decode_batch([data])
