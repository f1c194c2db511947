"""GPU: the scan-by-scan JPEG decoder (csrc/jpeg_prog.hip, `pnp_jpeg_decode_scans`) on progressive files, stage by stage: `coef`
against the coefficients the file was written from, then `rgb` against Pillow's `Image.open(...).convert('RGB')` of the same
bytes, both by exact equality and with err == 0.  The files come from _jpeg_progressive.py (a writer for arbitrary scan scripts,
checked against Pillow in test_jpeg_progressive_cpu.py) and from Pillow's own progressive encoder, whose baseline file of the
same image holds the coefficient reference.  Buffers are poisoned and sit between guard blocks, as in test_jpeg_ops_gpu.py."""
import numpy as np
import pytest
import torch

import _jpeg_progressive as P
import _jpeg_streams as S
from pnp_ovss import hip, jpeg as PJ
from test_jpeg_ops_gpu import POISON, _Bytes

pytestmark = pytest.mark.gpu


def run_scans(files):
    """pnp_jpeg_decode_scans on pack_scans(files) with poisoned, guarded buffers of its own -> dict of coef, rgb, rounds, err and
    the descriptors."""
    lib = hip.load_library()
    data, imgs, tabs, scans, segs, groups, sizes, tot = PJ.pack_scans(files)

    def up(buf):
        return torch.frombuffer(bytearray(bytes(buf)), dtype=torch.uint8).cuda()
    d_data, d_imgs, d_tabs, d_scans, d_segs = torch.from_numpy(data).cuda(), up(imgs), up(tabs), up(scans), up(segs)
    bufs = dict(clean=_Bytes(tot["clean_bytes"], POISON), seg_bits=_Bytes(4 * len(segs), POISON), coef=_Bytes(2 * tot["coef_elems"], POISON),
                hist=_Bytes(tot["coef_elems"] // 8, POISON), planes=_Bytes(tot["plane_bytes"], POISON), rgb=_Bytes(tot["rgb_bytes"], POISON),
                rounds=_Bytes(4 * len(segs), POISON))
    d_err = torch.zeros(1, dtype=torch.int32, device="cuda")
    groups = np.ascontiguousarray(groups, dtype=np.int32)
    r = lib.pnp_jpeg_decode_scans(d_data.data_ptr(), d_imgs.data_ptr(), d_tabs.data_ptr(), d_scans.data_ptr(), d_segs.data_ptr(),
                                  len(files), len(scans), len(segs), tot["base_segments"], groups.ctypes.data, len(groups),
                                  bufs["clean"].live.data_ptr(), bufs["seg_bits"].live.data_ptr(), bufs["coef"].live.data_ptr(),
                                  tot["coef_elems"], bufs["hist"].live.data_ptr(), bufs["planes"].live.data_ptr(),
                                  bufs["rgb"].live.data_ptr(), tot["max_blocks"], tot["max_pixels"], bufs["rounds"].live.data_ptr(),
                                  None, d_err.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert r == 0, f"pnp_jpeg_decode_scans returned {r}"
    out = {k: b.check(k) for k, b in bufs.items()}
    out["coef"], out["rounds"], out["seg_bits"] = out["coef"].view(np.int16), out["rounds"].view(np.int32), out["seg_bits"].view(np.int32)
    out.update(err=int(d_err.item()), imgs=imgs, scans=scans, segs=segs, sizes=sizes, tot=tot, groups=groups)
    return out


_REF = {}


def reference(src):
    """-> (frame, quantised coefficients per component, per component the blocks one-component scans cover), once per source."""
    if src not in _REF:
        j, q = S.quantised(src)
        _REF[src] = (j["frame"], q, P.covered(j["frame"]))
    return _REF[src]


def check_stages(files, sources, names, out=None):
    """coef, then rgb, of every image of the batch; the first differing stage is the one reported.  Coefficients: all 64 on the
    blocks one-component scans cover, zero AC on the others, the DC of the whole padded grid where a DC scan is interleaved."""
    out = run_scans(files) if out is None else out
    assert out["err"] == 0, f"coef: the decoder reported corrupt data in a batch of valid files ({names[0]} ...)"
    imgs = out["imgs"]
    for i, (f, src) in enumerate(zip(files, sources)):
        frame, q, cov = reference(src)
        im = imgs[i]
        prog = PJ.is_progressive(f)
        whole_dc = not prog or im.ncomp == 1 or any(sc.image == i and sc.kind == 1 and sc.ncomp > 1 for sc in out["scans"])
        for c in range(im.ncomp):
            nb = im.bx[c] * im.by[c]
            got = out["coef"][im.coef_off[c]:im.coef_off[c] + nb * 64].reshape(im.by[c], im.bx[c], 64)
            want = q[c].copy()
            if prog:
                want[~cov[c], 1:] = 0
                if not whole_dc:
                    want[~cov[c], 0] = 0
            bad = np.argwhere(got != want)
            assert not len(bad), (f"coef: {names[i]} component {c}: {len(bad)} differ, first (by, bx, k) = {bad[0]}: "
                                  f"{got[tuple(bad[0])]} != {want[tuple(bad[0])]}")
        H, W = out["sizes"][i]
        got = out["rgb"][im.rgb_off:im.rgb_off + H * W * 3].reshape(H, W, 3)
        rgb = S.pillow_rgb(f)
        bad = np.argwhere(got != rgb)
        assert not len(bad), f"rgb: {names[i]}: {len(bad)} differ, first (y, x, ch) = {bad[0]}: {got[tuple(bad[0])]} != {rgb[tuple(bad[0])]}"
    return out


def _cases(cases):
    return [d for _, _, d in cases], [s for _, s, _ in cases], [n for n, _, _ in cases]


# ------------------------------------------------------------------------------------------ 1. scan scripts x small shapes
def test_scripts_on_small_shapes():
    """Pillow's colour and grey scripts, spectral selection only, one band per coefficient, successive approximation from Al = 3,
    chroma before luma, DC scans per component, table ids 2 and 3, one DHT segment for all tables -- on 1 x 1, 8 x 8 and 17 x 17
    grey, 24 x 40 and 40 x 24 at 4:2:0 and 4:2:2 (5 of 6 luma block columns and 3 of 4 rows are real: one-component scans
    cover fewer blocks than the plane holds), a width of 4 at 4:2:0 (chroma replication) and 13 x 21 at 4:4:4: one batch, and
    a sample alone."""
    files, sources, names = _cases(P.script_cases())
    check_stages(files, sources, names)
    for k in (0, 8, 21, 40, len(files) - 4, len(files) - 2):
        check_stages([files[k]], [sources[k]], [names[k]])


def test_restart_intervals():
    """DRI 1, 2 and 7: MCUs in the interleaved DC scans, blocks in the one-component scans; Pillow's restart_marker_blocks=2."""
    files, sources, names = _cases(P.restart_cases())
    out = check_stages(files, sources, names)
    assert sum(1 for g in out["segs"] if g.image == 0) == 6 * 6 + 4 * 15        # 6 scans of 2 x 3 MCUs or chroma blocks, 4 luma scans of 3 x 5 blocks
    check_stages(files[-1:], sources[-1:], names[-1:])
    check_stages(files[2:3], sources[2:3], names[2:3])


# ------------------------------------------------------------------------------------------ 2. long segments, dense history
def test_dense_history_many_subsequences():
    """64 x 64 at quality 95 with sigma 25 noise: the luma AC segments span many sub-sequences, the refinement scans have history
    at most positions, and correction bits cross the cuts between sub-sequences."""
    src, a, b = P.dense_case()
    out = check_stages([a, b], [src, src], ["dense pillow script", "dense approximation script"])
    nsub = [-(-int(bits) // g.sub_bits) for g, bits in zip(out["segs"], out["seg_bits"])]
    refine = [k for k, g in enumerate(out["segs"]) if out["scans"][g.scan].kind == 4]
    assert max(nsub[k] for k in refine) >= 32
    assert all(1 <= out["rounds"][k] <= nsub[k] + 1 for k in refine), "the fixed point takes at most one round per sub-sequence"
    print("[measured] AC refinement: sub-sequences", [nsub[k] for k in refine], "rounds", [int(out["rounds"][k]) for k in refine])


def test_run_that_outlasts_the_bits_of_its_segment():
    """A refinement scan that ends on a byte boundary inside an end-of-band run over blocks without history: the last blocks of
    the segment come behind its last bit, and the stream has not ended early."""
    src, data = P.aligned_run_case()
    assert P.PAD_BITS[data][-1] == 0
    check_stages([data], [src], ["aligned end-of-band run"])


def test_end_of_band_run_longer_than_32767_blocks():
    """A flat 1456 x 1456 grey image: 33 124 blocks without AC, so the end-of-band run of the first AC scan and of the refinement
    scan is split at its maximum of 32 767."""
    src = S.pillow_jpeg(np.full((1456, 1456), 200, dtype=np.uint8), quality=75)
    data = P.recode_progressive(src, [((0,), 0, 0, 0, 0), ((0,), 1, 63, 0, 1), ((0,), 1, 63, 1, 0)])
    out = check_stages([data], [src], ["flat 1456 x 1456"])
    assert out["imgs"][0].bx[0] * out["imgs"][0].by[0] == 33124 > 32767
    assert all(s.raw_len < 16 for s in out["segs"][1:])           # two end-of-band runs each: 32 767 blocks, then 357


def test_pillow_default_375x500():
    img = S.noisy_image(375, 500, 12, sigma=6.0)
    base, prog = P.pillow_pair(img, quality=75)
    check_stages([prog], [base], ["Pillow progressive 375 x 500"])


# ------------------------------------------------------------------------------------------ 3. batches
def _mixed():
    cases = P.script_cases()
    rst = P.restart_cases()
    base = S.table_case("unary", "luma1", "422")
    brst = S.restart_cases()["dri7"]
    gray = S.table_case("skewed", "shared0", "gray")
    files = [cases[3][2], base[1], cases[0][2], brst[1], rst[0][2], gray[1], rst[-1][2]]
    sources = [cases[3][1], base[0], cases[0][1], brst[0], rst[0][1], gray[0], rst[-1][1]]
    return files, sources, ["progressive 4:2:0", "baseline 4:2:2", "progressive grey 1 x 1", "baseline dri7", "progressive dri1",
                            "baseline grey", "pillow progressive restart"]


def test_mixed_batch_equals_single_file_decodes():
    """Baseline, progressive, grey and restart files in one batch: every stage right, and jpeg_decode_batch returns views of ONE
    buffer, in batch order, equal to the single-file decodes bit for bit."""
    files, sources, names = _mixed()
    check_stages(files, sources, names)
    got = hip.jpeg_decode_batch(files)
    base = got[0].untyped_storage().data_ptr()
    off = 0
    for f, g, name in zip(files, got, names):
        assert g.untyped_storage().data_ptr() == base and g.data_ptr() == base + off, name
        off += g.numel()
        alone = hip.jpeg_decode_batch([f])[0]
        assert torch.equal(alone, g), name
        assert np.array_equal(g.cpu().numpy(), S.pillow_rgb(f)), name
    again = hip.jpeg_decode_batch(files)
    assert all(torch.equal(a, b) for a, b in zip(got, again)), "two calls, different bytes"
    only_base = [f for f in files if not PJ.is_progressive(f)]
    for g, f in zip(hip.jpeg_decode_batch(only_base), only_base):
        assert np.array_equal(g.cpu().numpy(), S.pillow_rgb(f))


def _refine_symbol_size_2():
    """The dense stream with the AC table of its first refinement scan relabelled so that symbol 0x01 reads 0x02: the first new
    coefficient of that scan arrives with size 2."""
    _, data, _ = P.dense_case()
    j = PJ.parse_progressive(data)
    k = [i for i, s in enumerate(j["scans"]) if s["kind"] == 4][0]
    start = j["scans"][k]["start"]
    dht = data.rfind(b"\xff\xc4", 0, start)
    sym = dht + 5 + 16
    at = data.index(b"\x01", sym, start)
    return data[:at] + b"\x02" + data[at + 1:]


@pytest.mark.parametrize("kind", ("refinement_size_2", "scan_cut"))
def test_corrupt_streams_are_reported(kind):
    """A refinement symbol of size 2 and a scan cut in the middle: err is set, the guard blocks are intact, jpeg_decode_batch
    raises RuntimeError, and the next valid batch decodes correctly."""
    src, good, _ = P.dense_case()
    if kind == "refinement_size_2":
        data = _refine_symbol_size_2()
    else:
        j = PJ.parse_progressive(good)
        s = j["scans"][5]
        mid = (s["start"] + s["end"]) // 2
        while good[mid - 1] == 0xFF or good[mid] == 0xFF:
            mid += 1
        data = good[:mid] + good[s["end"]:]
    PJ.parse_progressive(data)                                       # the strict parser accepts the file: only its entropy data is bad
    assert run_scans([data])["err"] == 1
    with pytest.raises(RuntimeError):
        hip.jpeg_decode_batch([data, good])
    got = hip.jpeg_decode_batch([good])[0].cpu().numpy()
    assert np.array_equal(got, S.pillow_rgb(good))


def test_argument_checks_come_first():
    lib = hip.load_library()
    g = np.array([[0, 1, 1, 0]], dtype=np.int32)
    assert lib.pnp_jpeg_decode_scans(None, None, None, None, None, 1, 1, 1, 0, g.ctypes.data, 1, None, None, None, 64, None, None, None,
                                     1, 1, None, None, None, None) != 0
    one = 1 << 12                                                    # non-null pointers that are never touched: the group list is wrong
    assert lib.pnp_jpeg_decode_scans(one, one, one, one, one, 1, 1, 2, 0, g.ctypes.data, 1, one, one, one, 64, one, one, one, 1, 1, None,
                                     None, one, None) != 0


# ------------------------------------------------------------------------------------------ 4. end to end
def test_segment_in_the_wild_progressive_equals_baseline(golden_dir):
    """segment_in_the_wild on Pillow's progressive file of an image gives the label map it gives on the baseline file."""
    import argparse
    import json
    import os
    import warnings
    from pnp_ovss import config as C, wild
    from pnp_ovss.model import build_model
    g = np.load(os.path.join(golden_dir, "checkpoint_small.npz"))
    cfg = C.ModelCfg(**json.loads(str(g["cfg"])))
    yy, xx = np.mgrid[0:40, 0:56].astype(np.float32)
    img = np.clip(np.stack([128 + 90 * np.sin(0.11 * (c + 1) * xx + 0.07 * (3 - c) * yy + c) for c in range(3)], -1), 0, 255).astype(np.uint8)
    base, prog = P.pillow_pair(img, quality=90)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = build_model(cfg=cfg, max_batch=2, max_text_len=32, stash_layer=7, bf16=False, seed=int(g["init_seed"]))
    args = argparse.Namespace(img_size=64, drop_iter=1, max_att_block_num=8, prune_att_head="9", threshold=0.15, postprocess="blur+crf",
                              batch_size=2, device_progressive=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                               # a fall-back to Pillow would warn
        res = wild.segment_in_the_wild(model, args, [base, prog], [["boat", "water"]] * 2, ["base", "prog"], overlays=False)
        dec = wild.decode_images([prog], ["prog"], True)[0]
    model.engine.close()
    assert isinstance(dec, torch.Tensor) and np.array_equal(dec.cpu().numpy(), S.pillow_rgb(prog))
    assert res[0].labels.shape == (40, 56) and np.array_equal(res[0].labels, res[1].labels)
