"""GPU: label maps as 8-bit PNG files, deflate-encoded on the device (csrc/png_enc.hip through hip.png_encode_batch).  The
contract is the byte format: every file must equal the pure-Python reference's (_png_refs.py) byte for byte, and open in Pillow
to the labels that went in."""
import glob
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _png_refs as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _runs(lengths, values):
    return np.concatenate([np.full(n, v, dtype=np.uint8) for n, v in zip(lengths, values)])


def _cases(golden_dir):
    rng = np.random.default_rng(17)
    c = {}
    for H, W in ((1, 1), (1, 2), (2, 1), (3, 7)):
        c[f"random {H}x{W}"] = rng.integers(0, 256, (H, W), dtype=np.uint8)
    # constant rows: label 0 joins the filter byte's run (rem = W), another label starts a run of its own (rem = W - 1) -- between
    # them rem = 0, 1, 2, 3 and 258 k + 0, 1, 2, 3 all occur
    for W in (2, 3, 4, 257, 258, 259, 260, 261, 516, 517, 518):
        c[f"constant 0 1x{W}"] = np.zeros((1, W), dtype=np.uint8)
        c[f"constant 5 2x{W}"] = np.full((2, W), 5, dtype=np.uint8)
    c["constant 1x1 label 0"] = np.zeros((1, 1), dtype=np.uint8)
    lens = (1, 2, 3, 4, 259, 260, 261, 262, 775)
    c["runs side by side"] = np.stack([_runs(lens, (1, 2, 1, 3, 9, 4, 200, 6, 7)), _runs(lens[::-1], (1, 2, 1, 3, 9, 4, 200, 6, 7))])
    # 9-bit literals (144, 255), the last 8-bit one (143); matches of length 114 (7-bit length code 279) and 115 (8-bit, 280):
    # runs of 115 and 116; row 1 = row 0 - 1 everywhere, so its Up difference is the constant 255 (a negative difference) and Up wins
    top = _runs((115, 116, 115, 116, 40), (255, 144, 143, 255, 144))
    c["high labels, Up of -1"] = np.stack([top, top - 1, _runs((116, 115, 116, 115, 40), (143, 144, 255, 143, 254))])
    base = _runs((10, 15, 15), (0, 3, 7))
    c["two rows c2 < c0"] = np.stack([base, _runs((10, 15, 15), (1, 4, 8))])                 # Up: constant 1
    c["two rows c2 = c0"] = np.stack([base, _runs((10, 15, 15), (0, 5, 7))])                 # raw 2 changes; Up 0 2 0: 2 changes
    c["two rows c2 > c0"] = np.stack([base, _runs((20, 20), (2, 9))])                        # raw 1 change; Up 3 changes
    c["random 33x65"] = rng.integers(0, 256, (33, 65), dtype=np.uint8)
    c["constant 64x600"] = np.full((64, 600), 12, dtype=np.uint8)
    c["blob 375x500"] = R.blob_map(375, 500, 5, 3)
    for k, (H, W) in enumerate(((9, 33), (40, 1), (1, 77), (17, 129), (5, 5), (64, 63), (2, 301))):      # the mixed batch
        c[f"mixed {H}x{W}"] = R.blob_map(H, W, 4, 20 + k) if k % 2 == 0 else rng.integers(0, 3, (H, W), dtype=np.uint8)
    g = np.load(os.path.join(golden_dir, "pipeline_voc.npz"))
    for k in sorted(k for k in g.files if k.startswith("labels_")):
        c[f"pipeline_voc {k}"] = np.ascontiguousarray(g[k])
    return c


@pytest.fixture(scope="module")
def cases(golden_dir):
    """name -> (labels, the reference's zlib stream); computed once."""
    return {name: (lab, R.zlib_stream(lab)[0]) for name, lab in _cases(golden_dir).items()}


def _first_diff(a, b):
    n = min(len(a), len(b))
    return next((i for i in range(n) if a[i] != b[i]), n)


def test_filter_choice_of_the_built_rows(cases):
    """The hand-built cases do what their names say (a property of the reference, checked here so the names can be trusted)."""
    for name, want in (("two rows c2 < c0", [0, 2]), ("two rows c2 = c0", [0, 0]), ("two rows c2 > c0", [0, 0]),
                       ("high labels, Up of -1", [0, 2])):
        filt, filters = R.filtered_stream(cases[name][0])
        assert filters[:2] == want, name
    filt, _ = R.filtered_stream(cases["high labels, Up of -1"][0])
    assert set(filt[503:1005]) == {2, 255}
    toks = R.zlib_stream(cases["high labels, Up of -1"][0])[2]
    assert ("match", 114) in toks and ("match", 115) in toks
    assert {t for t in R.zlib_stream(cases["runs side by side"][0])[2] if t[0] == "match"} >= {("match", 3), ("match", 258)}
    lab, stream = cases["random 33x65"]
    # uniform bytes cost 8 + 112 / 256 = 8.44 bits each against the bound's 9: the stream expands and ends within 10 % of the bound
    assert len(stream) > lab.size and R.stream_capacity_ref(33, 65) - len(stream) < 0.10 * len(stream)


@pytest.mark.parametrize("palette", ["voc", "overlay", None])
def test_png_encode_batch_equals_reference_bytes(cases, palette):
    """Every case in ONE batch (sizes from 1 x 1 to 375 x 500, so every image sits at another alignment of the label buffer and
    of the packed words): files equal the reference's byte for byte, and Pillow reads the labels (and the palette) back."""
    from PIL import Image
    from pnp_ovss import hip, vis
    pal = {"voc": R.voc_palette_ref(), "overlay": vis.default_palette(), None: None}[palette]
    names = list(cases)
    got = hip.png_encode_batch([cases[n][0] for n in names], palette)
    bad = []
    for n, f in zip(names, got):
        lab, stream = cases[n]
        want = R.png_file(lab.shape[0], lab.shape[1], stream, pal)
        if f != want:
            bad.append((n, len(f), len(want), _first_diff(f, want)))
    assert not bad, f"(case, bytes, reference's bytes, first difference) {bad[:8]} ({len(bad)} of {len(got)} differ)"
    for n, f in zip(names, got):
        Image.open(io.BytesIO(f)).verify()
        im = Image.open(io.BytesIO(f))
        assert im.mode == ("L" if pal is None else "P") and np.array_equal(np.asarray(im), cases[n][0]), n
        if pal is not None:
            assert np.array_equal(np.asarray(im.getpalette(), dtype=np.uint8).reshape(-1, 3), pal), n


def test_batch_equals_single_runs_and_tensors_equal_numpy(cases):
    """The seven mixed images (W odd, W = 1, H = 1) in one batch against seven single calls, bit for bit; device tensors (also a
    non-contiguous view and an int64 map) against numpy inputs; a random palette."""
    from pnp_ovss import hip
    names = [n for n in cases if n.startswith("mixed ")]
    assert len(names) == 7
    maps = [cases[n][0] for n in names]
    pal = np.random.default_rng(4).integers(0, 256, (256, 3), dtype=np.uint8)
    batch = hip.png_encode_batch(maps, pal)
    for n, lab, f in zip(names, maps, batch):
        assert f == R.png_file(lab.shape[0], lab.shape[1], cases[n][1], pal), n
        assert hip.png_encode_batch([lab], pal) == [f], n
    dev = [torch.from_numpy(m).cuda() for m in maps]
    assert hip.png_encode_batch(dev, pal) == batch
    assert hip.png_encode_batch([dev[0], maps[1], dev[2]], pal) == batch[:3]           # a mixed list goes through the host
    wide = torch.from_numpy(np.ascontiguousarray(np.repeat(maps[3], 2, axis=1))).cuda()
    assert hip.png_encode_batch([wide[:, ::2], dev[5].to(torch.int64)], pal) == [batch[3], batch[5]]
    assert hip.png_encode_batch([], pal) == []


def test_png_capacity_guard(cases):
    """An image whose capacity is one byte short gets length -1 and err = 1 and not one byte (the sentinel is intact over its
    range and past the end); an image with exactly its length fits; the neighbours are the reference's streams."""
    from pnp_ovss import hip, png
    names = ["mixed 9x33", "random 33x65", "blob 375x500", "constant 5 2x517", "runs side by side"]
    maps = [cases[n][0] for n in names]
    want = [cases[n][1] for n in names]
    caps = [png.stream_capacity(*m.shape) for m in maps]
    caps[1] = len(want[1]) - 1                     # one byte short
    caps[3] = len(want[3])                         # exactly enough
    SENT = 0xA5
    out = torch.full((sum(caps) + 4096,), SENT, dtype=torch.uint8, device="cuda")
    out, offs, lens, err = hip.png_encode_streams(maps, caps, out=out)
    assert err == 1 and lens == [len(w) if k != 1 else -1 for k, w in enumerate(want)], (err, lens, [len(w) for w in want])
    host = out.cpu().numpy()
    assert (host[offs[1]:offs[1] + caps[1]] == SENT).all(), "bytes of the image that did not fit were written"
    assert (host[sum(caps):] == SENT).all(), "bytes past the declared capacities were written"
    for k in (0, 2, 3, 4):
        assert host[offs[k]:offs[k] + lens[k]].tobytes() == want[k], names[k]
        assert (host[offs[k] + lens[k]:offs[k] + caps[k]] == SENT).all(), names[k]
    out2, offs2, lens2, err2 = hip.png_encode_streams(maps)                            # unguarded: everything fits, same streams
    assert err2 == 0 and lens2 == [len(w) for w in want]
    host2 = out2.cpu().numpy()
    assert [host2[o:o + n].tobytes() for o, n in zip(offs2, lens2)] == want


# ------------------------------------------------------------------------------------------ in the wild, end to end
WILD_NAMES = {"harbour": ["boat", "water"], "street": ["car", "streetlamp", "person"]}
WILD_SIZES = {"harbour": (40, 56), "street": (50, 36)}


def _wild_photo(rng, H, W):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    img = np.stack([128 + 90 * np.sin(0.11 * (c + 1) * xx + 0.07 * (3 - c) * yy + c) for c in range(3)], -1)
    return np.clip(img + rng.normal(0, 6, (H, W, 3)), 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def wild_home(tmp_path_factory, golden_dir):
    """{home}/In_the_wild/harbour.jpeg + street.jpg, names.json, the synthetic checkpoint of checkpoint_small.npz as a .pth and
    the model geometry file the command line reads (PNP_OVSS_MODEL_CONFIG) -- the set-up of test_vis_gpu.py's in-the-wild test."""
    from PIL import Image
    from pnp_ovss import config as C, synth
    home = tmp_path_factory.mktemp("wild_png")
    (home / "In_the_wild").mkdir()
    rng = np.random.default_rng(2)
    paths = {}
    for (name, (H, W)), ext in zip(WILD_SIZES.items(), ("jpeg", "jpg")):
        paths[name] = str(home / "In_the_wild" / f"{name}.{ext}")
        Image.fromarray(_wild_photo(rng, H, W)).save(paths[name], "JPEG", quality=90)
    (home / "names.json").write_text(json.dumps(WILD_NAMES))
    g = np.load(os.path.join(golden_dir, "checkpoint_small.npz"))
    cfgd = json.loads(str(g["cfg"]))
    cfg = C.ModelCfg(**cfgd)
    ck = synth.synth_checkpoint(cfg, C.ModelCfg(**json.loads(str(g["cfg_ckpt"]))), int(g["ckpt_seed"]))
    torch.save({"model": {k: torch.from_numpy(v.copy()) for k, v in ck.items()}}, str(home / "ckpt.pth"))
    (home / "model.json").write_text(json.dumps(dict(cfgd, weight_seed=int(g["init_seed"]))))
    return dict(home=home, paths=paths, cfg=cfg, seed=int(g["init_seed"]))


def test_segment_in_the_wild_png_and_cli(wild_home, tmp_path):
    """segment_in_the_wild(png=True): r.png is the reference's file of r.labels (VOC palette; grey on request) and the run
    without png leaves it None; the command line with --save_png writes {id}.png beside {id}.npy, Pillow opens it to the same
    label map, and the other files are those of a run without the flag."""
    import argparse
    import warnings
    from PIL import Image
    from pnp_ovss import wild
    from pnp_ovss.model import build_model
    ids = sorted(WILD_NAMES)
    names = [WILD_NAMES[i] for i in ids]
    files = [open(wild_home["paths"][i], "rb").read() for i in ids]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = build_model(cfg=wild_home["cfg"], max_batch=2, max_text_len=32, stash_layer=7, bf16=False,
                            checkpoint=str(wild_home["home"] / "ckpt.pth"), seed=wild_home["seed"])
    args = argparse.Namespace(img_size=64, drop_iter=4, max_att_block_num=8, prune_att_head="9", threshold=0.15,
                              postprocess="blur+crf", batch_size=2)
    res = wild.segment_in_the_wild(model, args, files, names, ids, png=True)
    plain = wild.segment_in_the_wild(model, args, files, names, ids, overlays=False)
    grey = wild.segment_in_the_wild(model, args, files, names, ids, overlays=False, png=True, png_palette="grey")
    model.engine.close()
    for r, p, g_, i in zip(res, plain, grey, ids):
        assert r.id == i and r.labels.shape == WILD_SIZES[i] and p.png is None and np.array_equal(p.labels, r.labels)
        assert r.jpeg is not None and r.png == R.encode(r.labels, R.voc_palette_ref())[2], i
        assert g_.png == R.encode(r.labels, None)[2], i
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(r.png))), r.labels)
    save = tmp_path / "out"
    env = dict(os.environ, PNP_OVSS_MODEL_CONFIG=str(wild_home["home"] / "model.json"))
    for k in ("PNP_OVSS_DTYPE", "PNP_OVSS_CHECKPOINT", "PNP_OVSS_VOCAB", "PNP_OVSS_STASH_LAYER"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "pnp-ovss_amd", "PnP_OVSS_0514_updated_segmentation.py"), "--in_the_wild", "--save_png",
           "--wild_classes", str(wild_home["home"] / "names.json"), "--home_dir", str(wild_home["home"]), "--save_path", str(save),
           "--world_size", "1", "--img_size", "64", "--del_patch_num", "sort_thresh005", "--batch_size", "2",
           "--max_att_block_num", "8", "--drop_iter", "4", "--prune_att_head", "9", "--threshold", "0.15",
           "--postprocess", "blur+crf", "--checkpoint", str(wild_home["home"] / "ckpt.pth")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    written = sorted(os.path.basename(f) for f in glob.glob(str(save / "0519_Segmentation" / "*")))
    assert written == sorted([f"BLIP_N_drop_{i}_blur+crf.jpeg" for i in ids] + [f"{i}.npy" for i in ids] + [f"{i}.png" for i in ids])
    for r in res:
        d = save / "0519_Segmentation"
        lab = np.load(d / f"{r.id}.npy")
        assert np.array_equal(lab, r.labels)
        assert open(d / f"{r.id}.png", "rb").read() == r.png
        im = Image.open(d / f"{r.id}.png")
        assert im.mode == "P" and np.array_equal(np.asarray(im), lab)
