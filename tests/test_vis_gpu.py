"""GPU: the output side -- label-map overlays rendered (csrc/vis.hip) and baseline-JPEG encoded (csrc/jpeg_enc.hip) on the
device, and the in-the-wild entry point built on them.  The JPEG contract is Pillow's own bytes; the overlay contract is the
numpy restatement in _vis_refs.py, bit for bit."""
import glob
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _vis_refs as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUALITIES = (30, 75, 95)


@pytest.fixture(scope="module")
def images():
    """Every size of the issue x every content, in one list (the batch mixes all sizes)."""
    return [(f"{kind} {H}x{W}", R.test_image(kind, H, W)) for (H, W) in R.SIZES for kind in R.CONTENTS]


@pytest.fixture(scope="module")
def pillow_files(images):
    return {q: [R.pillow_jpeg(im, q) for _, im in images] for q in QUALITIES}


def _first_diff(a, b):
    n = min(len(a), len(b))
    return next((i for i in range(n) if a[i] != b[i]), n)


@pytest.mark.parametrize("quality", QUALITIES)
def test_jpeg_encode_batch_equals_pillow_bytes(images, pillow_files, quality):
    """One batch of 45 images (9 sizes x 5 contents: dummy luma blocks on both edges, H % 16 == 8, stuffed 0xFF bytes, ZRL runs,
    size-10 AC and size-11 DC categories, DC-only blocks) against Pillow's files; a sample of them encoded alone must give
    the same bytes (offset bookkeeping), and every stream must decode through the device decoder to Pillow's pixels."""
    from PIL import Image
    from pnp_ovss import hip
    got = hip.jpeg_encode_batch([im for _, im in images], quality=quality)
    want = pillow_files[quality]
    bad = [(name, len(g), len(w), _first_diff(g, w)) for (name, _), g, w in zip(images, got, want) if g != w]
    assert not bad, f"quality {quality}: (image, bytes, Pillow's bytes, first difference) {bad[:8]} ({len(bad)} of {len(got)} differ)"
    for k in (0, 7, 17, 26, 41, 44):                 # alone: same bytes as inside the batch
        (alone,) = hip.jpeg_encode_batch([torch.from_numpy(images[k][1]).cuda()], quality=quality)
        assert alone == got[k], images[k][0]
    dec = hip.jpeg_decode_batch(got)
    for (name, _), d, f in zip(images, dec, want):
        assert np.array_equal(d.cpu().numpy(), np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))), name


def test_jpeg_encode_capacity_guard(images, pillow_files):
    """An image that does not fit its declared capacity raises err, gets length -1 and not one byte (the sentinel of a larger
    buffer is intact over its whole range and beyond); its neighbours in the batch are still Pillow's bytes."""
    from pnp_ovss import hip, jpeg as J
    names = ["smooth 37x29", "noise 375x500", "checker 24x40", "noise 17x33"]
    idx = [[n for n, _ in images].index(n) for n in names]
    ims = [images[i][1] for i in idx]
    want = [pillow_files[75][i] for i in idx]
    hdr = [len(J.encode_headers(im.shape[0], im.shape[1], J.quality_tables(75))) for im in ims]
    need = [len(w) - h - 2 for w, h in zip(want, hdr)]                      # scan bytes: the file minus markers and EOI
    caps = [J.scan_capacity(im.shape[0], im.shape[1]) for im in ims]
    caps[1] = need[1] - 1                                                   # one byte short
    caps[3] = need[3]                                                       # exactly enough
    SENT = 0xA5
    out = torch.full((sum(caps) + 4096,), SENT, dtype=torch.uint8, device="cuda")
    out, offs, lens, err = hip.jpeg_encode_scans(ims, 75, caps, out=out)
    assert err == 1 and lens[1] == -1 and [lens[k] for k in (0, 2, 3)] == [need[k] for k in (0, 2, 3)], (err, lens, need)
    host = out.cpu().numpy()
    assert (host[offs[1]:offs[1] + caps[1]] == SENT).all(), "bytes of the image that did not fit were written"
    assert (host[sum(caps):] == SENT).all(), "bytes past the declared capacities were written"
    for k in (0, 2, 3):
        assert host[offs[k]:offs[k] + lens[k]].tobytes() == want[k][hdr[k]:-2], names[k]
        assert (host[offs[k] + lens[k]:offs[k] + caps[k]] == SENT).all(), names[k]
    # and through the public entry point the same batch comes out whole (the short default is retried with the bound)
    assert hip.jpeg_encode_batch(ims, 75) == want


def test_overlay_labels_bit_for_bit():
    """5 x 7, 33 x 45 and 64 x 64 in one batch (odd pixel counts put the later images off every alignment), labels over all of
    0..255, RGB with 0, 255 and the truncation witness, a random palette besides the default one."""
    from pnp_ovss import hip, vis
    rng = np.random.default_rng(11)
    sizes = [(5, 7), (33, 45), (64, 64)]
    labs, rgbs = [], []
    for i, (h, w) in enumerate(sizes):
        lab = rng.integers(0, 256, (h, w), dtype=np.uint8)
        lab.reshape(-1)[:: 3] = 0
        if h * w >= 512:
            lab.reshape(-1)[:512:2] = np.arange(256, dtype=np.uint8)        # every label value, on every other pixel
        rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        rgb[0, 0], rgb[0, 1], rgb[0, 2], rgb[1, 0] = 0, 255, R.TRUNCATION_WITNESS_RGB, R.TRUNCATION_WITNESS_RGB
        lab[0, 2], lab[1, 0] = 0, 3
        labs.append(lab)
        rgbs.append(rgb)
    assert set(np.concatenate([l.reshape(-1) for l in labs]).tolist()) == set(range(256))
    d_lab = torch.from_numpy(np.concatenate([l.reshape(-1) for l in labs])).cuda()
    d_rgb = torch.from_numpy(np.concatenate([r.reshape(-1) for r in rgbs])).cuda()
    off = np.concatenate([[0], np.cumsum([h * w for h, w in sizes])]).astype(np.int64)
    np.testing.assert_array_equal(vis.default_palette(), R.default_palette_ref())
    for pal, alpha in ((vis.default_palette(), 0.3), (rng.integers(0, 256, (256, 3), dtype=np.uint8), 0.55)):
        out = hip.overlay_labels(d_lab, d_rgb, off, pal, alpha).cpu().numpy()
        for i, (h, w) in enumerate(sizes):
            got = out[3 * off[i]:3 * off[i + 1]].reshape(h, w, 3)
            want = R.overlay_ref(labs[i], rgbs[i], pal, alpha)
            assert np.array_equal(got, want), (i, alpha, int((got != want).sum()))
    # the views a Segmenter batch hands over
    views = vis.render_overlays([d_lab[off[i]:off[i + 1]].view(h, w) for i, (h, w) in enumerate(sizes)], d_rgb, sizes)
    for v, lab, rgb in zip(views, labs, rgbs):
        assert np.array_equal(v.cpu().numpy(), R.overlay_ref(lab, rgb))


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
    the model geometry file the command line reads (PNP_OVSS_MODEL_CONFIG)."""
    from PIL import Image
    from pnp_ovss import config as C, synth
    home = tmp_path_factory.mktemp("wild")
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
    assert cfg.img_size == 64
    ck = synth.synth_checkpoint(cfg, C.ModelCfg(**json.loads(str(g["cfg_ckpt"]))), int(g["ckpt_seed"]))
    torch.save({"model": {k: torch.from_numpy(v.copy()) for k, v in ck.items()}}, str(home / "ckpt.pth"))
    (home / "model.json").write_text(json.dumps(dict(cfgd, weight_seed=int(g["init_seed"]))))
    return dict(home=home, paths=paths, cfg=cfg, seed=int(g["init_seed"]))


def test_segment_in_the_wild_end_to_end_and_cli(wild_home, tmp_path):
    """Two JPEG files of different sizes with two and three class names, drop_iter 1 (only the 1-drop branch exists) and 4 (the
    COCO driver's rule: only the N-drop branch runs): the label maps are those of Segmenter.run on the same inputs, the
    overlay files are Pillow's encoding of the numpy overlay of those labels, and the command line writes exactly those files
    and no histogram directory."""
    import argparse
    import warnings
    from pnp_ovss import hip, synth, wild
    from pnp_ovss.model import Segmenter, build_model
    ids = sorted(WILD_NAMES)
    names = [WILD_NAMES[i] for i in ids]
    files = [open(wild_home["paths"][i], "rb").read() for i in ids]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = build_model(cfg=wild_home["cfg"], max_batch=2, max_text_len=32, stash_layer=7, bf16=False,
                            checkpoint=str(wild_home["home"] / "ckpt.pth"), seed=wild_home["seed"])
        # an engine reserves its post-processing workspace once: the direct Segmenter gets an engine of its own on the same weights
        direct = build_model(cfg=wild_home["cfg"], max_batch=2, max_text_len=32, stash_layer=7, bf16=False, donor=model)
    seg = Segmenter(direct, "coco_object", 4, threshold=0.15, postprocess="blur+crf", max_pixels_per_image=56 * 50, max_channels=4,
                    class_ids=[1, 2, 3])
    results = {}
    for drop_iter in (1, 4):
        args = argparse.Namespace(img_size=64, drop_iter=drop_iter, max_att_block_num=8, prune_att_head="9", threshold=0.15,
                                  postprocess="blur+crf", batch_size=2)
        res = wild.segment_in_the_wild(model, args, [wild_home["paths"][ids[0]], files[1]], names, ids)      # a path and the bytes
        org = hip.jpeg_decode_batch(files)
        imgs = hip.preprocess_images(org, 64, synth.CLIP_MEAN, synth.CLIP_STD)
        l1, ln = seg.run(args, imgs, wild.captions_of(names), [[0, 1], [0, 1, 2]], org, None)
        assert (l1 is None) == (drop_iter >= 3) and (ln is None) == (drop_iter == 1)
        maps = [x.cpu().numpy() for x in (ln if ln is not None else l1)]
        for r, i, lab, o in zip(res, ids, maps, org):
            assert r.id == i and r.branch == ("1_drop" if drop_iter == 1 else "N_drop")
            assert r.labels.dtype == np.uint8 and r.labels.shape == WILD_SIZES[i] and np.array_equal(r.labels, lab), (i, drop_iter)
            assert int(r.labels.max()) <= len(WILD_NAMES[i])
            print(f"[measured] wild drop_iter {drop_iter} {i}: label counts {np.bincount(r.labels.reshape(-1), minlength=4).tolist()}")
            assert r.jpeg == R.pillow_jpeg(R.overlay_ref(lab, o.cpu().numpy()), 75), (i, drop_iter)
        results[drop_iter] = res
        no_vis = wild.segment_in_the_wild(model, args, files, names, ids, overlays=False)
        assert all(r.jpeg is None and np.array_equal(r.labels, q.labels) for r, q in zip(no_vis, res))
    direct.engine.close()
    model.engine.close()
    # the command line: same files, nothing else
    save = tmp_path / "out"
    env = dict(os.environ, PNP_OVSS_MODEL_CONFIG=str(wild_home["home"] / "model.json"))
    for k in ("PNP_OVSS_DTYPE", "PNP_OVSS_CHECKPOINT", "PNP_OVSS_VOCAB", "PNP_OVSS_STASH_LAYER"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "pnp-ovss_amd", "PnP_OVSS_0514_updated_segmentation.py"), "--in_the_wild",
           "--wild_classes", str(wild_home["home"] / "names.json"), "--home_dir", str(wild_home["home"]), "--save_path", str(save),
           "--world_size", "1", "--img_size", "64", "--del_patch_num", "sort_thresh005", "--batch_size", "2",
           "--max_att_block_num", "8", "--drop_iter", "4", "--prune_att_head", "9", "--threshold", "0.15",
           "--postprocess", "blur+crf", "--checkpoint", str(wild_home["home"] / "ckpt.pth")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    assert sorted(os.listdir(save)) == ["0519_Segmentation"], "only the overlay directory: no histogram directories"
    written = sorted(os.path.basename(f) for f in glob.glob(str(save / "0519_Segmentation" / "*")))
    assert written == sorted([f"BLIP_N_drop_{i}_blur+crf.jpeg" for i in ids] + [f"{i}.npy" for i in ids])
    for r in results[4]:
        assert open(save / "0519_Segmentation" / f"BLIP_N_drop_{r.id}_blur+crf.jpeg", "rb").read() == r.jpeg
        assert np.array_equal(np.load(save / "0519_Segmentation" / f"{r.id}.npy"), r.labels)
