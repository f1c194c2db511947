"""In-the-wild segmentation: the caller's images and the caller's class names, no dataset tree, no ground truth, no histogram
-- the `args.in_the_wild` branch of the reference's COCO driver (PnP_OVSS_0514_updated_segmentation_coco.py:351-384, 594-595),
whose class lists are literals in the source; here they are arguments.

Rules (those of the COCO-Object driver, as pnp_ovss.model.Segmenter implements them for "coco_object"): caption
"A picture of " + " ".join(names) (:384); Scale_0_1 on both branches; the 1-drop branch only when drop_iter < 3; always a
background channel.  The label remap is the identity: label = position of the name in the image's list + 1, 0 = background.
Images are decoded on the device (hip.jpeg_decode_batch, Pillow for the files it does not cover) and resized there
(hip.preprocess_images); the overlays are rendered and JPEG-encoded there too (pnp_ovss.vis), and so are the label maps' PNG
files (hip.png_encode_batch)."""
import collections
import glob
import json
import os

import numpy as np

WildResult = collections.namedtuple("WildResult", "id labels jpeg branch png", defaults=(None,))
WildResult.__doc__ = """id; labels: uint8 (H, W) numpy label map; jpeg: the overlay file's bytes (None without overlays);
branch: "N_drop", or "1_drop" when the N-drop branch did not run (drop_iter 1); png: the label map as an 8-bit PNG file's bytes
(None unless asked for)."""

MAX_CLASSES = 255          # uint8 label maps, 0 = background


def check_inputs(images, class_names, ids=None):
    """Host-only validation (no device is touched): one non-empty list of names per image, one id per image.
    Returns the ids (default: 0, 1, ...)."""
    images, class_names = list(images), list(class_names)
    if len(images) != len(class_names):
        raise ValueError(f"{len(images)} images but {len(class_names)} class-name lists: one list per image")
    ids = list(range(len(images))) if ids is None else list(ids)
    if len(ids) != len(images):
        raise ValueError(f"{len(images)} images but {len(ids)} ids")
    for i, names in zip(ids, class_names):
        if isinstance(names, str) or not len(names):
            raise ValueError(f"image {i}: the class names are a non-empty list of strings, not {names!r}")
        if len(names) > MAX_CLASSES:
            raise ValueError(f"image {i}: {len(names)} class names; label maps are uint8 (at most {MAX_CLASSES})")
        for n in names:
            if not isinstance(n, str) or not n.strip():
                raise ValueError(f"image {i}: class name {n!r} is not a non-empty string")
    return ids


def captions_of(class_names):
    return ["A picture of " + " ".join(names) for names in class_names]


def _load(image):
    """JPEG bytes stay bytes (decoded on the device); a path to a JPEG file is read, any other path goes through Pillow; an
    array is taken as (H, W, 3) uint8 RGB."""
    if isinstance(image, (bytes, bytearray)):
        return bytes(image)
    if isinstance(image, (str, os.PathLike)):
        from .datasets import _read_rgb
        return _read_rgb(os.fspath(image), True)
    a = np.asarray(image.cpu() if hasattr(image, "cpu") else image)
    if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8:
        raise ValueError(f"an image array is (H, W, 3) uint8, not {a.shape} {a.dtype}")
    return np.ascontiguousarray(a)


def decode_images(images, ids, device_progressive=None):
    """-> list of (H, W, 3) uint8 images, device tensors where the device decoded them (datasets._Base._decode_on_device: the
    batch decode of the dataset drivers, with its Pillow fall-back for files the device decoder does not cover).
    device_progressive: progressive files on the device (True) or with Pillow (False); None: the datasets' default."""
    from .datasets import _Base
    items = [(None, i, _load(im), None) for i, im in zip(ids, images)]
    return [it[2] for it in _Base._decode_on_device(None, items, device_progressive)]


RESERVE_PIXELS, RESERVE_CHANNELS = 640 * 640, 24       # post-processing workspace of the first call on a model, unless it needs more


def _segmenter(model, args, pixels, channels):
    """The model's Segmenter for in-the-wild batches.  An engine reserves its post-processing workspace once, so the Segmenter
    is made at the first call -- COCO-Object rules, identity remap (class_ids[j] = j + 1), bounds of at least RESERVE_* -- and
    kept on the model; a later call that needs more than was reserved is refused with the numbers."""
    from .model import Segmenter
    m = model.module if hasattr(model, "module") else model
    seg = getattr(m, "_wild_segmenter", None)
    if seg is None:
        seg = Segmenter(model, "coco_object", MAX_CLASSES + 1, max_pixels_per_image=max(pixels, RESERVE_PIXELS),
                        max_channels=max(channels, RESERVE_CHANNELS), crf_chunk=int(getattr(args, "crf_chunk", 0) or 0),
                        class_ids=list(range(1, MAX_CLASSES + 1)))
        m._wild_segmenter = seg
    px, ch, _ = seg._reserve
    if pixels > px or channels > ch:
        raise ValueError(f"this model's post-processing workspace was reserved for images of {px} pixels and {ch} channels; the "
                         f"batch needs {pixels} and {channels}: segment the largest images first, or on a new model")
    seg.threshold = 0.15 if getattr(args, "threshold", None) is None else float(args.threshold)
    seg.mode = args.postprocess
    return seg


def segment_in_the_wild(model, args, images, class_names, ids=None, overlays=True, png=False, png_palette="voc"):
    """images: JPEG bytes, file paths or (H, W, 3) uint8 arrays; class_names: one list of names per image.  args: the drivers'
    namespace -- img_size, drop_iter, max_att_block_num, prune_att_head, threshold, postprocess; optional batch_size (default:
    the engine's max_batch), crf_chunk.  Returns one WildResult per image: the uint8 label
    map of the N-drop branch (of the 1-drop branch when drop_iter is 1) and, with overlays=True, its colour overlay as JPEG
    bytes.  Overlay colours are stable per label (pnp_ovss.vis), not ranked per image as in the reference.  png=True adds the
    label map as an 8-bit PNG file (r.png), deflate-encoded on the device; png_palette: "voc", "overlay", a (256, 3) uint8
    array, or None / "grey" for a greyscale file (hip.png_encode_batch)."""
    ids = check_inputs(images, class_names, ids)
    images, class_names = list(images), [list(n) for n in class_names]
    if not images:
        return []
    import torch
    from . import hip, synth, vis
    if not torch.cuda.is_available():
        raise RuntimeError("pnp_ovss.wild.segment_in_the_wild needs a HIP device (no CPU fallback)")
    m = model.module if hasattr(model, "module") else model
    bs = int(getattr(args, "batch_size", 0) or 0) or int(m._engine.max_batch if getattr(m, "_engine", None) is not None else 8)
    rgb = decode_images(images, ids, getattr(args, "device_progressive", None))
    seg = _segmenter(model, args, max(int(x.shape[0]) * int(x.shape[1]) for x in rgb), max(len(n) for n in class_names) + 1)
    out = []
    for o in range(0, len(rgb), bs):
        org, names = rgb[o:o + bs], class_names[o:o + bs]
        imgs = hip.preprocess_images(org, int(args.img_size), synth.CLIP_MEAN, synth.CLIP_STD)       # COCO driver: bicubic, CLIP statistics
        prep = seg.prepare(captions_of(names), [list(range(len(n))) for n in names], org, None)
        l1, ln = seg.launch(args, imgs, prep)
        maps, branch = (ln, "N_drop") if ln is not None else (l1, "1_drop")
        files = [None] * len(org)
        if overlays:
            files = vis.encode_overlays(maps, prep["rgb"], prep["sizes"])
        pngs = hip.png_encode_batch(maps, png_palette) if png else [None] * len(org)
        for i, lab, f, pf in zip(ids[o:o + bs], maps, files, pngs):
            out.append(WildResult(i, lab.cpu().numpy().astype(np.uint8), f, branch, pf))
    return out


def vis_file_name(save_path, branch, img_id, postprocess):
    """The reference's overlay file (Draw_Segmentation_map, :974-977, filename 'BLIP_N_drop' / 'BLIP_1_drop')."""
    return f"{save_path}/0519_Segmentation/BLIP_{branch}_{img_id}_{postprocess}.jpeg"


def list_wild_images(home_dir):
    """{home_dir}/In_the_wild/*.jpeg|*.jpg -> [(id, path)], sorted by id (the file name without its extension)."""
    files = []
    for ext in ("jpeg", "jpg"):
        files += glob.glob(os.path.join(home_dir, "In_the_wild", f"*.{ext}"))
    return sorted((os.path.splitext(os.path.basename(f))[0], f) for f in files)


def load_wild_classes(path, ids):
    """--wild_classes FILE.json: {"id": ["name", ...]}.  An image without an entry is an error, not a skipped image."""
    if not path:
        raise SystemExit("--in_the_wild needs --wild_classes FILE.json ({\"image id\": [\"class name\", ...]})")
    with open(path) as f:
        table = json.load(f)
    missing = [i for i in ids if i not in table]
    if missing:
        raise SystemExit(f"--wild_classes {path}: no class names for image id(s) {missing}")
    return [table[i] for i in ids]


def run_cli(rank, world_size, args):
    """`--in_the_wild` of the command line: every image of {home_dir}/In_the_wild with the class names of --wild_classes ->
    {save_path}/0519_Segmentation/BLIP_N_drop_{id}_{postprocess}.jpeg (the overlay) and {id}.npy (the label map) beside it;
    with --save_png also {id}.png, the label map as an 8-bit PNG file with the palette of --png_palette.
    Ranks take every world_size-th image and write their own files; no collective, no histogram directories."""
    import torch
    from lavis.models import load_model_and_preprocess
    found = list_wild_images(args.home_dir)
    if not found:
        raise SystemExit(f"--in_the_wild: no *.jpeg / *.jpg under {args.home_dir}/In_the_wild")
    ids = [i for i, _ in found]
    names = load_wild_classes(args.wild_classes, ids)
    check_inputs([p for _, p in found], names, ids)
    mine = list(range(rank, len(found), world_size))
    if args.prune_att_head is None:
        raise SystemExit("--prune_att_head is required")
    dev_idx = 0 if getattr(args, "share_gpu", False) else rank
    torch.cuda.set_device(dev_idx)
    model, _, _ = load_model_and_preprocess(
        "blip_image_text_matching", "large", device=dev_idx, is_eval=True, img_size=args.img_size, max_batch=args.batch_size,
        stash_layer=args.max_att_block_num - 1, mode=args.dtype, checkpoint=args.checkpoint, vocab=args.vocab,
        max_text_len=min(512, max(64, 8 + 6 * max(len(n) for n in names))))
    os.makedirs(f"{args.save_path}/0519_Segmentation", exist_ok=True)
    save_png = bool(getattr(args, "save_png", False))
    res = segment_in_the_wild(model, args, [found[k][1] for k in mine], [names[k] for k in mine], [ids[k] for k in mine],
                              png=save_png, png_palette=getattr(args, "png_palette", "voc"))
    for r in res:
        with open(vis_file_name(args.save_path, r.branch, r.id, args.postprocess), "wb") as f:
            f.write(r.jpeg)
        np.save(f"{args.save_path}/0519_Segmentation/{r.id}.npy", r.labels)
        if save_png:
            with open(f"{args.save_path}/0519_Segmentation/{r.id}.png", "wb") as f:
                f.write(r.png)
    print(json.dumps({"in_the_wild": True, "rank": rank, "images": len(res), "branch": res[0].branch if res else None,
                      "out": f"{args.save_path}/0519_Segmentation"}), flush=True)
    return res
