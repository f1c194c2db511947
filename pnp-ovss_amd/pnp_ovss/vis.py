"""Looking at a segmentation: colour overlays of label maps on their images, rendered (csrc/vis.hip) and baseline-JPEG encoded
(csrc/jpeg_enc.hip) on the device, next to the label maps and RGB buffers the post-processing leaves in HBM; only the finished
JPEG files cross to the host.  What the reference's Draw_Segmentation_map writes (PnP_OVSS_0514_updated_segmentation_coco.py:
966-983: skimage.color.label2rgb(kind="overlay", alpha=0.3, bg_label=0) saved by matplotlib).

One deliberate difference: the reference hands label2rgb no colours, so skimage cycles through its ten colours by the RANK of a
label among those present in the image -- a class changes colour from image to image.  Here the colour belongs to the class:
label l > 0 always gets colour (l - 1) % 10 of the same ten-colour cycle, whatever else the image holds."""
import numpy as np
import torch

from . import hip

# skimage.color.colorlabel.DEFAULT_COLORS, as their CSS values (matplotlib.colors.to_rgb) in 8 bits
PALETTE_NAMES = ("red", "blue", "yellow", "magenta", "green", "indigo", "darkorange", "cyan", "pink", "yellowgreen")
PALETTE_RGB = ((255, 0, 0), (0, 0, 255), (255, 255, 0), (255, 0, 255), (0, 128, 0), (75, 0, 130), (255, 140, 0), (0, 255, 255),
               (255, 192, 203), (154, 205, 50))


def default_palette():
    """uint8 [256, 3] indexed by label: row l > 0 is colour (l - 1) % 10 of the cycle; row 0 (background: the grey image) is unused."""
    pal = np.zeros((256, 3), dtype=np.uint8)
    pal[1:] = np.asarray(PALETTE_RGB, dtype=np.uint8)[np.arange(255) % 10]
    return pal


def render_overlays(label_views, rgb, sizes, palette=None, alpha=0.3):
    """label_views: the per-image uint8 (H, W) device label maps of a batch (Engine.split_labels); rgb: the batch's concatenated
    HWC uint8 device buffer (Segmenter.prepare's "rgb"); sizes: [(H, W)].  Returns the overlays as (H, W, 3) uint8 device
    views of one buffer: label 0 shows the grey image, label l > 0 the grey image blended with palette[l] (see the module text:
    colours are stable per class, unlike the reference's per-image ranks)."""
    sizes = [(int(h), int(w)) for h, w in sizes]
    if len(label_views) != len(sizes):
        raise ValueError("one label map per image")
    for v, (h, w) in zip(label_views, sizes):
        if tuple(v.shape) != (h, w):
            raise ValueError(f"label map {tuple(v.shape)} against image size {(h, w)}")
    labels = torch.cat([v.reshape(-1) for v in label_views]) if len(label_views) > 1 else label_views[0].contiguous().reshape(-1)
    off = np.concatenate([[0], np.cumsum([h * w for h, w in sizes])]).astype(np.int64)
    if rgb.numel() != 3 * int(off[-1]):
        raise ValueError(f"rgb holds {rgb.numel()} bytes, the sizes say {3 * int(off[-1])}")
    out = hip.overlay_labels(labels.to(torch.uint8), rgb.reshape(-1), off, default_palette() if palette is None else palette, alpha)
    return [out[3 * off[i]:3 * off[i + 1]].view(h, w, 3) for i, (h, w) in enumerate(sizes)]


def encode_overlays(label_views, rgb, sizes, palette=None, alpha=0.3, quality=75):
    """render_overlays + hip.jpeg_encode_batch: the overlay JPEG files of a batch as a list of bytes, equal to Pillow's
    `Image.fromarray(overlay).save(buf, "JPEG", quality=quality)` of the same overlays."""
    return hip.jpeg_encode_batch(render_overlays(label_views, rgb, sizes, palette, alpha), quality=quality)
