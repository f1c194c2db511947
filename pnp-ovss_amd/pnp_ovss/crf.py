"""Stand-alone DenseCRF on the GPU: the mean-field of the post-processing stage (csrc/crf.hip) on unary energies of your own.

    from pnp_ovss import crf
    labels, q = crf.densecrf(U, image)                       # one image: U (K, H, W) float32, image (H, W, 3) uint8
    solver = crf.DenseCRF(max_batch=35, max_total_pixels=35 * 375 * 500, max_pixels_per_image=375 * 500, max_labels=21)
    labels, q = solver.run(unaries, images, iters=10)        # a batch: images of any sizes and label counts

What pydensecrf's DenseCRF2D computes for the reference (PnP_OVSS_0514_updated_segmentation.py:1063-1073): Potts
compatibility, one Gaussian term (weight pos_w, width pos_xy) and one bilateral term (weight bi_w, widths bi_xy / bi_rgb),
symmetric normalisation.  `shims/pydensecrf` offers the same under pydensecrf's own names.  There is NO CPU fallback.
"""
import ctypes as C

import numpy as np
import torch

from . import hip

MAX_BATCH = 64           # images per batch (the image bits of the packed lattice key)
MAX_LABELS = 255         # uint8 labels

DEFAULTS = dict(iters=10, pos_w=7.0, pos_xy=3.0, bi_w=10.0, bi_xy=50.0, bi_rgb=5.0)      # PnP.py:1036-1041


def plan_batch(sizes, labels):
    """The layout pnp_crf_set_batch gives a batch -- host arithmetic only.  sizes: [(H, W)], labels: [K] per image.
    Per image (lists): Kp -- row stride of the pixel-major unary / Q arrays in floats (K padded to a multiple of 4); pix0 --
    index of its first pixel in the batch (labels and RGB are concatenated by pixel); off -- float offset of its (K, H*W)
    block in the concatenated unary input / marginal output; qoff -- float offset of its Kp * H * W block of rows; voff --
    (Gaussian, bilateral) float offsets of its lattice value blocks, 3 and 6 rows of Kp floats per pixel at most.
    And the bounds a solver needs for this batch: max_batch, max_total_pixels, max_pixels_per_image, max_labels."""
    sizes = [(int(h), int(w)) for h, w in sizes]
    labels = [int(k) for k in labels]
    if len(sizes) != len(labels) or not sizes:
        raise ValueError("one label count per image, at least one image")
    if len(sizes) > MAX_BATCH:
        raise ValueError(f"{len(sizes)} images: a batch holds at most {MAX_BATCH}")
    plan = dict(Kp=[], pix0=[], off=[], qoff=[], voff=[])
    pix = off = qoff = vg = vb = 0
    for (h, w), k in zip(sizes, labels):
        if h < 1 or w < 1:
            raise ValueError(f"bad image size {h} x {w}")
        if not 2 <= k <= MAX_LABELS:
            raise ValueError(f"{k} labels: 2..{MAX_LABELS}")
        kp = (k + 3) // 4 * 4
        n = h * w
        plan["Kp"].append(kp)
        plan["pix0"].append(pix)
        plan["off"].append(off)
        plan["qoff"].append(qoff)
        plan["voff"].append((vg, vb))
        pix += n
        off += k * n
        qoff += kp * n
        vg += 3 * n * kp
        vb += 6 * n * kp
    plan.update(max_batch=len(sizes), max_total_pixels=pix, max_pixels_per_image=max(h * w for h, w in sizes),
                max_labels=max(labels), total_unary=off)
    return plan


def _raise(lib, h, r, what):
    msg = lib.pnp_crf_last_error(h)
    msg = msg.decode() if msg else ""
    raise (ValueError if r == -22 else RuntimeError)(f"{what} failed ({r}): {msg}")


class DenseCRF:
    """One pnp_crf solver: owns the device workspace for batches up to the given bounds."""

    def __init__(self, max_batch, max_total_pixels, max_pixels_per_image, max_labels, device=None):
        if not torch.cuda.is_available():
            raise RuntimeError("pnp_ovss.crf.DenseCRF needs a HIP device (no CPU fallback)")
        if not (1 <= int(max_batch) <= MAX_BATCH and 2 <= int(max_labels) <= MAX_LABELS and
                1 <= int(max_pixels_per_image) <= int(max_total_pixels)):
            raise ValueError(f"bad bounds: at most {MAX_BATCH} images per batch, 2..{MAX_LABELS} labels, "
                             f"max_pixels_per_image <= max_total_pixels")
        self.lib = hip.load_library()
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.device = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
        self.bounds = (int(max_batch), int(max_total_pixels), int(max_pixels_per_image), int(max_labels))
        self.h = C.c_void_p()
        r = self.lib.pnp_crf_create(self.device.index, *self.bounds, C.byref(self.h))
        if r != 0:
            msg = self.lib.pnp_crf_last_error(self.h).decode() if self.h else "no device"
            self.close()
            raise RuntimeError(f"pnp_crf_create failed ({r}): {msg}")

    def close(self):
        if getattr(self, "h", None):
            self.lib.pnp_crf_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def allocated_bytes(self):
        return int(self.lib.pnp_crf_allocated_bytes(self.h))

    def fits(self, plan):
        b = self.bounds
        return (plan["max_batch"] <= b[0] and plan["max_total_pixels"] <= b[1] and plan["max_pixels_per_image"] <= b[2] and
                plan["max_labels"] <= b[3])

    def _gather(self, unaries, images):
        """-> (device unary floats, device rgb bytes, sizes, labels), both concatenated in batch order."""
        if len(unaries) != len(images) or not len(images):
            raise ValueError("one unary array per image, at least one image")
        sizes, labels, us, ims = [], [], [], []
        for u, im in zip(unaries, images):
            if im.ndim != 3 or int(im.shape[2]) != 3 or im.dtype not in (np.uint8, torch.uint8):
                raise ValueError(f"images are (H, W, 3) uint8, not {tuple(im.shape)} {im.dtype}")
            h, w = int(im.shape[0]), int(im.shape[1])
            if u.dtype not in (np.float32, torch.float32):
                raise ValueError(f"unary energies are float32, not {u.dtype}")
            if not ((u.ndim == 3 and tuple(u.shape[1:]) == (h, w)) or (u.ndim == 2 and int(u.shape[1]) == h * w)):
                raise ValueError(f"unary energies are (K, {h}, {w}) or (K, {h * w}), not {tuple(u.shape)}")
            sizes.append((h, w))
            labels.append(int(u.shape[0]))
            us.append(u)
            ims.append(im)

        def cat(parts, dtype):
            if all(isinstance(p, torch.Tensor) and p.is_cuda for p in parts):
                flat = [p.to(self.device).contiguous().reshape(-1) for p in parts]
                return torch.cat(flat) if len(flat) > 1 else flat[0]
            host = [np.ascontiguousarray(p.cpu().numpy() if isinstance(p, torch.Tensor) else p, dtype=dtype).reshape(-1) for p in parts]
            return torch.from_numpy(np.concatenate(host)).to(self.device)
        return cat(us, np.float32), cat(ims, np.uint8), sizes, labels

    def run(self, unaries, images, iters=10, pos_w=7.0, pos_xy=3.0, bi_w=10.0, bi_xy=50.0, bi_rgb=5.0, want_q=True):
        """unaries: per image (K, H, W) or (K, H*W) float32 energies (-log p, pydensecrf's setUnaryEnergy); images: (H, W, 3)
        uint8; numpy arrays or device tensors.  Returns (labels, q): lists of device tensors, (H, W) uint8 argmax labels and
        (K, H, W) float32 marginals (q is None when want_q is false)."""
        d_unary, d_rgb, sizes, labels = self._gather(unaries, images)
        self.set_batch(d_unary, d_rgb, sizes, labels, pos_xy=pos_xy, bi_xy=bi_xy, bi_rgb=bi_rgb)
        return self.infer(iters=iters, pos_w=pos_w, bi_w=bi_w, want_q=want_q)

    def set_batch(self, d_unary, d_rgb, sizes, labels, pos_xy=3.0, bi_xy=50.0, bi_rgb=5.0):
        """pnp_crf_set_batch on concatenated device tensors: d_unary float32, the (K_b, H_b * W_b) blocks back to back; d_rgb
        uint8, the (H_b, W_b, 3) images back to back.  Builds the lattices for these widths; synchronises."""
        plan = plan_batch(sizes, labels)
        if d_unary.dtype != torch.float32 or d_unary.numel() != plan["total_unary"] or d_rgb.dtype != torch.uint8 or \
                d_rgb.numel() != 3 * plan["max_total_pixels"]:
            raise ValueError("d_unary / d_rgb do not match the sizes and label counts")
        H = np.array([s[0] for s in sizes], dtype=np.int32)
        W = np.array([s[1] for s in sizes], dtype=np.int32)
        K = np.array(labels, dtype=np.int32)
        batch = hip.PnpCrfBatch(len(sizes), hip._i32p(H), hip._i32p(W), hip._i32p(K), hip._ptr(d_rgb), hip._ptr(d_unary))
        self._plan = None
        with torch.cuda.device(self.device):
            r = self.lib.pnp_crf_set_batch(self.h, C.byref(batch), float(pos_xy), float(bi_xy), float(bi_rgb), hip._stream())
        if r != 0:
            _raise(self.lib, self.h, r, "pnp_crf_set_batch")
        self._plan = (plan, [(int(h), int(w)) for h, w in sizes], [int(k) for k in labels])

    def infer(self, iters=10, pos_w=7.0, bi_w=10.0, want_q=True, want_labels=True):
        """pnp_crf_infer on the batch of the last set_batch -> (labels, q) as run() returns them (None where not wanted)."""
        if getattr(self, "_plan", None) is None:
            raise RuntimeError("pnp_ovss.crf.DenseCRF.infer: no batch is set (call set_batch or run first)")
        plan, sizes, labels = self._plan
        d_lab = torch.empty(plan["max_total_pixels"], dtype=torch.uint8, device=self.device) if want_labels else None
        d_q = torch.empty(plan["total_unary"], dtype=torch.float32, device=self.device) if want_q else None
        with torch.cuda.device(self.device):
            r = self.lib.pnp_crf_infer(self.h, int(iters), float(pos_w), float(bi_w), hip._ptr(d_q), hip._ptr(d_lab), hip._stream())
        if r != 0:
            _raise(self.lib, self.h, r, "pnp_crf_infer")
        out_l, out_q = [] if want_labels else None, [] if want_q else None
        for (h, w), k, p0, off in zip(sizes, labels, plan["pix0"], plan["off"]):
            if want_labels:
                out_l.append(d_lab[p0:p0 + h * w].view(h, w))
            if want_q:
                out_q.append(d_q[off:off + k * h * w].view(k, h, w))
        return out_l, out_q


_SOLVERS = {}            # device index -> the solver densecrf() uses there


def densecrf(unary, image, **params):
    """One image through a module-level solver of its device (re-created larger when a call needs more): returns
    (labels (H, W) uint8, q (K, H, W) float32) as device tensors.  params: DenseCRF.run's."""
    if not torch.cuda.is_available():
        raise RuntimeError("pnp_ovss.crf.densecrf needs a HIP device (no CPU fallback)")
    dev = unary.device if isinstance(unary, torch.Tensor) and unary.is_cuda else torch.device("cuda", torch.cuda.current_device())
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    h, w = int(image.shape[0]), int(image.shape[1])
    plan = plan_batch([(h, w)], [int(unary.shape[0])])
    solver = _SOLVERS.get(idx)
    if solver is None or not solver.fits(plan):
        old = solver.bounds if solver is not None else (1, 0, 0, 2)
        if solver is not None:
            solver.close()
        pix = max(old[2], plan["max_pixels_per_image"])
        solver = _SOLVERS[idx] = DenseCRF(1, pix, pix, max(old[3], plan["max_labels"]), device=torch.device("cuda", idx))
    labels, q = solver.run([unary], [image], **params)
    return labels[0], (q[0] if q is not None else None)
