"""Stand-alone DenseCRF on the GPU: the mean-field of the post-processing stage (csrc/crf.hip) on unary energies of your own.

    from pnp_ovss import crf
    labels, q = crf.densecrf(U, image)                       # one image: U (K, H, W) float32, image (H, W, 3) uint8
    solver = crf.DenseCRF(max_batch=35, max_total_pixels=35 * 375 * 500, max_pixels_per_image=375 * 500, max_labels=21)
    labels, q = solver.run(unaries, images, iters=10)        # a batch: images of any sizes and label counts

What pydensecrf's DenseCRF2D computes for the reference (PnP_OVSS_0514_updated_segmentation.py:1063-1073): Potts
compatibility, one Gaussian term (weight pos_w, width pos_xy) and one bilateral term (weight bi_w, widths bi_xy / bi_rgb),
symmetric normalisation.  `shims/pydensecrf` offers the same under pydensecrf's own names.  There is NO CPU fallback.

Beyond the reference's call: per-axis widths (pos_xy=(sx, sy), bi_xy=(sx, sy), bi_rgb=(sr, sg, sb)); a label-compatibility
vector or matrix per term (pos_compat / bi_compat: message weights, used as given -- logit[l] = -U[l] + sum_k M[l][k] msg[k],
Potts weight w being M = w I); and stepwise inference with the KL divergence:

    solver.set_batch(...); solver.set_compat(None, M)        # or solver.run(..., iters=0, bi_compat=M)
    solver.start()
    for _ in range(10):
        solver.step(); print(solver.kl())                    # one float per image
    labels, q = solver.read()

`shims/general/pydensecrf` offers these under pydensecrf's names (a package of its own: `shims/pydensecrf` keeps refusing them).
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


COMPAT_SCALAR, COMPAT_DIAGONAL, COMPAT_MATRIX = 0, 1, 2      # PNP_CRF_COMPAT_* (include/pnp_hip.h)


def _f32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _widths(v, n, name):
    """A kernel width as n positive floats: a number (the same for every axis) or n values."""
    a = np.asarray(v, dtype=np.float64).reshape(-1)
    if a.size == 1:
        a = np.repeat(a, n)
    if a.size != n:
        raise ValueError(f"{name} is a number or {n} values, not {v!r}")
    if not (a > 0).all():
        raise ValueError(f"{name} must be positive, not {v!r}")
    return [float(x) for x in a]


def compat_values(compat, name):
    """None | (K,) | (K, K) message weights -> (kind, float32 values or None, K).  The weights are used as given: logit[l] =
    -U[l] + sum_k M[l][k] msg[k] with M = diag(vector) or the matrix (include/pnp_hip.h, pnp_crf_set_compat)."""
    if compat is None:
        return COMPAT_SCALAR, None, 0
    a = compat.detach().cpu().numpy() if isinstance(compat, torch.Tensor) else np.asarray(compat)
    if a.dtype != np.float32:
        raise ValueError(f"{name} is float32, not {a.dtype}")
    if a.ndim == 1 and 2 <= a.shape[0] <= MAX_LABELS:
        return COMPAT_DIAGONAL, np.ascontiguousarray(a), int(a.shape[0])
    if a.ndim == 2 and a.shape[0] == a.shape[1] and 2 <= a.shape[0] <= MAX_LABELS:
        return COMPAT_MATRIX, np.ascontiguousarray(a), int(a.shape[0])
    raise ValueError(f"{name} is None, (K,) or (K, K) with 2 <= K <= {MAX_LABELS}, not shape {a.shape}")


def check_compat_labels(compat_k, labels, name):
    """A vector or matrix compatibility for compat_k labels needs that many labels in every image of the batch."""
    if compat_k and any(int(k) != compat_k for k in labels):
        raise ValueError(f"{name} is for {compat_k} labels, the batch has {[int(k) for k in labels]}: a vector or matrix "
                         f"compatibility needs that many labels in every image")


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

    def run(self, unaries, images, iters=10, pos_w=7.0, pos_xy=3.0, bi_w=10.0, bi_xy=50.0, bi_rgb=5.0, want_q=True,
            pos_compat=None, bi_compat=None):
        """unaries: per image (K, H, W) or (K, H*W) float32 energies (-log p, pydensecrf's setUnaryEnergy); images: (H, W, 3)
        uint8; numpy arrays or device tensors.  pos_xy / bi_xy: a number or (sx, sy); bi_rgb: a number or (sr, sg, sb).
        pos_compat / bi_compat: None (Potts with pos_w / bi_w) or (K,) / (K, K) float32 message weights, used as given
        (set_compat); they replace whatever the solver held.  Returns (labels, q): lists of device tensors, (H, W) uint8 argmax
        labels and (K, H, W) float32 marginals (q is None when want_q is false)."""
        d_unary, d_rgb, sizes, labels = self._gather(unaries, images)
        kinds = [compat_values(pos_compat, "pos_compat"), compat_values(bi_compat, "bi_compat")]
        for (_, _, k), name in zip(kinds, ("pos_compat", "bi_compat")):
            check_compat_labels(k, labels, name)
        self.set_batch(d_unary, d_rgb, sizes, labels, pos_xy=pos_xy, bi_xy=bi_xy, bi_rgb=bi_rgb)
        self.set_compat(pos_compat, bi_compat)
        return self.infer(iters=iters, pos_w=pos_w, bi_w=bi_w, want_q=want_q)

    def set_compat(self, pos_compat=None, bi_compat=None):
        """pnp_crf_set_compat for both terms: None -> Potts (the weight of the call), (K,) -> diag(v), (K, K) -> the matrix;
        message weights, used as given.  Holds until changed, across batches."""
        for term, (compat, name) in enumerate(((pos_compat, "pos_compat"), (bi_compat, "bi_compat"))):
            kind, vals, k = compat_values(compat, name)
            with torch.cuda.device(self.device):
                r = self.lib.pnp_crf_set_compat(self.h, term, kind, _f32p(vals) if vals is not None else None, k)
            if r != 0:
                _raise(self.lib, self.h, r, "pnp_crf_set_compat")

    def set_batch(self, d_unary, d_rgb, sizes, labels, pos_xy=3.0, bi_xy=50.0, bi_rgb=5.0):
        """pnp_crf_set_batch_aniso on concatenated device tensors: d_unary float32, the (K_b, H_b * W_b) blocks back to back;
        d_rgb uint8, the (H_b, W_b, 3) images back to back.  pos_xy / bi_xy: a number or (sx, sy); bi_rgb: a number or
        (sr, sg, sb).  Builds the lattices for these widths; synchronises."""
        p2, b2, b3 = _widths(pos_xy, 2, "pos_xy"), _widths(bi_xy, 2, "bi_xy"), _widths(bi_rgb, 3, "bi_rgb")
        plan = plan_batch(sizes, labels)
        if d_unary.dtype != torch.float32 or d_unary.numel() != plan["total_unary"] or d_rgb.dtype != torch.uint8 or \
                d_rgb.numel() != 3 * plan["max_total_pixels"]:
            raise ValueError("d_unary / d_rgb do not match the sizes and label counts")
        H = np.array([s[0] for s in sizes], dtype=np.int32)
        W = np.array([s[1] for s in sizes], dtype=np.int32)
        K = np.array(labels, dtype=np.int32)
        batch = hip.PnpCrfBatch(len(sizes), hip._i32p(H), hip._i32p(W), hip._i32p(K), hip._ptr(d_rgb), hip._ptr(d_unary))
        self._plan = None
        f2, f3 = C.c_float * 2, C.c_float * 3
        with torch.cuda.device(self.device):
            r = self.lib.pnp_crf_set_batch_aniso(self.h, C.byref(batch), f2(*p2), f2(*b2), f3(*b3), hip._stream())
        if r != 0:
            _raise(self.lib, self.h, r, "pnp_crf_set_batch")
        self._plan = (plan, [(int(h), int(w)) for h, w in sizes], [int(k) for k in labels])
        self._batches = self.batch_token() + 1

    def batch_token(self):
        """Changes with every set_batch: whoever holds a stepwise inference can tell that the batch is no longer theirs."""
        return getattr(self, "_batches", 0)

    def _outputs(self, what, want_q, want_labels):
        if getattr(self, "_plan", None) is None:
            raise RuntimeError(f"pnp_ovss.crf.DenseCRF.{what}: no batch is set (call set_batch or run first)")
        plan = self._plan[0]
        d_lab = torch.empty(plan["max_total_pixels"], dtype=torch.uint8, device=self.device) if want_labels else None
        d_q = torch.empty(plan["total_unary"], dtype=torch.float32, device=self.device) if want_q else None
        return d_q, d_lab

    def infer(self, iters=10, pos_w=7.0, bi_w=10.0, want_q=True, want_labels=True):
        """pnp_crf_infer on the batch of the last set_batch -> (labels, q) as run() returns them (None where not wanted).
        pos_w / bi_w are remembered for step() and kl()."""
        d_q, d_lab = self._outputs("infer", want_q, want_labels)
        self._w = (float(pos_w), float(bi_w))
        with torch.cuda.device(self.device):
            r = self.lib.pnp_crf_infer(self.h, int(iters), float(pos_w), float(bi_w), hip._ptr(d_q), hip._ptr(d_lab), hip._stream())
        if r != 0:
            _raise(self.lib, self.h, r, "pnp_crf_infer")
        return self._split(d_q, d_lab)

    # ---- stepwise inference: start() -> step(n) ... -> read() / kl(), the loop of pydensecrf's startInference / stepInference
    def start(self, pos_w=None, bi_w=None):
        """Q = softmax(-U) on the batch of the last set_batch.  pos_w / bi_w: the weights of the terms left scalar for the
        steps that follow (default: those of the last infer / run / start, 7 and 10 at first)."""
        self._outputs("start", False, False)
        old = getattr(self, "_w", (DEFAULTS["pos_w"], DEFAULTS["bi_w"]))
        self._w = (old[0] if pos_w is None else float(pos_w), old[1] if bi_w is None else float(bi_w))
        with torch.cuda.device(self.device):
            r = self.lib.pnp_crf_start(self.h, hip._stream())
        if r != 0:
            _raise(self.lib, self.h, r, "pnp_crf_start")

    def step(self, n=1):
        """n more mean-field updates from the current marginals: start(); step(a); step(b) leaves what infer(a + b) leaves."""
        self._outputs("step", False, False)
        w = getattr(self, "_w", (DEFAULTS["pos_w"], DEFAULTS["bi_w"]))
        with torch.cuda.device(self.device):
            r = self.lib.pnp_crf_step(self.h, int(n), w[0], w[1], hip._stream())
        if r != 0:
            _raise(self.lib, self.h, r, "pnp_crf_step")

    def read(self, want_q=True, want_labels=True):
        """The current marginals and their argmax -> (labels, q) as run() returns them (None where not wanted)."""
        d_q, d_lab = self._outputs("read", want_q, want_labels)
        with torch.cuda.device(self.device):
            r = self.lib.pnp_crf_read(self.h, hip._ptr(d_q), hip._ptr(d_lab), hip._stream())
        if r != 0:
            _raise(self.lib, self.h, r, "pnp_crf_read")
        return self._split(d_q, d_lab)

    def kl(self):
        """KL divergence of the current marginals, one float per image (pnp_crf_kl: densecrf's klDivergence as this project
        reads it).  One filter pass per term; synchronises."""
        self._outputs("kl", False, False)
        w = getattr(self, "_w", (DEFAULTS["pos_w"], DEFAULTS["bi_w"]))
        out = (C.c_double * len(self._plan[1]))()
        with torch.cuda.device(self.device):
            r = self.lib.pnp_crf_kl(self.h, w[0], w[1], out, hip._stream())
        if r != 0:
            _raise(self.lib, self.h, r, "pnp_crf_kl")
        return [float(v) for v in out]

    def _split(self, d_q, d_lab):
        plan, sizes, labels = self._plan
        want_q, want_labels = d_q is not None, d_lab is not None
        out_l, out_q = [] if want_labels else None, [] if want_q else None
        for (h, w), k, p0, off in zip(sizes, labels, plan["pix0"], plan["off"]):
            if want_labels:
                out_l.append(d_lab[p0:p0 + h * w].view(h, w))
            if want_q:
                out_q.append(d_q[off:off + k * h * w].view(k, h, w))
        return out_l, out_q


_SOLVERS = {}            # device index -> the solver densecrf() uses there


def _device_index(unary):
    dev = unary.device if isinstance(unary, torch.Tensor) and unary.is_cuda else torch.device("cuda", torch.cuda.current_device())
    return dev.index if dev.index is not None else torch.cuda.current_device()


def module_solver(unary):
    """The solver densecrf() last used for inputs like `unary` (None before the first call): it holds that call's batch, for
    start / step / read / kl."""
    return _SOLVERS.get(_device_index(unary))


def densecrf(unary, image, **params):
    """One image through a module-level solver of its device (re-created larger when a call needs more): returns
    (labels (H, W) uint8, q (K, H, W) float32) as device tensors.  params: DenseCRF.run's."""
    if not torch.cuda.is_available():
        raise RuntimeError("pnp_ovss.crf.densecrf needs a HIP device (no CPU fallback)")
    idx = _device_index(unary)
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
