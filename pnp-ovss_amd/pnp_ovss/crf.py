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

Any number of pairwise terms over features of your own (pydensecrf's addPairwiseEnergy): grey-scale or multi-channel images, a
depth channel in the bilateral kernel, two bilateral scales, 1-D signals:

    solver = crf.FeatureCRF(max_batch=1, max_total_pixels=H * W, max_pixels_per_image=H * W, max_labels=K, max_terms=3)
    terms = [crf.Term(crf.position_features([(H, W)], 3), 3.0),
             crf.Term(crf.image_features([rgb], 50, 5), 5.0),
             crf.Term(crf.image_features([np.dstack([rgb, depth])], 80, (13, 13, 13, 0.1)), M)]      # (K, K) message weights
    labels, q = solver.run([U], terms, iters=10)

Features arrive divided by their kernel widths and are used as given; a term has 1 .. 6 of them (max_dims) and the solver is
sized for the worst case of d + 1 lattice points per pixel -- that is the contract.  [position_features, image_features of an
RGB image] with scalar weights is DenseCRF.run bit for bit.  The KL divergence is not available for feature terms.

The feature-term mean-field as a differentiable layer (gradients of the unary energies and of the compatibilities; the
features are constants):

    M = torch.eye(K, device="cuda").mul_(5).requires_grad_()                     # a learnable (K, K) compatibility
    (q,) = solver.marginals([U_dev.requires_grad_()], [crf.Term(feats, M)], iters=5)          # (K, H, W), on the autograd graph
    loss(q).backward()                                                            # U_dev.grad, M.grad
"""
import ctypes as C
import numbers

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


def message_weights(compat, nlabels, where):
    """pydensecrf's compat -> (Potts weight, None) for a number, (None, (K, K) float32 message weights) for a vector
    (diag(-v)) or a matrix (-0.5 * (m + m^T)).  The one place where the pydensecrf shims (shims/general, shims/nd) turn a
    label-cost compat into this module's message weights: densecrf's PottsCompatibility / DiagonalCompatibility /
    MatrixCompatibility as this project reads them, pinned by nothing the reference holds (shims/general/pydensecrf/densecrf.py)."""
    if isinstance(compat, numbers.Real) and not isinstance(compat, bool):
        return float(compat), None
    a = np.asarray(compat)
    if a.dtype.kind not in "fiu":
        raise ValueError(f"{where}: compat is a number or a numeric array, not {a.dtype}")
    a = a.astype(np.float32)
    if a.shape == (nlabels,):
        return None, np.ascontiguousarray(np.diag(-a))
    if a.shape == (nlabels, nlabels):
        return None, np.ascontiguousarray((-0.5 * (a + a.T)).astype(np.float32))
    raise ValueError(f"{where}: compat is a number, ({nlabels},) or ({nlabels}, {nlabels}), not shape {a.shape}")


def check_compat_labels(compat_k, labels, name):
    """A vector or matrix compatibility for compat_k labels needs that many labels in every image of the batch."""
    if compat_k and any(int(k) != compat_k for k in labels):
        raise ValueError(f"{name} is for {compat_k} labels, the batch has {[int(k) for k in labels]}: a vector or matrix "
                         f"compatibility needs that many labels in every image")


def _raise(lib, h, r, what):
    msg = lib.pnp_crf_last_error(h)
    msg = msg.decode() if msg else ""
    raise (ValueError if r == -22 else RuntimeError)(f"{what} failed ({r}): {msg}")


def _check_bounds(max_batch, max_total_pixels, max_pixels_per_image, max_labels):
    if not (1 <= int(max_batch) <= MAX_BATCH and 2 <= int(max_labels) <= MAX_LABELS and
            1 <= int(max_pixels_per_image) <= int(max_total_pixels)):
        raise ValueError(f"bad bounds: at most {MAX_BATCH} images per batch, 2..{MAX_LABELS} labels, "
                         f"max_pixels_per_image <= max_total_pixels")
    return int(max_batch), int(max_total_pixels), int(max_pixels_per_image), int(max_labels)


def _cat_device(parts, dtype, device):
    """Arrays or tensors, flattened and concatenated, as one device tensor of `dtype` (a numpy dtype)."""
    if all(isinstance(p, torch.Tensor) and p.is_cuda for p in parts):
        flat = [p.to(device).contiguous().reshape(-1) for p in parts]
        return torch.cat(flat) if len(flat) > 1 else flat[0]
    host = [np.ascontiguousarray(p.cpu().numpy() if isinstance(p, torch.Tensor) else p, dtype=dtype).reshape(-1) for p in parts]
    return torch.from_numpy(np.concatenate(host)).to(device)


class _Solver:
    """What DenseCRF and FeatureCRF share: the pnp_crf handle, its bounds, and the outputs of the batch that is set."""

    def _create(self, what, device, bounds, create, *more):
        if not torch.cuda.is_available():
            raise RuntimeError(f"pnp_ovss.crf.{what} needs a HIP device (no CPU fallback)")
        self.lib = hip.load_library()
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.device = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
        self.bounds = bounds
        self.h = C.c_void_p()
        r = getattr(self.lib, create)(self.device.index, *self.bounds, *more, C.byref(self.h))
        if r != 0:
            msg = self.lib.pnp_crf_last_error(self.h).decode() if self.h else "bad bounds, or no device"
            self.close()
            raise RuntimeError(f"{create} failed ({r}): {msg}")

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

    def batch_token(self):
        """Changes with every set_batch: whoever holds a stepwise inference can tell that the batch is no longer theirs."""
        return getattr(self, "_batches", 0)

    def _outputs(self, what, want_q, want_labels):
        if getattr(self, "_plan", None) is None:
            raise RuntimeError(f"pnp_ovss.crf.{type(self).__name__}.{what}: no batch is set (call set_batch or run first)")
        plan = self._plan[0]
        d_lab = torch.empty(plan["max_total_pixels"], dtype=torch.uint8, device=self.device) if want_labels else None
        d_q = torch.empty(plan["total_unary"], dtype=torch.float32, device=self.device) if want_q else None
        return d_q, d_lab

    def read(self, want_q=True, want_labels=True):
        """The current marginals and their argmax -> (labels, q) as run() returns them (None where not wanted)."""
        d_q, d_lab = self._outputs("read", want_q, want_labels)
        with torch.cuda.device(self.device):
            r = self.lib.pnp_crf_read(self.h, hip._ptr(d_q), hip._ptr(d_lab), hip._stream())
        if r != 0:
            _raise(self.lib, self.h, r, "pnp_crf_read")
        return self._split(d_q, d_lab)

    # ---- a term's lattice stage by stage (pnp_crf_lattice_view_get / pnp_crf_probe_filter): for tests
    def _view(self, term):
        self._outputs("lattice_arrays", False, False)
        v = hip.PnpCrfLatticeView()
        r = self.lib.pnp_crf_lattice_view_get(self.h, int(term), C.byref(v))
        if r != 0:
            _raise(self.lib, self.h, r, "pnp_crf_lattice_view_get")
        return v

    def lattice_arrays(self, term):
        """The lattice of `term` (0 .. T - 1 of a terms batch; 0 Gaussian / 1 bilateral) as the last set_batch built it: a dict
        of numpy arrays trimmed to their live sizes -- M = idbase[B] points, E = pixels * D1 entries.  bary (E,) float32; offset,
        vals (E,); ent (E,) records (pixel, w, nr, pad); seg_lo, seg_hi (M,); idbase (B + 1,); n1, n2 (D1, M); nbr8 (D1 // 2, M, 8)
        image-local ids in the order ia, id, pa, pd, aa, ad, da, dd; norm (pixels,); and the numbers D1, cap, points."""
        v = self._view(term)
        D1, M, E, B, cap = int(v.D1), int(v.points), int(v.entries), int(v.images), int(v.cap)

        def arr(ptr, count, dtype):
            # count 4-byte words at ptr as a host array of dtype (read as int32 bits, whatever they hold)
            t = torch.as_tensor(hip._DevView(ptr, (count,), "<i4"), device=self.device)
            return t.cpu().numpy().view(dtype)
        i4, u4, f4 = np.int32, np.uint32, np.float32
        with torch.cuda.device(self.device):
            torch.cuda.synchronize()
            out = dict(D1=D1, cap=cap, points=M, bary=arr(v.bary, E, f4), offset=arr(v.offset, E, i4), vals=arr(v.vals, E, u4),
                       seg_lo=arr(v.seg_lo, M, i4), seg_hi=arr(v.seg_hi, M, i4), idbase=arr(v.idbase, B + 1, i4),
                       norm=arr(v.norm, E // D1, f4))
            out["ent"] = arr(v.ent, 4 * E, i4).view(np.dtype([("pixel", "<u4"), ("w", "<f4"), ("nr", "<f4"), ("pad", "<u4")]))
            # the axis tables have rows of `cap` points: the live part of every row
            out["n1"] = np.stack([arr(v.n1 + 4 * j * cap, M, i4) for j in range(D1)])
            out["n2"] = np.stack([arr(v.n2 + 4 * j * cap, M, i4) for j in range(D1)])
            out["nbr8"] = np.stack([arr(v.nbr8 + 32 * p * cap, 8 * M, i4).reshape(M, 8) for p in range(D1 // 2)])
        return out

    PROBE_STAGES = {"splat": 0, "forward": 1, "reverse": 2, "slice": 3}        # PNP_CRF_PROBE_*

    def probe_filter(self, term, stage, planes, out=None):
        """pnp_crf_probe_filter: part of one filter pass of `term` on `planes` -- a device float32 tensor laid out as the unary
        energies of the batch, (K_b, H_b * W_b) blocks back to back -- through the mean-field's own kernels.  stage: "splat",
        "forward", "reverse" -> per image a (M_b, K_b) device tensor of lattice value rows in id order; "slice" -> per image the
        (K_b, H_b, W_b) message.  out: a device float32 buffer to write into (default: a new one).  Overwrites the solver's
        marginals (start() anew)."""
        self._outputs("probe_filter", False, False)
        plan, sizes, labels = self._plan
        if stage not in self.PROBE_STAGES:
            raise ValueError(f"stage is one of {sorted(self.PROBE_STAGES)}, not {stage!r}")
        if planes.dtype != torch.float32 or planes.numel() != plan["total_unary"]:
            raise ValueError("planes do not match the sizes and label counts of the batch")
        v = self._view(term)
        with torch.cuda.device(self.device):
            torch.cuda.synchronize()
            idbase = torch.as_tensor(hip._DevView(v.idbase, (int(v.images) + 1,), "<i4"), device=self.device).cpu().numpy()
        counts = [int(idbase[b + 1] - idbase[b]) for b in range(len(sizes))]
        need = plan["total_unary"] if stage == "slice" else sum(m * k for m, k in zip(counts, labels))
        if out is None:
            out = torch.empty(need, dtype=torch.float32, device=self.device)
        if out.dtype != torch.float32 or out.numel() < need:
            raise ValueError(f"out holds {out.numel()} floats, the stage writes {need}")
        with torch.cuda.device(self.device):
            r = self.lib.pnp_crf_probe_filter(self.h, int(term), self.PROBE_STAGES[stage], hip._ptr(planes), hip._ptr(out), hip._stream())
        if r != 0:
            _raise(self.lib, self.h, r, "pnp_crf_probe_filter")
        if stage == "slice":
            return self._split(out, None)[1]
        res, at = [], 0
        for m, k in zip(counts, labels):
            res.append(out[at:at + m * k].view(m, k))
            at += m * k
        return res

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


class DenseCRF(_Solver):
    """One pnp_crf solver: owns the device workspace for batches up to the given bounds."""

    def __init__(self, max_batch, max_total_pixels, max_pixels_per_image, max_labels, device=None):
        self._create("DenseCRF", device, _check_bounds(max_batch, max_total_pixels, max_pixels_per_image, max_labels), "pnp_crf_create")

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
        return _cat_device(us, np.float32, self.device), _cat_device(ims, np.uint8, self.device), sizes, labels

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


MAX_TERMS = 8            # PNP_CRF_MAX_TERMS
MAX_DIMS = 6             # PNP_CRF_MAX_DIMS: feature axes of one term


def plan_terms(sizes, labels, dims):
    """plan_batch for feature terms -- host arithmetic only.  dims: feature axes of every term.  Adds, per term (lists over the
    terms): tvoff -- per image, the float offset of its lattice value rows in the value buffers the terms take turns in (d + 1
    rows of Kp floats per pixel at most); foff -- per image, the float offset of its (d, H*W) block in the term's concatenated
    features; total_features -- floats of that concatenation.  value_floats: what the widest term needs of a value buffer.
    q_floats: the pixel-major marginal rows of the batch (sum of Kp * H * W), one block of pnp_crf_infer_terms_saved's history.
    And the further bounds a solver needs: max_terms, max_dims."""
    dims = [int(d) for d in dims]
    if not 1 <= len(dims) <= MAX_TERMS:
        raise ValueError(f"{len(dims)} terms: 1..{MAX_TERMS}")
    for t, d in enumerate(dims):
        if not 1 <= d <= MAX_DIMS:
            raise ValueError(f"term {t} has {d} feature axes: 1..{MAX_DIMS}")
    plan = plan_batch(sizes, labels)
    pix = [int(h) * int(w) for h, w in sizes]
    plan.update(tvoff=[], foff=[], total_features=[])
    for d in dims:
        voff, rows = [], 0
        for n, kp in zip(pix, plan["Kp"]):
            voff.append(rows)
            rows += (d + 1) * n * kp
        plan["tvoff"].append(voff)
        plan["foff"].append([d * p0 for p0 in plan["pix0"]])
        plan["total_features"].append(d * plan["max_total_pixels"])
    plan.update(value_floats=max((d + 1) * sum(n * kp for n, kp in zip(pix, plan["Kp"])) for d in dims),
                max_terms=len(dims), max_dims=max(dims), q_floats=sum(n * kp for n, kp in zip(pix, plan["Kp"])))
    return plan


def _f32_quotient(a, width):
    return np.asarray(a, dtype=np.float32) / np.float32(width)            # IEEE float32 division of float32 operands


def position_features(sizes, sxy):
    """Per image of sizes [(H, W)] the (2, H, W) float32 features x / sx, y / sy; sxy: a number or (sx, sy)."""
    sx, sy = _widths(sxy, 2, "sxy")
    out = []
    for h, w in sizes:
        yy, xx = np.mgrid[0:int(h), 0:int(w)]
        out.append(np.stack([_f32_quotient(xx, sx), _f32_quotient(yy, sy)]))
    return out


def image_features(images, sxy, schan):
    """Per image -- (H, W) or (H, W, C) of any real dtype, C + 2 <= 6 -- the (2 + C, H, W) float32 features x / sx, y / sy,
    channel_c / schan_c; sxy: a number or (sx, sy); schan: a number or one width per channel."""
    out = []
    for im in images:
        a = im.detach().cpu().numpy() if isinstance(im, torch.Tensor) else np.asarray(im)
        if a.ndim == 2:
            a = a[:, :, None]
        if a.ndim != 3 or not (np.issubdtype(a.dtype, np.floating) or np.issubdtype(a.dtype, np.integer)):
            raise ValueError(f"images are (H, W) or (H, W, C) of a real dtype, not {a.shape} {a.dtype}")
        if a.shape[2] + 2 > MAX_DIMS:
            raise ValueError(f"{a.shape[2]} channels and two positions are {a.shape[2] + 2} feature axes: at most {MAX_DIMS}")
        sc = _widths(schan, a.shape[2], "schan")
        pos = position_features([a.shape[:2]], sxy)[0]
        out.append(np.concatenate([pos, np.stack([_f32_quotient(a[:, :, c], sc[c]) for c in range(a.shape[2])])]))
    return out


class Term:
    """One pairwise term: features -- per image one (d, H, W) or (d, H*W) float32 array or device tensor, already divided by the
    kernel widths -- and a compatibility: a number (the Potts weight), or (K,) / (K, K) float32 message weights, used as given
    (compat_values).  A torch.Tensor compatibility -- 0-d, (K,) or (K, K), on the host or the device -- is also kept as given
    (`tensor`): FeatureCRF.marginals differentiates with respect to it."""

    def __init__(self, features, compat=1.0):
        self.features = list(features)
        if not self.features:
            raise ValueError("a term has one feature array per image, at least one image")
        for f in self.features:
            if not hasattr(f, "dtype") or f.dtype not in (np.float32, torch.float32):
                raise ValueError(f"features are float32, not {getattr(f, 'dtype', type(f).__name__)}")
            if f.ndim not in (2, 3):
                raise ValueError(f"features are (d, H, W) or (d, H*W), not {tuple(f.shape)}")
        self.tensor = compat if isinstance(compat, torch.Tensor) else None
        self.dims = int(self.features[0].shape[0])
        if any(int(f.shape[0]) != self.dims for f in self.features):
            raise ValueError(f"a term has the same feature axes in every image, not {[int(f.shape[0]) for f in self.features]}")
        if not 1 <= self.dims <= MAX_DIMS:
            raise ValueError(f"a term has 1..{MAX_DIMS} feature axes, not {self.dims}")
        if isinstance(compat, (int, float, np.integer, np.floating)) or (hasattr(compat, "ndim") and compat.ndim == 0):
            self.weight, self.compat = float(compat.detach()) if isinstance(compat, torch.Tensor) else float(compat), None
        else:
            self.weight, self.compat = 0.0, compat
        self.kind, self.values, self.K = compat_values(self.compat, "compat")


class FeatureCRF(_Solver):
    """A pnp_crf solver of pnp_crf_create_terms: up to max_terms pairwise terms of up to max_dims features each, sized for the
    worst case of max_dims + 1 lattice points per pixel and term."""

    def __init__(self, max_batch, max_total_pixels, max_pixels_per_image, max_labels, max_terms=4, max_dims=6, device=None):
        if not (1 <= int(max_terms) <= MAX_TERMS and 1 <= int(max_dims) <= MAX_DIMS):
            raise ValueError(f"bad bounds: 1..{MAX_TERMS} terms of 1..{MAX_DIMS} feature axes")
        self.max_terms, self.max_dims = int(max_terms), int(max_dims)
        self._create("FeatureCRF", device, _check_bounds(max_batch, max_total_pixels, max_pixels_per_image, max_labels),
                     "pnp_crf_create_terms", self.max_terms, self.max_dims)

    def fits(self, plan):
        return _Solver.fits(self, plan) and plan["max_terms"] <= self.max_terms and plan["max_dims"] <= self.max_dims

    def _check_terms(self, terms):
        terms = list(terms)
        if not 1 <= len(terms) <= self.max_terms:
            raise ValueError(f"{len(terms)} terms: the solver holds 1..{self.max_terms}")
        for t, term in enumerate(terms):
            if not isinstance(term, Term):
                raise ValueError(f"term {t} is a pnp_ovss.crf.Term, not {type(term).__name__}")
            if term.dims > self.max_dims:
                raise ValueError(f"term {t} has {term.dims} feature axes: the solver holds 1..{self.max_dims}")
        return terms

    def _gather(self, unaries, terms):
        """-> (device unary floats, per term the device feature floats, sizes, labels), concatenated in batch order."""
        if not len(unaries):
            raise ValueError("one unary array per image, at least one image")
        sizes, labels = [], []
        for i, u in enumerate(unaries):
            if u.dtype not in (np.float32, torch.float32):
                raise ValueError(f"unary energies are float32, not {u.dtype}")
            if u.ndim not in (2, 3):
                raise ValueError(f"unary energies are (K, H, W) or (K, H*W), not {tuple(u.shape)}")
            shaped = [a for a in [u] + [t.features[i] for t in terms if i < len(t.features)] if a.ndim == 3]
            size = (int(shaped[0].shape[1]), int(shaped[0].shape[2])) if shaped else (1, int(u.shape[1]))      # a 1-D signal: one row
            sizes.append(size)
            labels.append(int(u.shape[0]))
        for t, term in enumerate(terms):
            if len(term.features) != len(sizes):
                raise ValueError(f"term {t} has features for {len(term.features)} images, the batch has {len(sizes)}")
            for i, (f, (h, w)) in enumerate(zip(term.features, sizes)):
                if not (tuple(f.shape[1:]) == (h, w) or (f.ndim == 2 and int(f.shape[1]) == h * w)):
                    raise ValueError(f"term {t}, image {i}: features are ({term.dims}, {h}, {w}) or ({term.dims}, {h * w}), not {tuple(f.shape)}")
        for i, (u, (h, w)) in enumerate(zip(unaries, sizes)):
            if not (tuple(u.shape[1:]) == (h, w) or (u.ndim == 2 and int(u.shape[1]) == h * w)):
                raise ValueError(f"image {i}: unary energies are (K, {h}, {w}) or (K, {h * w}), not {tuple(u.shape)}")
        feats = [_cat_device(term.features, np.float32, self.device) for term in terms]
        return _cat_device(list(unaries), np.float32, self.device), feats, sizes, labels

    def run(self, unaries, terms, iters=10, want_q=True):
        """unaries: per image (K, H, W) or (K, H*W) float32 energies; terms: Term objects, in the order their messages are
        added.  The terms' compatibilities replace whatever the solver held.  Returns (labels, q) as DenseCRF.run does."""
        terms = self._check_terms(terms)
        d_unary, feats, sizes, labels = self._gather(unaries, terms)
        for t, term in enumerate(terms):
            check_compat_labels(term.K, labels, f"term {t}'s compat")
        self.set_batch(d_unary, feats, [term.dims for term in terms], sizes, labels)
        self.set_compat([term.compat for term in terms])
        return self.infer(iters=iters, weights=[term.weight for term in terms], want_q=want_q)

    def set_compat(self, compats):
        """pnp_crf_set_term_compat for terms 0 .. len(compats) - 1: None -> scalar (the weight of the call), (K,) -> diag(v),
        (K, K) -> the matrix; message weights, used as given.  Holds until changed, across batches."""
        for term, compat in enumerate(compats):
            kind, vals, k = compat_values(compat, f"term {term}'s compat")
            with torch.cuda.device(self.device):
                r = self.lib.pnp_crf_set_term_compat(self.h, term, kind, _f32p(vals) if vals is not None else None, k)
            if r != 0:
                _raise(self.lib, self.h, r, "pnp_crf_set_term_compat")

    def set_batch(self, d_unary, d_features, dims, sizes, labels):
        """pnp_crf_set_batch_terms on concatenated device tensors: d_unary float32, the (K_b, H_b * W_b) blocks back to back;
        d_features[t] float32, term t's (dims[t], H_b * W_b) blocks back to back.  Builds every lattice; synchronises."""
        self._plan = None
        plan = plan_terms(sizes, labels, dims)
        if len(dims) > self.max_terms or plan["max_dims"] > self.max_dims:
            raise ValueError(f"{len(dims)} terms of up to {plan['max_dims']} feature axes: the solver holds {self.max_terms} of {self.max_dims}")
        if d_unary.dtype != torch.float32 or d_unary.numel() != plan["total_unary"]:
            raise ValueError("d_unary does not match the sizes and label counts")
        if len(d_features) != len(dims) or any(f.dtype != torch.float32 or f.numel() != n for f, n in zip(d_features, plan["total_features"])):
            raise ValueError("d_features do not match the sizes and the terms' feature axes")
        H = np.array([s[0] for s in sizes], dtype=np.int32)
        W = np.array([s[1] for s in sizes], dtype=np.int32)
        K = np.array(labels, dtype=np.int32)
        batch = hip.PnpCrfBatch(len(sizes), hip._i32p(H), hip._i32p(W), hip._i32p(K), None, hip._ptr(d_unary))
        arr = (hip.PnpCrfTerm * len(dims))(*[hip.PnpCrfTerm(int(d), hip._ptr(f)) for d, f in zip(dims, d_features)])
        with torch.cuda.device(self.device):
            r = self.lib.pnp_crf_set_batch_terms(self.h, C.byref(batch), len(dims), arr, hip._stream())
        if r != 0:
            _raise(self.lib, self.h, r, "pnp_crf_set_batch_terms")
        self._plan = (plan, [(int(h), int(w)) for h, w in sizes], [int(k) for k in labels])
        self._batches = self.batch_token() + 1
        self._w = [1.0] * len(dims)

    def _weights(self, weights):
        n = len(self._plan[0]["tvoff"])
        w = self._w if weights is None else [float(x) for x in weights]
        if len(w) != n:
            raise ValueError(f"{len(w)} weights for {n} terms")
        self._w = w
        return (C.c_float * n)(*w)

    def infer(self, iters=10, weights=None, want_q=True, want_labels=True):
        """pnp_crf_infer_terms on the batch of the last set_batch -> (labels, q).  weights: one per term, the weight of a term
        left scalar (default: those of the last call, 1 at first); remembered for step()."""
        d_q, d_lab = self._outputs("infer", want_q, want_labels)
        w = self._weights(weights)
        with torch.cuda.device(self.device):
            r = self.lib.pnp_crf_infer_terms(self.h, int(iters), w, hip._ptr(d_q), hip._ptr(d_lab), hip._stream())
        if r != 0:
            _raise(self.lib, self.h, r, "pnp_crf_infer_terms")
        return self._split(d_q, d_lab)

    def start(self, weights=None):
        """Q = softmax(-U) on the batch of the last set_batch; weights: as infer()'s, for the steps that follow."""
        self._outputs("start", False, False)
        self._weights(weights)
        with torch.cuda.device(self.device):
            r = self.lib.pnp_crf_start(self.h, hip._stream())
        if r != 0:
            _raise(self.lib, self.h, r, "pnp_crf_start")

    def step(self, n=1):
        """n more mean-field updates from the current marginals: start(); step(a); step(b) leaves what infer(a + b) leaves."""
        self._outputs("step", False, False)
        with torch.cuda.device(self.device):
            r = self.lib.pnp_crf_step_terms(self.h, int(n), self._weights(None), hip._stream())
        if r != 0:
            _raise(self.lib, self.h, r, "pnp_crf_step_terms")

    def marginals(self, unaries, terms, iters=5):
        """run() as a differentiable function: per image the (K, H, W) float32 marginals after `iters` updates, attached to
        the autograd graph of the unaries (device tensors) and of every term's compatibility given as a torch.Tensor (0-d, (K,)
        or (K, K), host or device; its gradient comes back in that shape on that device).  Features are constants.  Labels
        are not differentiable and not returned.  The backward pass (pnp_crf_backward_terms) needs the batch of the forward
        still set on this solver and raises RuntimeError otherwise; it recomputes a term's message only where that term's
        compatibility needs a gradient; no double backward.  The first call allocates the gradient workspace."""
        if not torch.cuda.is_available():
            raise RuntimeError("pnp_ovss.crf.FeatureCRF.marginals needs a HIP device (no CPU fallback)")
        terms = self._check_terms(terms)
        for i, u in enumerate(unaries):
            if not (isinstance(u, torch.Tensor) and u.is_cuda):
                raise ValueError(f"image {i}: marginals() takes the unary energies as device tensors")
        _, feats, sizes, labels = self._gather([u.detach() for u in unaries], terms)
        for t, term in enumerate(terms):
            check_compat_labels(term.K, labels, f"term {t}'s compat")
        if not getattr(self, "_grad", False):
            with torch.cuda.device(self.device):
                r = self.lib.pnp_crf_reserve_grad(self.h)
            if r != 0:
                _raise(self.lib, self.h, r, "pnp_crf_reserve_grad")
            self._grad = True
        flat = [u.to(self.device).contiguous().reshape(-1) for u in unaries]
        d_unary = torch.cat(flat) if len(flat) > 1 else flat[0]
        # a compatibility that is no tensor (a number, a numpy vector or matrix) enters as a constant of the graph
        compats = [term.tensor if term.tensor is not None else
                   torch.from_numpy(np.array(term.compat, dtype=np.float32)) if term.compat is not None else torch.tensor(term.weight)
                   for term in terms]
        d_q = _Marginals.apply(self, feats, [term.dims for term in terms], sizes, labels, int(iters), d_unary, *compats)
        plan = self._plan[0]
        return [d_q[off:off + k * h * w].view(k, h, w) for (h, w), k, off in zip(sizes, labels, plan["off"])]

    def lattice_points(self):
        """Lattice points of every term over the whole batch of the last set_batch (at most d + 1 per pixel)."""
        self._outputs("lattice_points", False, False)
        return [int(self.lib.pnp_crf_lattice_points(self.h, t)) for t in range(len(self._plan[0]["tvoff"]))]

    def kl(self):
        raise NotImplementedError("pnp_ovss.crf.FeatureCRF.kl: the KL divergence is not available for feature terms (use DenseCRF)")


def _compat_host(t):
    """A compatibility tensor as run() takes it: None for a 0-d one (the weight of the call), else float32 on the host."""
    return None if t.ndim == 0 else t.detach().to("cpu", torch.float32).contiguous().numpy()


class _Marginals(torch.autograd.Function):
    """FeatureCRF.marginals: the concatenated unary tensor and one compatibility tensor per term -> the concatenated marginals."""

    @staticmethod
    def forward(ctx, solver, feats, dims, sizes, labels, iters, d_unary, *compats):
        solver.set_batch(d_unary.detach(), feats, dims, sizes, labels)
        solver.set_compat([_compat_host(c) for c in compats])
        plan = solver._plan[0]
        w = solver._weights([float(c) if c.ndim == 0 else 0.0 for c in compats])
        history = torch.empty((iters + 1) * plan["q_floats"], dtype=torch.float32, device=solver.device)
        d_q = torch.empty(plan["total_unary"], dtype=torch.float32, device=solver.device)
        with torch.cuda.device(solver.device):
            r = solver.lib.pnp_crf_infer_terms_saved(solver.h, iters, w, hip._ptr(history), hip._ptr(d_q), None, hip._stream())
        if r != 0:
            _raise(solver.lib, solver.h, r, "pnp_crf_infer_terms_saved")
        ctx.solver, ctx.iters, ctx.token = solver, iters, solver.batch_token()
        # copies: backward re-sends the compatibilities this history was computed with, whatever an optimiser step (an in-place
        # update autograd's version check would not see on these) has made of the caller's tensors since
        ctx.compats = [c.detach().clone() for c in compats]
        ctx.save_for_backward(history)
        return d_q

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_q):
        solver, compats = ctx.solver, ctx.compats
        if solver.batch_token() != ctx.token or getattr(solver, "_plan", None) is None:
            raise RuntimeError("pnp_ovss.crf.FeatureCRF.marginals: backward needs the batch of its forward, but the solver has been "
                               "given another batch since (set_batch / run / marginals); run the forward again")
        (history,) = ctx.saved_tensors
        plan = solver._plan[0]
        solver.set_compat([_compat_host(c) for c in compats])     # the compatibilities of the forward, whatever came since
        w = (C.c_float * len(compats))(*[float(c) if c.ndim == 0 else 0.0 for c in compats])
        need = ctx.needs_input_grad[7:]
        outs = [torch.empty(max(c.numel(), 1), dtype=torch.float32, device=solver.device) if n else None for c, n in zip(compats, need)]
        ptrs = (C.c_void_p * len(compats))(*[o.data_ptr() if o is not None else None for o in outs])
        g_unary = torch.empty(plan["total_unary"], dtype=torch.float32, device=solver.device)
        grad_q = grad_q.to(solver.device, torch.float32).contiguous()
        with torch.cuda.device(solver.device):
            r = solver.lib.pnp_crf_backward_terms(solver.h, ctx.iters, w, hip._ptr(history), hip._ptr(grad_q), hip._ptr(g_unary), ptrs,
                                                  hip._stream())
        if r != 0:
            _raise(solver.lib, solver.h, r, "pnp_crf_backward_terms")
        g_compats = [o.reshape(c.shape).to(c.device, c.dtype) if o is not None else None for o, c in zip(outs, compats)]
        return (None,) * 6 + (g_unary if ctx.needs_input_grad[6] else None,) + tuple(g_compats)


_FEATURE_SOLVERS = {}    # device index -> the solver feature_solver() hands out there


def feature_solver(plan, device_index=None):
    """A module-level FeatureCRF of the device that holds batches of `plan` (plan_terms): re-created larger when a call needs
    more.  What shims/nd/pydensecrf runs on."""
    if not torch.cuda.is_available():
        raise RuntimeError("pnp_ovss.crf.feature_solver needs a HIP device (no CPU fallback)")
    idx = torch.cuda.current_device() if device_index is None else int(device_index)
    solver = _FEATURE_SOLVERS.get(idx)
    if solver is None or not solver.fits(plan):
        old = solver.bounds + (solver.max_terms, solver.max_dims) if solver is not None else (1, 0, 0, 2, 1, 1)
        if solver is not None:
            solver.close()
        grown = [max(o, plan[k]) for o, k in zip(old, ("max_batch", "max_total_pixels", "max_pixels_per_image", "max_labels",
                                                       "max_terms", "max_dims"))]
        solver = _FEATURE_SOLVERS[idx] = FeatureCRF(*grown, device=torch.device("cuda", idx))
    return solver


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
