"""Throughput of the device JPEG decoder against Pillow on the same synthetic files (GPU box only).

    python tools/jpeg_bench.py [--images 35] [--size 375x500] [--quality 90] [--reps 5] [--out gpurun_out/jpeg_bench.json]
    python tools/jpeg_bench.py --encode [--images 35] [--size 375x500] [--enc_quality 75] [--out profiles/jpeg_encode.json]

    python tools/jpeg_bench.py --progressive [--images 35] [--size 375x500] [--enc_quality 75] [--reps 30] [--out profiles/jpeg_progressive.json]

--progressive: the same images as Pillow's default PROGRESSIVE files (10 scans) through the scan-by-scan decoder
(pnp_jpeg_decode_scans): the batch between HIP events and end to end (hip.jpeg_decode_batch), per scan kind the kernel time and
the synchronisation rounds per segment, Pillow on one host thread for the same files, and the baseline files of the same images
through the baseline device decoder.  Its `device_faster` decides where the datasets send progressive files by default.

--encode: the other direction -- the same images, already on the device, through hip.jpeg_encode_batch (pnp_jpeg_encode: warm,
HIP events around the device work; the wall time of the whole call with its read-back and marker writing beside it) against
`Image.fromarray(rgb).save(buf, "JPEG", quality=q)` on one host thread.

Images are smooth colour fields plus texture noise (compressed size close to a VOC / COCO photograph of that size),
written with Pillow at 4:2:0.  Prints one JSON line: host marker walk (pack_batch), device time per batch by kernel
(HIP events), Pillow single-thread (what the reference's DataLoader does) and 8-thread decode times.
"""
import argparse
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "pnp-ovss_amd"))


def synth_photo(rng, H, W):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    img = np.zeros((H, W, 3), np.float32)
    for c in range(3):
        for _ in range(6):
            fx, fy, ph = rng.uniform(0.002, 0.05), rng.uniform(0.002, 0.05), rng.uniform(0, 6.28)
            img[..., c] += rng.uniform(10, 40) * np.sin(fx * xx + fy * yy + ph)
    img += 128 + rng.normal(0, 12, (H, W, 1)).astype(np.float32) + rng.normal(0, 4, (H, W, 3)).astype(np.float32)
    return np.clip(img, 0, 255).astype(np.uint8)


def encode_leg(a, H, W, rng):
    from PIL import Image
    import torch
    from pnp_ovss import hip, jpeg as J
    imgs = [synth_photo(rng, H, W) for _ in range(a.images)]

    def pil_one(im):
        b = io.BytesIO()
        Image.fromarray(im).save(b, "JPEG", quality=a.enc_quality)
        return b.getvalue()
    ref = [pil_one(im) for im in imgs]
    t0 = time.perf_counter()
    for _ in range(a.reps):
        for im in imgs:
            pil_one(im)
    t_pil1 = (time.perf_counter() - t0) / a.reps
    dev = [torch.from_numpy(im).cuda() for im in imgs]
    got = hip.jpeg_encode_batch(dev, a.enc_quality)                        # warm-up + the check
    exact = got == ref
    caps = [J.scan_capacity(H, W)] * a.images
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    hip.jpeg_encode_scans(dev, a.enc_quality, caps)
    ev_ms = []
    for _ in range(a.reps):                                                # device work only: events around the launch sequence
        torch.cuda.synchronize()
        e0.record()
        hip.jpeg_encode_scans(dev, a.enc_quality, caps)
        e1.record()
        torch.cuda.synchronize()
        ev_ms.append(e0.elapsed_time(e1))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.reps):
        hip.jpeg_encode_batch(dev, a.enc_quality)
    t_total = (time.perf_counter() - t0) / a.reps
    rec = dict(images=a.images, size=[H, W], quality=a.enc_quality, jpeg_bytes=sum(len(f) for f in ref), byte_exact_vs_pillow=bool(exact),
               pillow_1thread_ms=t_pil1 * 1e3, device_events_ms=float(np.median(ev_ms)), device_call_wall_ms=t_total * 1e3,
               note="device_events_ms spans concatenation, workspace allocation, the kernels and the length read-back of "
                    "jpeg_encode_scans; device_call_wall_ms is jpeg_encode_batch end to end (bytes objects on the host)",
               images_per_s=dict(pillow_1thread=a.images / t_pil1, device=a.images / t_total))
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


def progressive_leg(a, H, W, rng):
    from PIL import Image
    import torch
    from pnp_ovss import hip, jpeg as J
    imgs = [synth_photo(rng, H, W) for _ in range(a.images)]

    def save(im, **kw):
        b = io.BytesIO()
        Image.fromarray(im).save(b, "JPEG", quality=a.enc_quality, **kw)
        return b.getvalue()

    def pil_one(f):
        return np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))

    def wall(fn):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.reps * 1e3
    prog, base = [save(im, progressive=True) for im in imgs], [save(im) for im in imgs]
    ref = [pil_one(f) for f in prog]
    t_pil = {}
    for name, files in (("progressive", prog), ("baseline", base)):
        t0 = time.perf_counter()
        for _ in range(a.reps):
            for f in files:
                pil_one(f)
        t_pil[name] = (time.perf_counter() - t0) / a.reps * 1e3
    exact = all(np.array_equal(o.cpu().numpy(), r) for o, r in zip(hip.jpeg_decode_batch(prog), ref))
    t_total = wall(lambda: hip.jpeg_decode_batch(prog))
    t_base = wall(lambda: hip.jpeg_decode_batch(base))
    t0 = time.perf_counter()
    for _ in range(a.reps):
        J.pack_scans(prog)
    t_pack = (time.perf_counter() - t0) / a.reps * 1e3
    ctx = hip.jpeg_scans_upload(prog)
    hip.jpeg_scans_run(ctx)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev_ms = []
    for _ in range(a.reps):                                                # the device work only
        torch.cuda.synchronize()
        e0.record()
        hip.jpeg_scans_run(ctx)
        e1.record()
        torch.cuda.synchronize()
        ev_ms.append(e0.elapsed_time(e1))
    ctx = hip.jpeg_scans_upload(prog, profile=True)                        # one launch group at a time between events
    per_kind = {k: [] for k in J.SCAN_KINDS[1:]}
    for _ in range(a.reps):
        hip.jpeg_scans_run(ctx)
        for k, name in enumerate(J.SCAN_KINDS[1:], 1):
            per_kind[name].append(float(ctx["group_ms"][ctx["groups"][:, 2] == k].sum()))
    rounds = ctx["d_rounds"].cpu().numpy()
    kinds = np.array([ctx["scans"][g.scan].kind for g in ctx["segs"]])
    kind_ms = {name: float(np.median(v)) for name, v in per_kind.items()}
    total_kind = sum(kind_ms.values())
    stats = {name: dict(kernel_ms=kind_ms[name], share_of_scan_kernels=kind_ms[name] / total_kind, segments=int((kinds == k).sum()),
                        rounds_min=int(rounds[kinds == k].min()), rounds_median=float(np.median(rounds[kinds == k])),
                        rounds_max=int(rounds[kinds == k].max()))
             for k, name in enumerate(J.SCAN_KINDS[1:], 1)}
    rec = dict(images=a.images, size=[H, W], quality=a.enc_quality, reps=a.reps, script="Pillow default (10 scans)",
               jpeg_bytes=dict(progressive=sum(len(f) for f in prog), baseline=sum(len(f) for f in base)),
               bit_exact_vs_pillow=bool(exact), pillow_1thread_ms=t_pil["progressive"], pillow_1thread_baseline_files_ms=t_pil["baseline"],
               device_events_ms=float(np.median(ev_ms)), device_end_to_end_ms=t_total, host_pack_ms=t_pack,
               device_baseline_files_end_to_end_ms=t_base, scan_kinds=stats,
               device_faster=bool(t_total < t_pil["progressive"]),
               note="device_events_ms: one pnp_jpeg_decode_scans call on an uploaded batch between two events; device_end_to_end_ms: "
                    "hip.jpeg_decode_batch with the marker walk, packing, uploads and the error read-back; scan_kinds: kernel time per "
                    "kind with one synchronisation per launch group, rounds over the restart segments of that kind")
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


def main():
    from PIL import Image
    import torch
    from pnp_ovss import hip, jpeg as J
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=35)
    ap.add_argument("--size", default="375x500")
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--restart", type=int, default=0, help="restart interval in MCU rows (0 = none, what the datasets ship)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--encode", action="store_true", help="measure the device encoder against Pillow's instead of the decoder")
    ap.add_argument("--enc_quality", type=int, default=75)
    ap.add_argument("--progressive", action="store_true", help="measure the scan-by-scan decode of progressive files (quality: --enc_quality)")
    a = ap.parse_args()
    H, W = map(int, a.size.split("x"))
    rng = np.random.default_rng(0)
    if a.encode:
        return encode_leg(a, H, W, rng)
    if a.progressive:
        return progressive_leg(a, H, W, rng)
    files = []
    for _ in range(a.images):
        b = io.BytesIO()
        kw = dict(restart_marker_rows=a.restart) if a.restart else {}
        Image.fromarray(synth_photo(rng, H, W)).save(b, "JPEG", quality=a.quality, **kw)
        files.append(b.getvalue())
    nbytes = sum(len(f) for f in files)

    def pil_one(f):
        return np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))
    ref = [pil_one(f) for f in files]
    t0 = time.perf_counter()
    for _ in range(a.reps):
        for f in files:
            pil_one(f)
    t_pil1 = (time.perf_counter() - t0) / a.reps
    with ThreadPoolExecutor(8) as ex:
        list(ex.map(pil_one, files))
        t0 = time.perf_counter()
        for _ in range(a.reps):
            list(ex.map(pil_one, files))
        t_pil8 = (time.perf_counter() - t0) / a.reps

    out = hip.jpeg_decode_batch(files)
    exact = all(np.array_equal(o.cpu().numpy(), r) for o, r in zip(out, ref))
    t0 = time.perf_counter()
    for _ in range(a.reps):
        J.pack_batch(files)
    t_pack = (time.perf_counter() - t0) / a.reps
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.reps):
        hip.jpeg_decode_batch(files)
    torch.cuda.synchronize()
    t_total = (time.perf_counter() - t0) / a.reps
    rec = dict(images=a.images, size=[H, W], quality=a.quality, restart_rows=a.restart, jpeg_bytes=nbytes, bit_exact_vs_pillow=bool(exact),
               pillow_1thread_ms=t_pil1 * 1e3, pillow_8thread_ms=t_pil8 * 1e3, host_pack_ms=t_pack * 1e3,
               device_total_ms=t_total * 1e3, device_only_ms=(t_total - t_pack) * 1e3,
               images_per_s=dict(pillow_1thread=a.images / t_pil1, pillow_8thread=a.images / t_pil8, device=a.images / t_total))
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
