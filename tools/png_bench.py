"""Label maps as indexed PNG files: the device encoder (hip.png_encode_batch, csrc/png_enc.hip) against Pillow (GPU box only).

    python tools/png_bench.py [--images 35] [--size 375x500] [--reps 30] [--out profiles/png_encode.json]

The workload: label maps of one batch already on the device -- the blob maps of the test generator (tests/_png_refs.py) at 3, 8
and 21 classes in turn.  Warm.  Times: hip.png_encode_batch end to end (bytes objects on the host), the device work between HIP
events (hip.png_encode_streams: concatenation, workspace allocation, the kernels, the length read-back), and Pillow's
`save(buf, "PNG")` of the same maps as mode-P images with the same palette, at its default level and at compress_level=1, on one
host thread in the same process (the maps already on the host: the copy Pillow would need first is not counted).
Sizes, whole files: the device format, Pillow at both levels, and the same format with the filter forced to None and to Up for
every row -- what the per-row choice buys.  Prints one JSON line."""
import argparse
import io
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "pnp-ovss_amd"))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))

# bits of a match of length t at distance 1 under the fixed code: 7- or 8-bit length code + extra bits + 5-bit distance code
_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_MATCH_BITS = np.zeros(259, dtype=np.int64)
for _t in range(3, 259):
    _c = max(k for k in range(29) if _BASE[k] <= _t)
    _MATCH_BITS[_t] = (7 if 257 + _c < 280 else 8) + _EXTRA[_c] + 5


def stream_bytes(filt, H, W):
    """Length of the format's zlib stream for a filtered stream (the run / token rules, counted with numpy)."""
    rows = np.frombuffer(filt, dtype=np.uint8).reshape(H, W + 1)
    head = np.ones((H, W + 1), dtype=bool)
    head[:, 1:] = rows[:, 1:] != rows[:, :-1]
    pos = np.flatnonzero(head.reshape(-1))
    r = np.diff(np.append(pos, H * (W + 1)))
    b = rows.reshape(-1)[pos].astype(np.int64)
    lit = np.where(b < 144, 8, 9)
    rem = r - 1
    t = rem % 258
    bits = lit + (rem // 258) * _MATCH_BITS[258] + np.where(t >= 3, _MATCH_BITS[t], t * lit)
    return 2 + (10 + int(bits.sum()) + 7) // 8 + 4


def main():
    from PIL import Image
    import torch
    import _png_refs as R
    from pnp_ovss import hip, png
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=35)
    ap.add_argument("--size", default="375x500")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    H, W = map(int, a.size.split("x"))
    classes = [(3, 8, 21)[k % 3] for k in range(a.images)]
    maps = [R.blob_map(H, W, c, 100 + k) for k, c in enumerate(classes)]
    pal = png.voc_palette()

    def pil_one(lab, **kw):
        im = Image.fromarray(lab, "P")
        im.putpalette(pal.tobytes())
        b = io.BytesIO()
        im.save(b, "PNG", **kw)
        return b.getvalue()

    def pil_ms(**kw):
        t0 = time.perf_counter()
        for _ in range(a.reps):
            for lab in maps:
                pil_one(lab, **kw)
        return (time.perf_counter() - t0) / a.reps * 1e3
    pil_default = [pil_one(m) for m in maps]
    pil_l1 = [pil_one(m, compress_level=1) for m in maps]
    t_pil, t_pil1 = pil_ms(), pil_ms(compress_level=1)

    dev = [torch.from_numpy(m).cuda() for m in maps]
    got = hip.png_encode_batch(dev, pal)                                   # warm-up + the checks
    exact = all(got[k] == R.encode(maps[k], pal)[2] for k in range(min(3, a.images)))
    reads_back = all(np.array_equal(np.asarray(Image.open(io.BytesIO(f))), m) for f, m in zip(got, maps))
    framing = len(png.encode_chunks(H, W, b"", pal))
    sizes = {"device": [len(f) for f in got], "pillow_default": [len(f) for f in pil_default], "pillow_level1": [len(f) for f in pil_l1]}
    for name, force in (("filter_none_everywhere", 0), ("filter_up_everywhere", 2), ("filter_per_row", None)):
        sizes[name] = [framing + stream_bytes(R.filtered_stream(m, force)[0], H, W) for m in maps]
    assert sizes["filter_per_row"] == sizes["device"], "the size formula of this tool disagrees with the device's files"
    hip.png_encode_streams(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev_ms = []
    for _ in range(a.reps):                                                # device work only: events around the launch sequence
        torch.cuda.synchronize()
        e0.record()
        hip.png_encode_streams(dev)
        e1.record()
        torch.cuda.synchronize()
        ev_ms.append(e0.elapsed_time(e1))
    wall = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hip.png_encode_batch(dev, pal)
        wall.append((time.perf_counter() - t0) * 1e3)
    t_total = float(np.median(wall))
    tot = {k: int(sum(v)) for k, v in sizes.items()}
    by_classes = {str(c): {k: int(np.mean([v[i] for i in range(a.images) if classes[i] == c])) for k, v in sizes.items()}
                  for c in sorted(set(classes))}
    rec = dict(images=a.images, size=[H, W], classes=[3, 8, 21], reps=a.reps, raw_bytes=a.images * H * W,
               byte_exact_vs_reference=bool(exact), pillow_reads_labels_back=bool(reads_back),
               device_end_to_end_ms=t_total, device_end_to_end_ms_min_max=[float(min(wall)), float(max(wall))],
               device_events_ms=float(np.median(ev_ms)), pillow_default_1thread_ms=t_pil, pillow_level1_1thread_ms=t_pil1,
               images_per_s=dict(device=a.images / t_total * 1e3, pillow_default=a.images / t_pil * 1e3, pillow_level1=a.images / t_pil1 * 1e3),
               device_faster_than_pillow_level1=bool(t_total < t_pil1),
               file_bytes_total=tot, mean_file_bytes_by_classes=by_classes,
               size_ratio_device_to_pillow_default=tot["device"] / tot["pillow_default"],
               size_ratio_device_to_pillow_level1=tot["device"] / tot["pillow_level1"],
               per_row_choice_saves_vs_best_single_filter=1.0 - tot["device"] / min(tot["filter_none_everywhere"], tot["filter_up_everywhere"]),
               note="whole files with the 256-entry VOC palette on every side (780 bytes of PLTE chunk in each); device_events_ms spans "
                    "concatenation, workspace allocation, the kernels and the length read-back of png_encode_streams; "
                    "device_end_to_end_ms is png_encode_batch (median), bytes objects on the host; Pillow encodes host arrays, the "
                    "device-to-host copy it would need is not counted")
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
