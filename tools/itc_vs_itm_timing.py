#!/usr/bin/env python
"""Time BlipITM.forward(match_head="itc") against forward(match_head="itm") on ONE engine (same ViT work; the text-only pass of
the ITC head has no cross-attention sub-layers, then two 256-wide projections and a B x B similarity).

    python tools/itc_vs_itm_timing.py [--batch 35] [--img 336] [--mode bf16x3] [--iters 20] [--rounds 3] [--out FILE.json]

Needs an MI355X.  Both calls are warmed up, then timed in alternation (itm, itc, itm, ...) with device events around each call on
the current stream, `rounds` times `iters` calls each; the record holds every round's median so the spread is visible.  The
times include the host side of a call (tokenizer, H2D copy of the ids) -- it is the public call that is timed, not a kernel.
"""
import argparse
import json
import os
import statistics
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pnp-ovss_amd"))

import torch                                     # noqa: E402

from pnp_ovss import config as C, synth          # noqa: E402
from pnp_ovss.model import build_model           # noqa: E402

VOC = ("aeroplane bicycle bird boat bottle bus car cat chair cow table dog horse motorbike person pottedplant sheep sofa train "
       "tvmonitor")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=35)
    ap.add_argument("--img", type=int, default=336)
    ap.add_argument("--mode", default="bf16x3")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: a timing taken anywhere else says nothing")
    cfg = C.blip_itm_large(a.img)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = build_model(cfg=cfg, max_batch=a.batch, max_text_len=64, stash_layer=7, mode=a.mode, seed=0)
    _, imgs = synth.synth_images(a.batch, a.img, seed=1234)
    s = {"image": torch.from_numpy(imgs).cuda(), "text_input": ["A picture of " + VOC] * a.batch}
    L = int(m._tok_longest(s["text_input"]).input_ids.shape[1])

    def timed(head):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        m(s, match_head=head)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)
    for _ in range(a.warmup):
        timed("itm")
        timed("itc")
    rounds = []
    for _ in range(a.rounds):
        t = {"itm": [], "itc": []}
        for _ in range(a.iters):
            for head in ("itm", "itc"):
                t[head].append(timed(head))
        rounds.append({h: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for h, v in t.items()})
    rec = {"what": "BlipITM.forward per call, device events around the public call, itm / itc alternating on one engine",
           "device": torch.cuda.get_device_name(0), "mode": a.mode, "batch": a.batch, "img_size": a.img, "text_len": L,
           "iters_per_round": a.iters, "rounds": rounds,
           "itm_median_ms": statistics.median(r["itm"]["median_ms"] for r in rounds),
           "itc_median_ms": statistics.median(r["itc"]["median_ms"] for r in rounds)}
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
    m.engine.close()


if __name__ == "__main__":
    main()
