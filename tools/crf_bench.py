"""Time of the stand-alone DenseCRF (pnp_ovss.crf, the pydensecrf shim) on the bench-shaped problem (GPU box only).

    timeout 900 python tools/crf_bench.py [--images 35] [--size 375x500] [--labels 21] [--reps 30] [--out profiles/crf_standalone.json]
    timeout 900 python tools/crf_bench.py --terms          # crf.FeatureCRF next to DenseCRF.run -> profiles/crf_terms.json
    timeout 900 python tools/crf_bench.py --grad           # the mean-field's backward pass -> profiles/crf_grad.json
    timeout 300 python tools/crf_bench.py --grad_errors    # its errors against the float64 reference -> `errors` of that record

Warm, then `reps` repetitions, device work between HIP events:
  one image through the shim      the host-to-host call (numpy in, numpy out: DenseCRF2D ... inference(10)), and separately the
                                  device-event time of set_batch (unary ingest + both lattice builds) and of infer
  `images` images in one run      DenseCRF.run, set_batch and infer likewise
  oracle/densecrf_ref.c           the same single-image problem on ONE host core: the only stand-in for pydensecrf that can run
                                  where pydensecrf is not installed -- it is the project's own C restatement, not pydensecrf
  the engine's own CRF stage      the same images and maps through Engine.densecrf(), timed by its stage profile
                                  (pnp_profile_read_stage 1: the mean-field iterations alone)
The maps come from the engine's own merge / upsample / blur stages on random patch-grid maps; the stand-alone runs get the
unary energies the engine computed from exactly those maps, so both paths must give the same bits (`agreement`).  Prints one
JSON line and writes it to --out.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "pnp-ovss_amd"))


def synth_photo(rng, H, W):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    img = np.zeros((H, W, 3), np.float32)
    for c in range(3):
        for _ in range(6):
            fx, fy, ph = rng.uniform(0.002, 0.05), rng.uniform(0.002, 0.05), rng.uniform(0, 6.28)
            img[..., c] += rng.uniform(10, 40) * np.sin(fx * xx + fy * yy + ph)
    img += 128 + rng.normal(0, 12, (H, W, 1)).astype(np.float32) + rng.normal(0, 4, (H, W, 3)).astype(np.float32)
    return np.clip(img, 0, 255).astype(np.uint8)


def events_ms(torch, fn, reps):
    """median device time of fn() between two events (fn may synchronise inside: the events are on the same stream)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(np.median(out))


def kernel_times_us(torch, fn):
    """Device time of every crf_update kernel launch inside fn(), by torch's profiler: {kernel family: [us per launch]}.
    Empty where the profiler reports no device kernels (the caller then records nothing rather than an estimate)."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    out = {"crf_update_compat_kernel": [], "crf_update_kernel": []}
    for ev in prof.events():
        if "DeviceType.CUDA" not in str(getattr(ev, "device_type", "")):
            continue
        us = getattr(ev, "device_time", None)
        if us is None:
            us = getattr(ev, "cuda_time", 0.0)
        for name in out:                                     # (the longer name first: it contains no other)
            if name in ev.name:
                out[name].append(float(us))
                break
    return out


def compat_matrix(torch, crf, a):
    """--compat matrix: one mean-field step (both filters + the update) with Potts weights against the same step with full
    matrices on both terms, and the update kernels' own device times per launch, at the tool's geometry and at K = 150."""
    H, W = map(int, a.size.split("x"))
    rng = np.random.default_rng(0)
    rec = {}
    for K, B in ((a.labels, a.images), (150, min(a.images, 8))):
        imgs = [synth_photo(rng, H, W) for _ in range(B)]
        d_rgb = torch.from_numpy(np.concatenate([im.reshape(-1) for im in imgs])).cuda()
        logits = torch.from_numpy(rng.normal(0, 2, (B, K, H * W)).astype(np.float32)).cuda()
        d_unary = (-torch.log_softmax(logits, 1).clamp_min(float(np.log(1e-5)))).contiguous().reshape(-1)
        del logits
        mats = [(np.diag(np.full(K, w)) + rng.uniform(-0.3 * w, 0, (K, K)) * (1 - np.eye(K))).astype(np.float32) for w in (7.0, 10.0)]
        solver = crf.DenseCRF(B, B * H * W, H * W, K)
        solver.set_batch(d_unary, d_rgb, [(H, W)] * B, [K] * B)
        one = {}
        for name, cm in (("potts", (None, None)), ("matrix", tuple(mats))):
            solver.set_compat(*cm)
            solver.start(7.0, 10.0)
            solver.step(2)                                                        # warm
            one[name + "_step_events_ms"] = events_ms(torch, lambda: solver.step(10), max(a.reps // 3, 3)) / 10
            kt = kernel_times_us(torch, lambda: solver.step(10))
            fam = "crf_update_kernel" if name == "potts" else "crf_update_compat_kernel"
            if len(kt[fam]) == 10:                                                # every launch seen, or nothing recorded
                one[name + "_update_kernel_us_per_launch"] = float(np.median(kt[fam]))
                one[name + "_update_kernel_us_min_max"] = [float(min(kt[fam])), float(max(kt[fam]))]
        solver.close()
        one.update(images=B)
        rec[f"K{K}"] = one
        del d_unary, d_rgb
        torch.cuda.empty_cache()
    rec["size"] = [H, W]
    rec["note"] = ("*_step_events_ms: one mean-field step = both lattice filters + one update launch, device events over 10 "
                   "steps; the two steps launch the same filter kernels, so their difference is the compatibility kernel's "
                   "launch minus the Potts kernel's.  *_update_kernel_us_per_launch: median device time of the update kernel's "
                   "10 launches as torch's profiler reports them (absent where it reported none).  Random unaries and random "
                   "matrices w I + U[-0.3 w, 0]: the arithmetic does not depend on the values")
    return rec


def terms_bench(torch, crf, a):
    """--terms: the feature-terms solver (crf.FeatureCRF) next to DenseCRF.run.  (a) the xy + xy.rgb problem through both, the
    two alternated repetition by repetition: set_batch and one mean-field step by device events, and whether the results are
    the same bits; (b) the same plus a third term xy / 80 . rgb / 13 . depth / 0.1 (D = 6): lattice points per pixel, ms per
    step, allocated bytes.  And the device time per launch of the iteration kernels inside the FeatureCRF steps."""
    H, W = map(int, a.size.split("x"))
    B, K = a.images, a.labels
    rng = np.random.default_rng(0)
    imgs = [synth_photo(rng, H, W) for _ in range(B)]
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    depth = [(0.5 + 0.4 * np.sin(xx / 7.0) * np.cos(yy / 5.0) + rng.normal(0, 0.02, (H, W))).astype(np.float32) for _ in range(B)]
    d_rgb = torch.from_numpy(np.concatenate([im.reshape(-1) for im in imgs])).cuda()
    logits = torch.from_numpy(rng.normal(0, 2, (B, K, H * W)).astype(np.float32)).cuda()
    d_unary = (-torch.log_softmax(logits, 1).clamp_min(float(np.log(1e-5)))).contiguous().reshape(-1)
    del logits
    sizes, labels = [(H, W)] * B, [K] * B

    def dev(parts):
        return torch.from_numpy(np.concatenate([p.reshape(-1) for p in parts])).cuda()
    d_pos = dev(crf.position_features(sizes, 3.0))
    d_bil = dev(crf.image_features(imgs, 50.0, 5.0))
    d_dep = dev(crf.image_features([np.dstack([im.astype(np.float32), dp]) for im, dp in zip(imgs, depth)], 80.0, (13.0, 13.0, 13.0, 0.1)))
    two = crf.DenseCRF(B, B * H * W, H * W, K)
    feat = crf.FeatureCRF(B, B * H * W, H * W, K, max_terms=3, max_dims=6)
    reps = a.reps

    def set_two():
        two.set_batch(d_unary, d_rgb, sizes, labels)

    def set_feat2():
        feat.set_batch(d_unary, [d_pos, d_bil], [2, 5], sizes, labels)

    def set_feat3():
        feat.set_batch(d_unary, [d_pos, d_bil, d_dep], [2, 5, 6], sizes, labels)

    def alternated(f0, f1, n):
        """medians of f0 / f1 by device events, one repetition of each in turn"""
        t0, t1 = [], []
        for _ in range(n):
            t0.append(events_ms(torch, f0, 1))
            t1.append(events_ms(torch, f1, 1))
        return float(np.median(t0)), float(np.median(t1))
    set_two()
    set_feat2()
    lab2, q2 = two.infer(10, 7.0, 10.0)
    labf, qf = feat.infer(10, [7.0, 10.0])
    same = all(bool(torch.equal(x, y)) for x, y in zip(q2, qf)) and all(bool(torch.equal(x, y)) for x, y in zip(lab2, labf))
    del lab2, q2, labf, qf
    set_two_ms, set_feat_ms = alternated(set_two, set_feat2, max(reps // 3, 3))
    two.start(7.0, 10.0)
    feat.start([7.0, 10.0])
    two.step(2)
    feat.step(2)                                                                 # warm
    step_two, step_feat = alternated(lambda: two.step(10), lambda: feat.step(10), reps)
    points2 = feat.lattice_points()

    def kernel_us(fn, launches):
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        fam = {"crf_term_update_kernel": [], "crf_splat_kernel": [], "crf_blur4x2_kernel": [], "crf_blur4_kernel": []}
        for ev in prof.events():
            if "DeviceType.CUDA" not in str(getattr(ev, "device_type", "")):
                continue
            us = getattr(ev, "device_time", None)
            if us is None:
                us = getattr(ev, "cuda_time", 0.0)
            for name in fam:
                if name in ev.name:
                    fam[name].append(float(us))
                    break
        return {k: dict(launches_per_step=len(v) / launches, us_per_step=float(np.sum(v)) / launches) for k, v in fam.items() if v}
    kern2 = kernel_us(lambda: feat.step(5), 5)
    a_rec = dict(densecrf_set_batch_ms=set_two_ms, featurecrf_set_batch_ms=set_feat_ms, densecrf_step_ms=step_two / 10,
                 featurecrf_step_ms=step_feat / 10, step_ratio=step_feat / step_two, bit_identical=bool(same),
                 lattice_points_per_pixel=[p / (B * H * W) for p in points2], featurecrf_kernels_us_per_step=kern2)
    set_feat3()
    feat.start([7.0, 10.0, 5.0])
    feat.step(2)
    set3_ms = events_ms(torch, set_feat3, max(reps // 3, 3))
    feat.start([7.0, 10.0, 5.0])
    step3 = events_ms(torch, lambda: feat.step(10), reps)
    b_rec = dict(set_batch_ms=set3_ms, step_ms=step3 / 10, lattice_points_per_pixel=[p / (B * H * W) for p in feat.lattice_points()],
                 allocated_bytes=feat.allocated_bytes(), featurecrf_kernels_us_per_step=kernel_us(lambda: feat.step(5), 5))
    rec = dict(images=B, size=[H, W], labels=K, reps=reps, two_terms=a_rec, three_terms=b_rec,
               densecrf_allocated_bytes=two.allocated_bytes(),
               note="two_terms: xy / 3 and xy / 50 . rgb / 5 with weights 7 / 10 through DenseCRF (the fused two-term update) and "
                    "through FeatureCRF (one slice-and-accumulate launch per term, the softmax in the last), alternated repetition "
                    "by repetition in one process; *_step_ms = device events over 10 mean-field steps / 10; set_batch = unary "
                    "ingest + every lattice build with its read-back (DenseCRF keeps its Gaussian lattice after the first call, "
                    "FeatureCRF caches none).  three_terms: plus xy / 80 . rgb / 13 . depth / 0.1 (D = 6), weight 5, depth = 0.5 + "
                    "0.4 sin(x / 7) cos(y / 5) + N(0, 0.02).  featurecrf_kernels_us_per_step: device time of the iteration "
                    "kernels per mean-field step as torch's profiler reports them.  Random unaries: the arithmetic does not "
                    "depend on the values")
    two.close()
    feat.close()
    return rec


def grad_bench(torch, crf, a):
    """--grad: the reverse mode of the feature-term mean-field (pnp_crf_infer_terms_saved / pnp_crf_backward_terms) on three terms
    -- xy / 3 (weight 7), xy / 50 . rgb / 5 (weight 10), xy / 80 . rgb / 13 . depth / 0.1 (a K x K matrix) -- and 5 iterations:
    the forward with and without the history, alternated; the backward with every compatibility gradient and with none,
    alternated; the bytes pnp_crf_reserve_grad adds; the device time of every kernel family of one backward call."""
    import ctypes as C
    from pnp_ovss import hip
    H, W = map(int, a.size.split("x"))
    B, K, iters = a.images, a.labels, 5
    rng = np.random.default_rng(0)
    imgs = [synth_photo(rng, H, W) for _ in range(B)]
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    depth = [(0.5 + 0.4 * np.sin(xx / 7.0) * np.cos(yy / 5.0) + rng.normal(0, 0.02, (H, W))).astype(np.float32) for _ in range(B)]
    logits = torch.from_numpy(rng.normal(0, 2, (B, K, H * W)).astype(np.float32)).cuda()
    d_unary = (-torch.log_softmax(logits, 1).clamp_min(float(np.log(1e-5)))).contiguous().reshape(-1)
    del logits
    sizes, labels = [(H, W)] * B, [K] * B

    def dev(parts):
        return torch.from_numpy(np.concatenate([p.reshape(-1) for p in parts])).cuda()
    feats = [dev(crf.position_features(sizes, 3.0)), dev(crf.image_features(imgs, 50.0, 5.0)),
             dev(crf.image_features([np.dstack([im.astype(np.float32), dp]) for im, dp in zip(imgs, depth)], 80.0, (13.0, 13.0, 13.0, 0.1)))]
    M = (5.0 * np.eye(K) + 0.3 * rng.normal(size=(K, K))).astype(np.float32)
    feat = crf.FeatureCRF(B, B * H * W, H * W, K, max_terms=3, max_dims=6)
    before = feat.allocated_bytes()
    r = feat.lib.pnp_crf_reserve_grad(feat.h)
    assert r == 0, feat.lib.pnp_crf_last_error(feat.h)
    reserved = feat.allocated_bytes() - before
    feat.set_batch(d_unary, feats, [2, 5, 6], sizes, labels)
    feat.set_compat([None, None, M])
    plan = feat._plan[0]
    w = (C.c_float * 3)(7.0, 10.0, 0.0)
    history = torch.empty((iters + 1) * plan["q_floats"], dtype=torch.float32, device="cuda")
    d_q = torch.empty(plan["total_unary"], dtype=torch.float32, device="cuda")
    grad_q = torch.from_numpy(rng.normal(size=plan["total_unary"]).astype(np.float32)).cuda()
    g_unary = torch.empty_like(d_q)
    g_compat = [torch.empty(1, device="cuda"), torch.empty(1, device="cuda"), torch.empty(K * K, device="cuda")]
    all_ptrs = (C.c_void_p * 3)(*[g.data_ptr() for g in g_compat])

    def check(r, what):
        assert r == 0, (what, feat.lib.pnp_crf_last_error(feat.h))

    def fwd_plain():
        check(feat.lib.pnp_crf_infer_terms(feat.h, iters, w, hip._ptr(d_q), None, hip._stream()), "infer_terms")

    def fwd_saved():
        check(feat.lib.pnp_crf_infer_terms_saved(feat.h, iters, w, hip._ptr(history), hip._ptr(d_q), None, hip._stream()), "infer_terms_saved")

    def bwd(ptrs):
        check(feat.lib.pnp_crf_backward_terms(feat.h, iters, w, hip._ptr(history), hip._ptr(grad_q), hip._ptr(g_unary), ptrs,
                                              hip._stream()), "backward_terms")

    def alternated(f0, f1, n):
        t0, t1 = [], []
        for _ in range(n):
            t0.append(events_ms(torch, f0, 1))
            t1.append(events_ms(torch, f1, 1))
        return float(np.median(t0)), float(np.median(t1)), [float(min(t0)), float(max(t0))], [float(min(t1)), float(max(t1))]
    fwd_plain()
    q_plain = d_q.clone()
    fwd_saved()
    same = bool(torch.equal(q_plain, d_q))
    del q_plain
    bwd(all_ptrs)
    first = [g.clone() for g in [g_unary] + g_compat]
    bwd(all_ptrs)                                                                 # warm; and the same bits twice
    deterministic = all(bool(torch.equal(x, y)) for x, y in zip(first, [g_unary] + g_compat))
    bwd(None)
    unary_same = bool(torch.equal(first[0], g_unary))
    reps = max(a.reps // 3, 5)
    f_plain, f_saved, f_plain_mm, f_saved_mm = alternated(fwd_plain, fwd_saved, reps)
    b_all, b_none, b_all_mm, b_none_mm = alternated(lambda: bwd(all_ptrs), lambda: bwd(None), reps)

    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        bwd(all_ptrs)
        torch.cuda.synchronize()
    fam = {k: [] for k in ("crf_softmax_backward_kernel", "crf_term_backward_kernel", "crf_slice_add_kernel", "crf_grad_image_kernel",
                           "crf_grad_final_kernel", "crf_splat_kernel", "crf_blur4x2_kernel", "crf_blur4_kernel", "crf_planes_rows")}
    for ev in prof.events():
        if "DeviceType.CUDA" not in str(getattr(ev, "device_type", "")):
            continue
        us = getattr(ev, "device_time", None)
        if us is None:
            us = getattr(ev, "cuda_time", 0.0)
        for name in fam:
            if name in ev.name:
                fam[name].append(float(us))
                break
    kernels = {k: dict(launches=len(v), ms=float(np.sum(v)) / 1e3) for k, v in fam.items() if v}
    rec = dict(images=B, size=[H, W], labels=K, iters=iters, reps=reps,
               forward_ms=f_plain, forward_saved_ms=f_saved, forward_min_max_ms=f_plain_mm, forward_saved_min_max_ms=f_saved_mm,
               backward_all_compat_ms=b_all, backward_unary_only_ms=b_none, backward_all_compat_min_max_ms=b_all_mm,
               backward_unary_only_min_max_ms=b_none_mm, backward_per_forward=b_all / f_plain, backward_unary_only_per_forward=b_none / f_plain,
               reserve_grad_bytes=reserved, allocated_bytes_before=before, history_bytes=history.numel() * 4,
               forward_saved_bit_identical=same, backward_deterministic=deterministic, unary_gradient_same_without_compat=unary_same,
               backward_kernels=kernels,
               note="forward = pnp_crf_infer_terms with the marginals out and no labels, forward_saved = pnp_crf_infer_terms_saved (the "
                    "same launches plus iters + 1 device copies of the marginal rows), alternated repetition by repetition, medians of "
                    "device events; backward_all_compat = pnp_crf_backward_terms with the gradient of every compatibility (two scalars "
                    "and one K x K matrix: one forward filter per term and update on top), backward_unary_only = with none; "
                    "backward_kernels = device time of one backward_all_compat call by kernel family as torch's profiler reports it "
                    "(crf_blur4x2 / crf_splat also serve the recomputed forward filters).  Random unaries, cotangent and matrix: the "
                    "arithmetic does not depend on the values")
    feat.close()
    return rec


def grad_errors(crf):
    """--grad_errors: max|g - g_ref| / max|g_ref| of every gradient tensor of the GPU test's cases (tests/_crf_grad_ref.GRAD_CASES,
    measured by tests/test_crf_grad_gpu.measure) -- the figures the test's bound (_crf_grad_ref.WORST_MEASURED, BOUND) is set from."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _crf_grad_ref as R
    import _crf_terms_ref as TR
    import test_crf_grad_gpu as G
    pix = sorted(c[0][1] * c[0][2] for c in TR.CASES)
    solver = crf.FeatureCRF(2, pix[-1] + pix[-2], pix[-1], 150, max_terms=4, max_dims=6)
    cases = {name: G.measure(crf, solver, i, k) for (i, k), name in zip(R.GRAD_CASES, G.CASE_IDS)}
    solver.close()
    worst = max(v for d in cases.values() for v in d.values())
    return dict(what="max|g - g_ref| / max|g_ref| per gradient tensor against the float64 reference of tests/_crf_grad_ref.py, "
                     f"{R.ITERS} iterations (tools/crf_bench.py --grad_errors)",
                cases=cases, worst=worst, bound=float(10.0 ** np.ceil(np.log10(10 * worst) - 1e-9)))


def main():
    import torch
    from oracle import pipeline_np as OP
    from pnp_ovss import config as C, crf
    from pnp_ovss.hip import Engine
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=35)
    ap.add_argument("--size", default="375x500")
    ap.add_argument("--labels", type=int, default=21)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--oracle_reps", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crf_standalone.json"))
    ap.add_argument("--compat", choices=["matrix"], default=None,
                    help="matrix: measure only the compatibility-matrix update next to the Potts one and merge the result into "
                         "the record at --out as `compat_matrix` (the other fields stay as the last full run wrote them)")
    ap.add_argument("--terms", action="store_true",
                    help="measure only the feature-terms solver (crf.FeatureCRF) next to DenseCRF.run and write the record to "
                         "profiles/crf_terms.json (or --terms_out)")
    ap.add_argument("--terms_out", default=os.path.join(ROOT, "profiles", "crf_terms.json"))
    ap.add_argument("--grad", action="store_true",
                    help="measure only the backward pass of the feature-term mean-field and write the record to profiles/crf_grad.json "
                         "(or --grad_out), keeping the `errors` entry of the record that is there")
    ap.add_argument("--grad_out", default=os.path.join(ROOT, "profiles", "crf_grad.json"))
    ap.add_argument("--grad_errors", action="store_true",
                    help="measure only the gradients' errors against the float64 reference and write them as the `errors` entry of "
                         "the record at --grad_out, keeping its other fields")
    a = ap.parse_args()
    if a.grad or a.grad_errors:
        old = {}
        if a.grad_out and os.path.exists(a.grad_out):
            with open(a.grad_out) as f:
                old = json.loads(f.read())
        if a.grad:
            rec = grad_bench(torch, crf, a)
            if "errors" in old:
                rec["errors"] = old["errors"]
        else:
            rec = dict(old, errors=grad_errors(crf))
        line = json.dumps(rec)
        print(line)
        if a.grad_out:
            with open(a.grad_out, "w") as f:
                f.write(line + "\n")
        return
    if a.terms:
        line = json.dumps(terms_bench(torch, crf, a))
        print(line)
        if a.terms_out:
            with open(a.terms_out, "w") as f:
                f.write(line + "\n")
        return
    if a.compat == "matrix":
        rec = {}
        if a.out and os.path.exists(a.out):
            with open(a.out) as f:
                rec = json.loads(f.read())
        rec["compat_matrix"] = compat_matrix(torch, crf, a)
        line = json.dumps(rec)
        print(json.dumps(rec["compat_matrix"]))
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return
    H, W = map(int, a.size.split("x"))
    B, K, IMG = a.images, a.labels, 336
    rng = np.random.default_rng(0)
    imgs = [synth_photo(rng, H, W) for _ in range(B)]
    d_rgb = torch.from_numpy(np.concatenate([im.reshape(-1) for im in imgs])).cuda()
    sizes = [(H, W)] * B

    # ---- the engine's CRF stage on maps of its own making
    e = Engine(C.blip_itm_small(IMG), max_batch=B, max_text_len=max(32, K + 8), stash_layer=7, bf16=True)
    e.post_reserve(B, B * H * W, H * W, K, 0)
    grid = IMG // 16
    cam = rng.random((B, K + 3, grid, grid), dtype=np.float32) ** 4
    cam[:, :, :, 2 * grid // 3:] = 0                    # a third of every image belongs to no class: the background channel is
    d_cam = torch.from_numpy(cam).cuda()                 # neither empty nor full, and min-max leaves no 0 / 0 = NaN channel
    e.post_prepare(sizes, [[([i], 1) for i in range(K - 1)]] * B, [list(range(K))] * B, [True] * B, rgb=d_rgb, gt=None, want_crf=True)
    e.merge_tokens(d_cam)
    e.threshold_upsample(0.15, False)
    e.blur_minmax()
    maps = [m.clone() for m in e.post_maps("maps")]
    if any(bool(torch.isnan(m).any()) for m in maps):
        raise SystemExit("the engine's maps hold NaN: the timings would be those of NaN arithmetic")
    e.densecrf()                                                                  # warm
    # the engine's own unary rows (pixel-major, Kp floats) as (K, H*W) planes: the stand-alone runs start from the same bits
    rows, kp = e.buffer("unary"), (K + 3) // 4 * 4
    d_unary = torch.cat([rows[b * kp * H * W:(b + 1) * kp * H * W].view(H * W, kp)[:, :K].t().contiguous().reshape(-1) for b in range(B)])
    torch.cuda.synchronize()
    e.profile_enable(True)
    for _ in range(a.reps):
        e.densecrf()
    n_eng, _, ms_eng = e.profile_read_stage(1)
    e.profile_enable(False)
    eng_call_ms = events_ms(torch, e.densecrf, a.reps)                            # unary stage + mean-field
    q_eng = [q.clone() for q in e.post_q()]
    lab_eng = e.split_labels(e.remap_hist(True))
    e.close()

    # ---- the same problem through the stand-alone solver
    solver = crf.DenseCRF(B, B * H * W, H * W, K)

    def set_all():
        solver.set_batch(d_unary, d_rgb, sizes, [K] * B)
    set_all()
    lab, q = solver.infer()                                                       # warm
    # same unary bits, same kernels, same order: the marginals and labels of the two paths must be identical
    q_err = max(float((q[b].reshape(K, -1).t() - q_eng[b]).abs().max()) for b in range(B))
    lab_diff = sum(int((lab[b] != lab_eng[b]).sum()) for b in range(B))
    batch_set_ms = events_ms(torch, set_all, a.reps)
    batch_infer_ms = events_ms(torch, lambda: solver.infer(want_q=True), a.reps)
    batch_infer_labels_ms = events_ms(torch, lambda: solver.infer(want_q=False), a.reps)
    batch_meanfield_ms = events_ms(torch, lambda: solver.infer(want_q=False, want_labels=False), a.reps)
    U0 = d_unary[:K * H * W].reshape(K, H * W).cpu().numpy()
    t0 = time.perf_counter()
    for _ in range(a.reps):
        solver.run([U0.reshape(K, H, W)] * B, imgs)[0][0].cpu()
    batch_run_wall_ms = (time.perf_counter() - t0) / a.reps * 1e3
    bytes_batch = solver.allocated_bytes()
    solver.close()

    # ---- one image: through the shim (host to host), and the two device phases by events
    sys.path.insert(0, os.path.join(ROOT, "pnp-ovss_amd", "shims"))
    import pydensecrf.densecrf as dcrf
    assert sys.modules["pydensecrf"].__pnp_ovss_shim__

    def shim_call():
        d = dcrf.DenseCRF2D(W, H, K)
        d.setUnaryEnergy(U0)
        d.addPairwiseGaussian(sxy=3, compat=7)
        d.addPairwiseBilateral(sxy=50, srgb=5, rgbim=imgs[0], compat=10)
        Q = np.array(d.inference(10)).reshape((K, H, W))
        return np.argmax(Q, axis=0)
    shim_call()                                                                   # warm (creates the module's solver)
    t0 = time.perf_counter()
    for _ in range(a.reps):
        shim_call()
    shim_wall_ms = (time.perf_counter() - t0) / a.reps * 1e3
    one = crf.DenseCRF(1, H * W, H * W, K)
    d_u0, d_rgb0 = d_unary[:K * H * W], d_rgb[:3 * H * W]
    one.set_batch(d_u0, d_rgb0, [(H, W)], [K])
    one.infer()
    one_set_ms = events_ms(torch, lambda: one.set_batch(d_u0, d_rgb0, [(H, W)], [K]), a.reps)
    one_infer_ms = events_ms(torch, lambda: one.infer(want_q=True), a.reps)
    one.close()

    # ---- the oracle on one host core, same single image
    zeros = np.zeros((K, H, W), np.float32)
    t0 = time.perf_counter()
    for _ in range(a.oracle_reps):
        OP.densecrf_variant(imgs[0], zeros, variant=0, unary=U0.reshape(K, H, W))
    oracle_ms = (time.perf_counter() - t0) / a.oracle_reps * 1e3

    rec = dict(images=B, size=[H, W], labels=K, iters=10, reps=a.reps,
               one_image=dict(shim_host_to_host_ms=shim_wall_ms, set_batch_events_ms=one_set_ms, infer_events_ms=one_infer_ms),
               batch=dict(run_wall_ms=batch_run_wall_ms, set_batch_events_ms=batch_set_ms, infer_events_ms=batch_infer_ms,
                          infer_labels_only_events_ms=batch_infer_labels_ms, meanfield_only_events_ms=batch_meanfield_ms,
                          allocated_bytes=bytes_batch),
               engine=dict(meanfield_stage_ms=ms_eng / max(n_eng, 1), densecrf_call_events_ms=eng_call_ms, runs=int(n_eng)),
               oracle_one_core_one_image_ms=oracle_ms,
               agreement=dict(max_abs_q_standalone_vs_engine=q_err, labels_differing=lab_diff, pixels=B * H * W,
                              bit_identical=bool(q_err == 0.0 and lab_diff == 0)),
               note="oracle_one_core_one_image_ms is oracle/densecrf_ref.c, the project's own C restatement of the mean-field, on "
                    "one host core: the only stand-in for pydensecrf that runs where pydensecrf cannot be installed; it is NOT "
                    "pydensecrf.  set_batch_events_ms spans the unary ingest and both lattice builds with their read-backs "
                    "(the Gaussian lattice is reused after the first call); infer_events_ms = mean-field + fused labels + "
                    "marginals out; meanfield_only = infer with neither output; engine.meanfield_stage_ms = the engine's stage "
                    "profile around the same iteration kernels; run_wall_ms = DenseCRF.run from numpy inputs to the first "
                    "label map on the host")
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
