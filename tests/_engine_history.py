"""Case tables and helpers of tests/test_engine_history_gpu.py: what an engine call may carry over from earlier calls.

An engine's activation workspace is laid out by the shapes of the CURRENT call (text rows at b * L, token rows at b * N, the
probabilities as [B, heads, L, Nst]), so after a larger call everything behind the current call's rows holds the previous call's
numbers.  Every case here is a `before` sequence of calls and a `probe` call on one engine; the probe's outputs must equal, bit
for bit, those of the same probe on an engine that has run nothing else.

Geometry: blip_itm_small(128) -- 8 x 8 patches, N = 65 image tokens, Npad = 128: the second 64-key tile holds ONE valid key and 63
pad keys, the smallest shape at which every attention variant has a tile tail.  Two text capacities: 32, and 208 for the captions
above TXT_MAX_L = 192 (csrc/text_kernels.hip), where the self-attention forward / backward switch to their _long kernels and to
global scratch.

Importable without torch or a GPU (tests/test_engine_history_cpu.py proves the tables are what they claim); run_call() is the only
function that touches the device."""
from collections import namedtuple

import numpy as np

from pnp_ovss import config as C, synth

CFG = C.blip_itm_small(128)
WEIGHT_SEED = 3
HEAD, STASH_LAYER, MAX_BATCH = 9, 7, 4             # as the small goldens
CAP_SHORT, CAP_LONG = 32, 208                      # max_text_len of the two engine capacities
TXT_MAX_L = 192                                    # csrc/text_kernels.hip: captions above it take the _long self-attention kernels
LD_EXTRA = 8                                       # ids / mask rows are max_text_len + LD_EXTRA wide: every L is shorter than ld
MODES = (("f32", 1), ("bf16", 1), ("bf16x3", 1), ("bf16x3", 2))       # (compute mode, pnp_set_tuning("streamk"))

# One engine call.  kind: "gradcam" | "drop_loop" | "text" | "project"
#   lens: caption length per row (its max is the call's L, its count the call's B / T); seed: images and captions
#   layer: compute_gradcam(layer=) | dropped_seed: an explicit `dropped` mask | drop_iter: drop_loop
#   which / rows: project_normalize of `rows` seeded rows with vision_proj (0) / text_proj (1)
Call = namedtuple("Call", "kind lens seed layer dropped_seed drop_iter which rows", defaults=(None,) * 5)
Case = namedtuple("Case", "name cap before probe same_shape")

PROBE_SEED = 21                                    # every probe's images and captions; the before calls use 31, 41, ...


def gradcam(lens, seed, layer=None, dropped_seed=None):
    return Call("gradcam", tuple(lens), seed, layer, dropped_seed)


def drop_loop(lens, seed, drop_iter):
    return Call("drop_loop", tuple(lens), seed, None, None, drop_iter)


def text(lens, seed):
    return Call("text", tuple(lens), seed)


def project(which, rows, seed):
    return Call("project", (), seed, None, None, None, which, rows)


def _full(B, L):
    return (L,) * B


RAGGED = (5, 11, 25)
P_B1_L12 = gradcam(_full(1, 12), PROBE_SEED)
P_B3_L12 = gradcam(_full(3, 12), PROBE_SEED)
P_B2_L12 = gradcam(_full(2, 12), PROBE_SEED)
P_B3_L7 = gradcam(_full(3, 7), PROBE_SEED)
P_B3_L25 = gradcam(_full(3, 25), PROBE_SEED)
P_B2_L25 = gradcam(_full(2, 25), PROBE_SEED)
P_RAGGED = gradcam(RAGGED, PROBE_SEED)
P_LOOP4 = drop_loop(_full(2, 12), PROBE_SEED, 4)
P_LOOP1 = drop_loop(_full(2, 12), PROBE_SEED, 1)
P_TEXT = text((6, 5, 6), PROBE_SEED)
LONG_L = 200

CASES = (
    # 1. B shrinks: at B = 3 the last image's tile tails and the GEMM M-tail land on image 3's stale rows
    Case("b4_then_b1", CAP_SHORT, (gradcam(_full(4, 12), 31),), P_B1_L12, False),
    Case("b4_then_b3", CAP_SHORT, (gradcam(_full(4, 12), 31),), P_B3_L12, False),
    # 2. L shrinks / grows; the long kernels' dS / scratch and 200-row Ps / Pc blocks behind a short-kernel call
    Case("l25_then_l7", CAP_SHORT, (gradcam(_full(3, 25), 31),), P_B3_L7, False),
    Case("l7_then_l25", CAP_SHORT, (gradcam(_full(3, 7), 31),), P_B3_L25, False),
    Case("l200_then_l25", CAP_LONG, (gradcam(_full(2, LONG_L), 31),), P_B2_L25, False),
    # 3. ragged masks behind a full-length mask of the same L
    Case("full_then_ragged", CAP_SHORT, (gradcam(_full(3, 25), 31),), P_RAGGED, True),
    # 4. other entry points in between: text-only (a chunk of 4 and a remainder of 2), both projections, another target layer
    Case("other_entry_points", CAP_SHORT,
         (gradcam(_full(4, 12), 31), text((9, 5, 7, 9, 6, 8), 41), project(0, 260, 51), project(1, 50, 52),
          gradcam(_full(4, 12), 61, layer=9)), P_B2_L12, False),
    # 5. the drop loop's x0 copy and in-place `dropped` mask
    Case("loop_then_gradcam", CAP_SHORT, (drop_loop(_full(4, 12), 31, 4),), P_B2_L12, False),
    Case("loop_then_loop4", CAP_SHORT, (drop_loop(_full(4, 12), 31, 4),), P_LOOP4, False),
    Case("loop_then_loop1", CAP_SHORT, (drop_loop(_full(4, 12), 31, 4),), P_LOOP1, False),
    Case("dropped_then_none", CAP_SHORT, (gradcam(_full(3, 12), 31, dropped_seed=71),), P_B3_L12, True),
    # 6. a text-only probe behind a multimodal pass
    Case("gradcam_then_text", CAP_SHORT, (gradcam(_full(4, 25), 31),), P_TEXT, False),
)


def probes():
    """The distinct (capacity, probe) pairs of CASES, in table order."""
    seen = []
    for c in CASES:
        if (c.cap, c.probe) not in seen:
            seen.append((c.cap, c.probe))
    return seen


def call_id(call):
    if call.kind == "project":
        return f"project{call.which}x{call.rows}"
    s = f"{call.kind}-B{len(call.lens)}-L{max(call.lens)}"
    if len(set(call.lens)) > 1:
        s += "r"
    if call.drop_iter:
        s += f"-d{call.drop_iter}"
    if call.layer is not None:
        s += f"-layer{call.layer}"
    if call.dropped_seed is not None:
        s += "-dropped"
    return s


def shape_of(call):
    """(B or T, L) of a call with captions."""
    return len(call.lens), max(call.lens)


def inputs(call, cap):
    """The host arrays of a call on an engine of text capacity `cap`, every one a function of the call alone."""
    if call.kind == "project":
        K = CFG.vit_dim if call.which == 0 else CFG.txt_hidden
        return {"x": np.random.default_rng([call.seed, 13]).standard_normal((call.rows, K)).astype(np.float32)}
    B, L = shape_of(call)
    ids, mask = synth.synth_tokens(CFG, [n - 5 for n in call.lens], seed=call.seed + 1, max_length=cap + LD_EXTRA)
    out = {"ids": ids, "mask": mask, "L": L}
    if call.kind != "text":
        out["imgs"] = synth.synth_images(B, CFG.img_size, seed=call.seed)[1]
    if call.dropped_seed is not None:
        g = np.random.default_rng([call.dropped_seed, 17])
        d = np.zeros((B, CFG.grid * CFG.grid), dtype=np.uint8)
        for b in range(B):
            d[b, g.choice(d.shape[1], 10, replace=False)] = 1
        out["dropped"] = d
    return out


def state_dict():
    """synth_state_dict plus the ITC projections, so project_normalize runs in every mode."""
    sd = dict(synth.synth_state_dict(CFG, WEIGHT_SEED))
    sd.update(synth.itc_state_dict(CFG, WEIGHT_SEED))
    return sd


def run_call(e, call, cap):
    """Run one call on engine `e`; returns everything its entry point returns, as a tuple of device tensors.
    gradcam: (maps, logits) | drop_loop: (g0, agg, picks, logits), agg left out at drop_iter 1 | text: (hidden, text_proj of the
    [CLS] rows where the projection is loaded) | project: (rows,)."""
    import torch
    a = {k: (torch.from_numpy(v).cuda() if isinstance(v, np.ndarray) else v) for k, v in inputs(call, cap).items()}
    if call.kind == "gradcam":
        out = e.compute_gradcam(a["imgs"], a["ids"], a["mask"], a["L"], HEAD, dropped=a.get("dropped"), layer=call.layer)
    elif call.kind == "drop_loop":
        out = e.drop_loop(a["imgs"], a["ids"], a["mask"], a["L"], HEAD, call.drop_iter)
    elif call.kind == "text":
        hid = e.text_forward_text(a["ids"], a["mask"], a["L"])
        out = (hid,)
        if not e.missing_proj((1,)):
            out += (e.project_normalize(1, hid, row_stride=a["L"] * CFG.txt_hidden, rows=hid.shape[0]),)
    elif call.kind == "project":
        out = (e.project_normalize(call.which, a["x"]),)
    else:
        raise ValueError(call.kind)
    torch.cuda.synchronize()
    return tuple(t for t in out if t is not None)


def norm01(m):
    """The pipeline's per-token min-max normalisation of the maps (the criterion of test_gradcam_small_vs_reference_golden)."""
    m = m.astype(np.float64)
    lo = m.min(axis=(-1, -2), keepdims=True)
    hi = m.max(axis=(-1, -2), keepdims=True)
    return (m - lo) / np.maximum(hi - lo, 1e-30)
