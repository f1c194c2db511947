"""GPU: BlipITM.forward(match_head="itc") and BlipITM.extract_features on the HIP engine against the reference's own CPU run
(tests/golden/itc_small.npz, itc_large.npz; generator tests/golden/make_itc_golden.py), the three new device pieces as
operators, and what the text-only pass must leave alone.
Run on the MI355X box:  python -m pytest tests/test_itc_gpu.py -m gpu -q -s

Bounds.  Cosine similarities and normalised features are at most 1 in size, so max-abs is the norm that means something.
Ceilings (from the neighbouring tests, set before anything was measured): 1e-4 max-abs on `sim` and on every `*_proj` output in
"f32" and "bf16x3" (north_star's float bound; test_gradcam_small_vs_reference_golden); on the un-normalised embeddings the
bounds of test_vit_forward_small -- "f32" 2e-4 max-abs, "bf16x3" 1e-3 max-abs and 2e-5 mean-abs.  Every comparison prints its
measured error (pytest -s; appended to $PNP_TEST_MEASURE_LOG when set); where ~2x the value measured on MI355X is tighter than
the ceiling, that is the bound, with the measured values beside it (PROJ / EMBED / PROJ_OP below).  "bf16" is not a parity mode anywhere in this project: its
outputs must be finite and within 5e-2 (bf16 storage: ~1 % error on O(1) image_embeds, include/pnp_hip.h, against outputs
bounded by 1).
"""
import json
import os
import warnings

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from pnp_ovss import config as C, synth            # noqa: E402

pytestmark = pytest.mark.gpu

FIELDS = ("image_embeds", "image_embeds_proj", "text_embeds", "text_embeds_proj", "multimodal_embeds")
_MODEL = {}


def _golden(name):
    here = os.path.dirname(os.path.abspath(__file__))
    return np.load(os.path.join(here, "golden", name), allow_pickle=False)


def _cfg(g):
    return C.ModelCfg(**json.loads(str(g["cfg"])))


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def _model(cfg, seed, mode, max_batch=4, max_text_len=32):
    """An eager model with seeded weights, ITC projections included; one alive at a time (device memory)."""
    from pnp_ovss.model import build_model
    key = (cfg, seed, mode, max_batch, max_text_len)
    if key not in _MODEL:
        for m in _MODEL.values():
            m.engine.close()
        _MODEL.clear()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")               # "no BLIP checkpoint given": the seeded weights are the point
            _MODEL[key] = build_model(cfg=cfg, max_batch=max_batch, max_text_len=max_text_len, stash_layer=7, mode=mode, seed=seed)
    return _MODEL[key]


def _err(tag, got, ref, reduce="max"):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    d = np.abs(got - ref)
    v = float(d.max() if reduce == "max" else d.mean())
    print(f"[itc error] {tag} ({reduce}): {v:.3e}")
    log = os.environ.get("PNP_TEST_MEASURE_LOG")
    if log:
        with open(log, "a") as f:
            f.write(json.dumps({"tag": tag, "value": v, "reduce": reduce}) + "\n")
    return v


# Bounds = ~2x the worst value measured on MI355X over the small and the BLIP-large fixtures, all below the ceilings of the module
# docstring (1e-4 | 2e-4 | 1e-3 max-abs, 2e-5 mean-abs):
#   sim / *_proj      f32    measured 6.5e-7 (sim small) 9.3e-7 (sim large) 2.8e-7 .. 2.4e-6 (features; worst: large image tokens)
#                     bf16x3 measured 1.2e-6 (sim small) 3.9e-6 (sim large) 2.4e-6 .. 5.4e-6 (features; worst: large image tokens)
#   embeddings max    f32    measured 6.9e-6 image (small) 5.0e-5 image (large) 4.1e-5 / 4.0e-5 text 5.0e-5 / 6.5e-5 multimodal
#                     bf16x3 measured 2.0e-5 image (small) 1.1e-4 image (large) 7.1e-5 / 6.8e-5 text 7.2e-5 / 1.0e-4 multimodal
#   embeddings mean   bf16x3 measured 1.1e-6 .. 1.5e-5 (worst: large image / multimodal): 2x that is above the 2e-5 ceiling, which stays
PROJ = {"f32": 5e-6, "bf16x3": 1.2e-5}
EMBED = {"f32": (1.3e-4, None), "bf16x3": (2.3e-4, 2e-5)}
# the operators alone, against float64 (no encoder in front): measured f32 3.0e-7, bf16x3 1.7e-6
PROJ_OP = {"f32": 6e-7, "bf16x3": 3.5e-6}


def _check_embed(tag, mode, got, ref):
    mx, mean = EMBED[mode]
    assert _err(tag, got, ref) < mx
    if mean is not None:
        assert _err(tag, got, ref, "mean") < mean


def _samples(g, cfg):
    caps = [str(c) for c in g["captions"]]
    _, imgs = synth.synth_images(len(caps), cfg.img_size, seed=int(g["image_seed"]))
    return {"image": torch.from_numpy(imgs), "text_input": caps}


# ------------------------------------------------------------------------------------------ 1 / 2: small geometry
@pytest.mark.parametrize("mode", ["f32", "bf16x3", "bf16"])
def test_forward_itc_small_vs_reference_golden(mode):
    """forward(match_head="itc") against the reference's sim (3, 3); one caption is a single word (an L = 3 row)."""
    g = _golden("itc_small.npz")
    cfg = _cfg(g)
    m = _model(cfg, int(g["weight_seed"]), mode)
    sim = m(_samples(g, cfg), match_head="itc")
    torch.cuda.synchronize()
    assert sim.is_cuda and tuple(sim.shape) == (3, 3) and sim.dtype == torch.float32
    got = sim.cpu().numpy()
    assert np.isfinite(got).all()
    e = _err(f"forward_itc_small[{mode}] sim", got, g["sim"])
    assert e < (5e-2 if mode == "bf16" else PROJ[mode])          # bf16: measured 5.6e-4; the loose bound of the docstring stays
    with pytest.raises(ValueError):
        m(_samples(g, cfg), match_head="itx")


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
@pytest.mark.parametrize("feat", ["image", "text", "multimodal"])
def test_extract_features_small_vs_reference_golden(feat, mode):
    from pnp_ovss.model import BlipOutputFeatures
    from lavis.models.blip_models.blip_image_text_matching import BlipOutputFeatures as shim_cls
    assert shim_cls is BlipOutputFeatures
    g = _golden("itc_small.npz")
    cfg = _cfg(g)
    m = _model(cfg, int(g["weight_seed"]), mode)
    out = m.extract_features(_samples(g, cfg), mode=feat)
    torch.cuda.synchronize()
    assert isinstance(out, BlipOutputFeatures)
    none = set(str(k) for k in g["none_fields"])
    for f in FIELDS:
        v = getattr(out, f)
        key = f"{feat}__{f}"
        if key in none:
            assert v is None, key
            continue
        assert v is not None and v.is_cuda and tuple(v.shape) == g[key].shape, key
        got = v.cpu().numpy()
        if f.endswith("_proj"):
            assert _err(f"extract_features_small[{feat},{mode}] {f}", got, g[key]) < PROJ[mode]
            assert np.abs(np.linalg.norm(got.astype(np.float64), axis=-1) - 1.0).max() < 1e-6
        else:
            _check_embed(f"extract_features_small[{feat},{mode}] {f}", mode, got, g[key])
    with pytest.raises(ValueError):
        m.extract_features(_samples(g, cfg), mode="audio")


# ------------------------------------------------------------------------------------------ 3: BLIP-ITM-large 336^2
@pytest.mark.parametrize("mode", [pytest.param("f32", marks=pytest.mark.slow), "bf16x3"])
def test_itc_and_features_large_vs_reference_golden(mode):
    g = _golden("itc_large.npz")
    cfg = _cfg(g)
    m = _model(cfg, int(g["weight_seed"]), mode, max_batch=2, max_text_len=16)
    s = _samples(g, cfg)
    sim = m(s, match_head="itc")
    torch.cuda.synchronize()
    assert _err(f"itc_large[{mode}] sim", sim.cpu().numpy(), g["sim"]) < PROJ[mode]
    none = set(str(k) for k in g["none_fields"])
    for feat in ("image", "text", "multimodal"):
        out = m.extract_features(s, mode=feat)
        torch.cuda.synchronize()
        for f in FIELDS:
            v = getattr(out, f)
            if f"{feat}__{f}" in none:
                assert v is None
                continue
            got, ref = v.cpu().numpy(), g[f"{feat}__{f}__first8"]
            if f.endswith("_proj"):
                assert np.abs(np.linalg.norm(got.astype(np.float64), axis=-1) - 1.0).max() < 1e-6
                assert _err(f"itc_large[{feat},{mode}] {f}", got[:, :8], ref) < PROJ[mode]
                cls = g["image_cls_proj"] if f == "image_embeds_proj" else g["text_cls_proj"]
                assert _err(f"itc_large[{feat},{mode}] {f} cls", got[:, 0], cls) < PROJ[mode]
            else:
                _check_embed(f"itc_large[{feat},{mode}] {f}", mode, got[:, :8], ref)


# ------------------------------------------------------------------------------------------ 4: operators
def _op_engine(mode, max_batch=35, max_text_len=16, seed=3):
    from pnp_ovss.hip import Engine
    cfg = C.blip_itm_small(64)
    for m in _MODEL.values():
        m.engine.close()
    _MODEL.clear()
    e = Engine(cfg, max_batch=max_batch, max_text_len=max_text_len, stash_layer=7, mode=mode)
    sd = dict(synth.synth_state_dict(cfg, seed))
    itc = synth.itc_state_dict(cfg, seed)
    sd.update(itc)
    e.load_state_dict(sd)
    return cfg, e, itc


def _ref_project(x, w, b):
    y = x.astype(np.float64) @ w.astype(np.float64).T + b.astype(np.float64)
    return y / np.maximum(np.linalg.norm(y, axis=-1, keepdims=True), 1e-12)


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_project_normalize_operator(mode):
    """pnp_project_normalize against float64 numpy: random rows of both widths, an all-zero input row with a zero bias (the eps
    clamp: zeros, not NaN), more rows than one tile, and the strided CLS rows of a (B, N, D) tensor without a gather."""
    cfg, e, itc = _op_engine(mode)
    rng = np.random.default_rng(11)
    try:
        for which, K in ((0, cfg.vit_dim), (1, cfg.txt_hidden)):
            pre = "vision_proj" if which == 0 else "text_proj"
            w, b = itc[pre + ".weight"], itc[pre + ".bias"]
            x = rng.standard_normal((333, K)).astype(np.float32)
            got = e.project_normalize(which, _dev(x))
            torch.cuda.synchronize()
            assert tuple(got.shape) == (333, 256)
            assert _err(f"project_normalize[{mode}] which={which}", got.cpu().numpy(), _ref_project(x, w, b)) < PROJ_OP[mode]
            # strided rows: the CLS rows of (B, N, K)
            B, N = 5, 17
            x3 = rng.standard_normal((B, N, K)).astype(np.float32)
            got = e.project_normalize(which, _dev(x3), row_stride=N * K, rows=B)
            torch.cuda.synchronize()
            assert tuple(got.shape) == (B, 256)
            assert _err(f"project_normalize[{mode}] which={which} strided", got.cpu().numpy(), _ref_project(x3[:, 0], w, b)) < PROJ_OP[mode]
        # the eps clamp: y = W . 0 + 0 = 0 -> 0 / max(0, 1e-12) = 0
        from pnp_ovss.hip import Engine
        e2 = Engine(cfg, max_batch=2, max_text_len=16, stash_layer=7, mode=mode)
        sd = dict(synth.synth_state_dict(cfg, 3))
        sd.update(itc)
        sd["vision_proj.bias"] = np.zeros(256, np.float32)
        e2.load_state_dict(sd)
        x = rng.standard_normal((6, cfg.vit_dim)).astype(np.float32)
        x[2] = 0.0
        got = e2.project_normalize(0, _dev(x)).cpu().numpy()
        e2.close()
        assert np.isfinite(got).all() and (got[2] == 0).all()
        ref = _ref_project(x, itc["vision_proj.weight"], np.zeros(256))
        assert _err(f"project_normalize[{mode}] zero row", got, ref) < PROJ_OP[mode]
    finally:
        e.close()


def test_itc_similarity_operator():
    """pnp_itc_similarity against float64 for B = 35 images x T = 150 texts of unit-norm 256-wide features: four fp32 FMA chains
    of 64 terms whose sum is at most 1 in size -> below 2e-6 (16 x 2^-23) by construction; measured 5.7e-8, bound ~2x that."""
    from pnp_ovss import hip
    lib = hip.load_library()
    rng = np.random.default_rng(2)
    a = rng.standard_normal((35, 256))
    t = rng.standard_normal((150, 256))
    a = (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)
    t = (t / np.linalg.norm(t, axis=1, keepdims=True)).astype(np.float32)
    da, dt = _dev(a), _dev(t)
    sim = torch.empty(35, 150, device="cuda")
    assert lib.pnp_itc_similarity(da.data_ptr(), dt.data_ptr(), 35, 150, 256, sim.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert _err("itc_similarity 35x150", sim.cpu().numpy(), a.astype(np.float64) @ t.astype(np.float64).T) < 1.2e-7


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_text_only_pass_chunking_is_bit_identical(mode):
    """T = 150 texts on an engine with max_batch = 35 (five pieces inside the call) equal the same texts run in separate calls
    of 30, bit for bit; and a text's hidden states do not depend on its neighbours."""
    cfg, e, _ = _op_engine(mode, max_batch=35)
    try:
        rng = np.random.default_rng(5)
        T, L = 150, 9
        ids = rng.integers(110, cfg.vocab - 2, size=(T, L)).astype(np.int64)
        ids[:, 0] = 101
        lens = rng.integers(3, L + 1, size=T)
        lens[:3] = (3, L, 4)
        mask = (np.arange(L)[None, :] < lens[:, None]).astype(np.int64)
        for r in range(T):
            ids[r, lens[r] - 1] = cfg.sep_token_id
        ids = ids * mask
        d_ids, d_mask = _dev(ids), _dev(mask)
        whole = e.text_forward_text(d_ids, d_mask, L)
        torch.cuda.synchronize()
        assert tuple(whole.shape) == (T, L, cfg.txt_hidden) and torch.isfinite(whole).all()
        parts = [e.text_forward_text(d_ids[o:o + 30].contiguous(), d_mask[o:o + 30].contiguous(), L) for o in range(0, T, 30)]
        torch.cuda.synchronize()
        assert torch.equal(whole, torch.cat(parts))
        # "text_hidden" holds the last piece (rows 140..149) of the whole-call run order
        whole2 = e.text_forward_text(d_ids, d_mask, L)
        torch.cuda.synchronize()
        tail = e.buffer("text_hidden")[: 10 * L * cfg.txt_hidden].view(10, L, cfg.txt_hidden)
        assert torch.equal(whole2, whole) and torch.equal(tail, whole[140:])
    finally:
        e.close()


# ------------------------------------------------------------------------------------------ 5: isolation
@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_itc_forward_leaves_gradcam_intact_and_invalidates_the_hooks(mode):
    import argparse
    from lavis.models.blip_models.blip_image_text_matching import compute_gradcam_ensemble
    from pnp_ovss.model import build_model
    g = _golden("itc_small.npz")
    cfg = _cfg(g)
    m = _model(cfg, int(g["weight_seed"]), mode)
    s = _samples(g, cfg)
    caps = ["A picture of cat aeroplane dog", "A picture of bus", "A picture of person tvmonitor sheep boat"]
    tok500 = m.tokenizer(caps, padding="max_length", max_length=500, return_tensors="pt")
    args = argparse.Namespace(img_size=cfg.img_size)

    def gradcam():
        blocks, _, logits = compute_gradcam_ensemble(args, m, s["image"], caps, tok500)
        return blocks[7][9].clone(), blocks[9][3].clone(), logits.cpu().clone()
    a = gradcam()
    cross = m.text_encoder.base_model.base_model.encoder.layer[7].crossattention.self
    assert cross.get_attention_map().shape[0] == 3                  # valid after a multimodal forward
    sim = m(s, match_head="itc")
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="multimodal forward"):
        cross.get_attention_map()
    with pytest.raises(RuntimeError, match="multimodal forward"):
        cross.get_attn_gradients()
    B, L = 3, int(tok500.attention_mask.sum(1).max())
    with pytest.raises(RuntimeError, match="pnp_text_forward_text"):   # the engine itself refuses the backward as well
        m.engine.xattn_grad(B, L)
    b = gradcam()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert cross.get_attention_map().shape[0] == 3
    # an engine pair on one weight copy gives the same similarities, bit for bit
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        twin = build_model(cfg=cfg, max_batch=3, max_text_len=16, stash_layer=7, mode=mode, donor=m)
    assert twin.engine.shares_weights
    sim2 = twin(s, match_head="itc")
    torch.cuda.synchronize()
    assert torch.equal(sim, sim2)
    twin.engine.close()


# ------------------------------------------------------------------------------------------ 6: no projection weights
def test_engine_without_projection_weights_serves_the_old_paths_and_refuses_itc():
    from pnp_ovss.hip import Engine
    from pnp_ovss.model import BlipITM
    from pnp_ovss.tokenizer import SynthTokenizer
    for m in _MODEL.values():
        m.engine.close()
    _MODEL.clear()
    g = _golden("itc_small.npz")
    cfg = _cfg(g)
    e = Engine(cfg, max_batch=3, max_text_len=16, stash_layer=7, mode="f32")
    e.load_state_dict(synth.synth_state_dict(cfg, int(g["weight_seed"])))       # finalizes without the four tensors
    m = BlipITM(cfg, e, SynthTokenizer(cfg.vocab))
    s = _samples(g, cfg)
    logits = m(s)                                                               # the ITM head works as before
    torch.cuda.synchronize()
    assert tuple(logits.shape) == (3, 2) and torch.isfinite(logits).all()
    with pytest.raises(RuntimeError, match="vision_proj.weight"):
        m(s, match_head="itc")
    with pytest.raises(RuntimeError, match="text_proj.weight"):
        m.extract_features(s, mode="text")
    with pytest.raises(RuntimeError, match="vision_proj.weight"):
        m.extract_features(s, mode="image")
    x = torch.zeros(4, cfg.vit_dim, device="cuda")
    with pytest.raises(RuntimeError, match=r"\(-1\).*missing weight vision_proj.weight"):     # PNP_ERR_STATE from the C ABI itself
        e.project_normalize(0, x)
    with pytest.raises(RuntimeError, match=r"\(-1\).*missing weight text_proj.weight"):
        e.project_normalize(1, torch.zeros(4, cfg.txt_hidden, device="cuda"))
    out = m.extract_features(s, mode="multimodal")                              # needs no projection
    assert out.multimodal_embeds is not None and out.image_embeds_proj is None
    # a projection whose second dimension contradicts the model is an error, like every other tensor
    e2 = Engine(cfg, max_batch=1, max_text_len=16, stash_layer=7, mode="f32")
    with pytest.raises(RuntimeError, match="vision_proj.weight"):
        e2.load_state_dict({"vision_proj.weight": np.zeros((256, cfg.vit_dim + 4), np.float32)}, finalize=False)
    e2.close()
    e.close()


# ------------------------------------------------------------------------------------------ 7: no allocation per call
def test_itc_forward_allocates_nothing_after_the_first_call():
    """Ten repeated calls after the first: neither torch's live device bytes nor the engine's allocation grow, and the result
    repeats bit for bit.  Device tensors that earlier tests left in uncollected reference cycles (exception tracebacks) are
    freed whenever Python's collector happens to run, which LOWERS torch.cuda.memory_allocated() in the middle of the loop: the
    collector is run before the baseline is taken, and the condition is "never above the previous reading", call by call."""
    import gc
    g = _golden("itc_small.npz")
    cfg = _cfg(g)
    m = _model(cfg, int(g["weight_seed"]), "bf16x3")
    s = _samples(g, cfg)
    s = {"image": s["image"].cuda(), "text_input": s["text_input"]}
    first = m(s, match_head="itc").clone()
    torch.cuda.synchronize()
    gc.collect()
    prev_t, base_e = torch.cuda.memory_allocated(), m.engine.allocated_bytes()
    for i in range(10):
        sim = m(s, match_head="itc")
        torch.cuda.synchronize()
        assert torch.equal(sim, first)
        del sim
        now_t = torch.cuda.memory_allocated()
        print(f"[itc alloc] call {i}: torch {now_t} (before {prev_t}), engine {m.engine.allocated_bytes()} (before {base_e})")
        assert now_t <= prev_t and m.engine.allocated_bytes() == base_e
        prev_t = now_t
