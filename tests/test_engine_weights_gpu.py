"""GPU: the weight loader's bookkeeping (pnp_load_weight / pnp_finalize_weights) on the core tensors: what it refuses, that a
refusal can be recovered from, and that neither the order nor a repeated load of a tensor changes a bit of the result.
Run on the MI355X box:  python -m pytest tests/test_engine_weights_gpu.py -m gpu -q

Every comparison is bit for bit: the engines differ only in how the same fp32 values reached the device, so the conversion and
every kernel see identical inputs.  The small geometry in "f32" mode, one image, eight tokens: a case is an engine or two.
"""
import re
from collections import OrderedDict

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from pnp_ovss import config as C, synth            # noqa: E402

pytestmark = pytest.mark.gpu

HEAD = 9
SMALL = "visual_encoder.norm.bias"                                       # a direct fp32 destination
GEMM = "text_encoder.encoder.layer.0.intermediate.dense.weight"          # staged until finalize, then converted


def _engine(cfg, **kw):
    from pnp_ovss.hip import Engine
    return Engine(cfg, max_batch=1, max_text_len=8, mode="f32", **kw)


@pytest.fixture(scope="module")
def base():
    """cfg, the state dict, run(engine) -> (gradcam, logits) on one fixed input, an engine loaded in one call and its result."""
    cfg = C.blip_itm_small(64)
    sd = synth.synth_state_dict(cfg, 3)
    _, imgs = synth.synth_images(1, cfg.img_size, seed=5)
    ids, mask = synth.synth_tokens(cfg, [3], seed=1)
    L = int(mask.sum(1).max())
    imgs, ids, mask = (torch.from_numpy(a).cuda() for a in (imgs, ids, mask))

    def run(e):
        out, logits = e.compute_gradcam(imgs, ids, mask, L, HEAD)
        torch.cuda.synchronize()
        return out.cpu().numpy(), logits.cpu().numpy()

    e = _engine(cfg)
    e.load_state_dict(sd)
    ref = run(e)
    assert np.isfinite(ref[0]).all() and np.abs(ref[0]).max() > 0
    yield cfg, sd, run, e, ref
    e.close()


def _same(got, ref):
    for a, b in zip(got, ref):
        np.testing.assert_array_equal(a, b)


def _missing_names(cfg):
    return ["visual_encoder.pos_embed",
            "visual_encoder.blocks.0.mlp.fc1.weight",
            "text_encoder.encoder.layer.0.attention.self.value.bias",                       # an offset into the fused q|k|v bias
            f"text_encoder.encoder.layer.{cfg.txt_layers - 1}.crossattention.self.key.bias"]  # ... into the layer-major array


@pytest.mark.parametrize("which", range(4))
def test_missing_tensor_is_refused_and_recovered(base, which):
    """Finalize without one tensor names it; loading that tensor and finalizing again gives the bits of an engine loaded in one
    call (a bias written at a wrong offset of its fused / layer-major array would not)."""
    cfg, sd, run, _, ref = base
    name = _missing_names(cfg)[which]
    e = _engine(cfg)
    try:
        with pytest.raises(RuntimeError, match=r"\(-1\).*missing weight " + re.escape(name)):
            e.load_state_dict(OrderedDict((n, w) for n, w in sd.items() if n != name))
        e.load_state_dict({name: sd[name]})
        _same(run(e), ref)
    finally:
        e.close()


def test_reversed_load_order(base):
    cfg, sd, run, _, ref = base
    e = _engine(cfg)
    try:
        e.load_state_dict(OrderedDict(reversed(list(sd.items()))))
        _same(run(e), ref)
    finally:
        e.close()


@pytest.mark.parametrize("name", [SMALL, GEMM])
def test_double_load_keeps_the_second_value(base, name):
    cfg, sd, run, _, ref = base
    other = synth.synth_tensor(name, sd[name].shape, 4)
    assert (other != sd[name]).any()
    twice, once = _engine(cfg), _engine(cfg)
    try:
        twice.load_state_dict(sd, finalize=False)
        twice.load_state_dict({name: other})
        changed = OrderedDict(sd)
        changed[name] = other
        once.load_state_dict(changed)
        got = run(twice)
        _same(got, run(once))
        assert (got[0] != ref[0]).any()             # the tensor matters to the result: the first value would have shown
    finally:
        twice.close()
        once.close()


@pytest.mark.parametrize("name", [SMALL, GEMM])
def test_wrong_element_count_is_refused(base, name):
    cfg, sd, _, _, _ = base
    e = _engine(cfg)
    try:
        with pytest.raises(RuntimeError, match=r"\(-22\).*expected \d+ elements, got \d+"):
            e.load_state_dict({name: sd[name].reshape(-1)[:-1]}, finalize=False)
    finally:
        e.close()


def test_unknown_name_is_accepted_and_changes_nothing(base):
    cfg, sd, run, own, ref = base
    e = _engine(cfg)
    try:
        e.load_state_dict({"visual_encoder.no_such_tensor": np.ones(5, np.float32)}, finalize=False)
        e.load_state_dict(sd, finalize=False)
        e.load_state_dict({"text_encoder.encoder.layer.99.output.dense.bias": np.ones(cfg.txt_hidden, np.float32)})
        assert e.allocated_bytes() == own.allocated_bytes()
        _same(run(e), ref)
    finally:
        e.close()


def test_load_after_finalize_is_refused(base):
    _, sd, _, own, _ = base
    with pytest.raises(RuntimeError, match=r"\(-1\).*weights already finalized"):
        own.load_state_dict({SMALL: sd[SMALL]}, finalize=False)


def test_load_on_a_sharing_engine_is_refused(base):
    cfg, sd, run, own, ref = base
    e = _engine(cfg, share_weights_with=own)
    try:
        with pytest.raises(RuntimeError, match=r"\(-1\).*donor's weights"):
            e.load_state_dict({SMALL: sd[SMALL]}, finalize=False)
        _same(run(e), ref)
    finally:
        e.close()
