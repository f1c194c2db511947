"""An engine call reads nothing that an earlier call on the same engine wrote ("What a call may carry over"): the ViT,
cross K / V, text stack, backward, gather, drop loop and the text-only / projection passes, after calls of other shapes.

For every row of tests/_engine_history.py a USED engine runs the `before` calls and then the probe; a PRISTINE engine -- same
config, capacity, stash layer and mode, the used engine's weights (share_weights_with), nothing run on it -- runs the probe alone.
Every output of the probe must be equal bit for bit (torch.equal): the reference is the same code on untouched memory, so there is
no tolerance.  One used engine per (mode, capacity) serves all rows of the module, so each row also sees the rows before it.
(Most of a new engine's workspace is not cleared at creation: it holds zeros or what a closed engine left there -- in either case
not the used engine's history, which is all the comparison needs.)

Three mutants of csrc/model.hip, each one stale read, fail these rows and the unmodified library passes: pnp_drop_loop_layer
without its clear of the dropped mask (loop_then_loop4); the text-prefix reuse switched on for pnp_compute_gradcam_layer (every
compute_gradcam probe); text_self_attn called with the largest L the engine has seen (every row behind a longer caption).

Controls: two pristine engines agree on every probe (else bit equality would mean nothing for that kernel), and in fp32 the
pristine probes of row 1 agree with the numpy oracle (else used and pristine could be wrong together)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import _engine_history as EH                       # noqa: E402
from oracle import blip_itm_np as OM               # noqa: E402

pytestmark = pytest.mark.gpu

_SD = {}


def _state_dict():
    if not _SD:
        _SD.update(EH.state_dict())
    return _SD


def _new_engine(mode, cap, donor=None):
    from pnp_ovss.hip import Engine
    e = Engine(EH.CFG, max_batch=EH.MAX_BATCH, max_text_len=cap, stash_layer=EH.STASH_LAYER, mode=mode, share_weights_with=donor)
    if donor is None:
        e.load_state_dict(_state_dict())
    return e


class Rig:
    """The used engines of one mode (one per capacity, made on first use) and the probes' pristine references."""

    def __init__(self, mode, streamk):
        self.mode, self.streamk, self.engines, self.refs = mode, streamk, {}, {}

    def used(self, cap):
        if cap not in self.engines:
            self.engines[cap] = _new_engine(self.mode, cap)
        return self.engines[cap]

    def pristine_run(self, cap, probe):
        """The probe on an engine that runs nothing else, as host tensors."""
        e = _new_engine(self.mode, cap, donor=self.used(cap))
        try:
            return tuple(t.cpu() for t in EH.run_call(e, probe, cap))
        finally:
            e.close()

    def reference(self, cap, probe):
        if (cap, probe) not in self.refs:
            self.refs[cap, probe] = self.pristine_run(cap, probe)
        return self.refs[cap, probe]

    def close(self):
        for e in self.engines.values():
            e.close()
        self.engines.clear()


@pytest.fixture(scope="module", params=EH.MODES, ids=[m if sk == 1 else f"{m}-streamk{sk}" for m, sk in EH.MODES])
def rig(request):
    """pnp_set_tuning("streamk", 2) cuts every partial last tile round of the split-bf16 GEMMs along K: its partial-tile slots
    and flags are a history channel of their own."""
    from pnp_ovss import hip
    mode, sk = request.param
    hip.set_tuning("streamk", sk)
    r = Rig(mode, sk)
    try:
        yield r
    finally:
        r.close()
        hip.set_tuning("streamk", 1)


def _assert_same(tag, got, ref):
    assert len(got) == len(ref), tag
    for i, (a, b) in enumerate(zip(got, ref)):
        a = a.cpu()
        assert a.shape == b.shape and a.dtype == b.dtype, (tag, i)
        if not torch.equal(a, b):
            d = (a.double() - b.double()).abs()
            raise AssertionError(f"{tag}: output {i} {tuple(a.shape)} differs in {int((a != b).sum())} elements, max |diff| "
                                 f"{float(d.max()):.3e} (max |ref| {float(b.double().abs().max()):.3e})")


@pytest.mark.parametrize("case", EH.CASES, ids=[c.name for c in EH.CASES])
def test_probe_does_not_see_earlier_calls(rig, case):
    ref = rig.reference(case.cap, case.probe)                  # (first: a pristine engine is made while the used one is as it was)
    e = rig.used(case.cap)
    last = None
    for b in case.before:
        last = EH.run_call(e, b, case.cap)
    got = EH.run_call(e, case.probe, case.cap)
    if case.same_shape:                                        # the before call left other numbers in the very same rows
        assert last[0].shape == got[0].shape and not torch.equal(last[0], got[0])
    for t in got:
        assert bool(torch.isfinite(t.float()).all())
    if rig.streamk == 2:                                       # the forced mode did cut the ViT's tile rounds, and no spin gave up
        launches, gave_up = e.streamk_status()
        assert launches > 0 and gave_up == 0, (launches, gave_up)
    _assert_same(f"{rig.mode} {case.name}", got, ref)


@pytest.mark.parametrize("cap,probe", EH.probes(), ids=[f"cap{c}-{EH.call_id(p)}" for c, p in EH.probes()])
def test_two_pristine_engines_agree(rig, cap, probe):
    """Control 1: the probe is a function of its inputs at all (no unordered accumulation)."""
    _assert_same(f"{rig.mode} pristine twice", rig.pristine_run(cap, probe), rig.reference(cap, probe))


@pytest.mark.parametrize("probe", [EH.P_B1_L12, EH.P_B3_L12], ids=EH.call_id)
def test_pristine_f32_probe_vs_oracle(probe):
    """Control 2: criterion and bounds of test_hip_parity.py::test_gradcam_small_vs_reference_golden[False]."""
    a = EH.inputs(probe, EH.CAP_SHORT)
    maps, ref_logits, _ = OM.compute_gradcam(_state_dict(), EH.CFG, a["imgs"], a["ids"], a["mask"], layers=[EH.STASH_LAYER])
    ref = maps[EH.STASH_LAYER][:, EH.HEAD]
    e = _new_engine("f32", EH.CAP_SHORT)
    try:
        out, logits = EH.run_call(e, probe, EH.CAP_SHORT)
        got, logits = out.cpu().numpy(), logits.cpu().numpy()
    finally:
        e.close()
    nerr = float(np.abs(EH.norm01(got) - EH.norm01(ref)).max())
    print(f"[measured] {EH.call_id(probe)}: logits {np.abs(logits - ref_logits).max():.3e} maps {np.abs(got - ref).max():.3e} "
          f"normalised {nerr:.3e}")
    np.testing.assert_allclose(logits, ref_logits, rtol=0, atol=5e-3)
    assert np.abs(got - ref).max() < 1e-4
    assert nerr < 2e-4
