"""The case tables of tests/_engine_history.py are what they claim (no GPU): every call fits its engine, the before calls feed
the engine other numbers than the probe, the ragged and long-caption rows have the stated shapes, and the chosen geometry has the
tile tails the GPU tests rely on."""
import os
import re

import numpy as np
import pytest

import _engine_history as EH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = [(c.name, c.cap, call) for c in EH.CASES for call in c.before + (c.probe,)]


def test_geometry_has_a_one_key_tile_tail():
    assert EH.CFG.grid == 8 and EH.CFG.n_img_tokens == 65
    npad = (EH.CFG.n_img_tokens + 63) // 64 * 64               # csrc/engine.hip: Npad
    assert npad == 128 and EH.CFG.n_img_tokens - 64 == 1       # the second 64-key tile: one valid key, 63 pad keys
    assert EH.CFG.n_img_tokens % 16 == 1                       # and a 16-key tile of the cross-attention with one valid key
    assert 0 <= EH.HEAD < EH.CFG.txt_heads and 0 <= EH.STASH_LAYER < EH.CFG.txt_layers
    assert EH.CFG.max_pos >= EH.CAP_LONG


def test_long_switch_is_the_kernels_own():
    src = open(os.path.join(ROOT, "pnp-ovss_amd", "csrc", "text_kernels.hip")).read()
    assert int(re.search(r"constexpr int TXT_MAX_L = (\d+);", src).group(1)) == EH.TXT_MAX_L
    long_rows = [c for c in EH.CASES if c.cap == EH.CAP_LONG]
    assert long_rows
    for c in long_rows:                                        # a long-kernel call, then a short-kernel call
        assert max(EH.shape_of(b)[1] for b in c.before) > EH.TXT_MAX_L >= EH.shape_of(c.probe)[1]
    for c in EH.CASES:
        if c.cap == EH.CAP_SHORT:
            assert all(EH.shape_of(x)[1] <= 64 for x in c.before + (c.probe,) if x.kind != "project")


@pytest.mark.parametrize("name,cap,call", CALLS, ids=[f"{n}:{EH.call_id(c)}" for n, _, c in CALLS])
def test_every_call_fits_its_engine(name, cap, call):
    a = EH.inputs(call, cap)
    if call.kind == "project":
        assert call.which in (0, 1) and a["x"].shape == (call.rows, (EH.CFG.vit_dim, EH.CFG.txt_hidden)[call.which])
        return
    B, L = EH.shape_of(call)
    assert a["L"] == L == int(a["mask"].sum(1).max()) and L <= cap < a["ids"].shape[1]
    assert tuple(a["mask"].sum(1)) == call.lens
    assert a["ids"].shape == a["mask"].shape == (B, cap + EH.LD_EXTRA)
    assert a["ids"].max() < EH.CFG.vocab and np.array_equal(a["mask"], (a["ids"] != EH.CFG.pad_token_id).astype(np.int64))
    if call.kind == "text":
        assert L >= 2
    else:
        assert L >= 5 and B <= EH.MAX_BATCH and a["imgs"].shape == (B, 3, EH.CFG.img_size, EH.CFG.img_size)
    if call.kind == "drop_loop":
        assert call.drop_iter >= 1 and call.drop_iter * 10 <= EH.CFG.grid ** 2
    if call.layer is not None:
        assert EH.STASH_LAYER <= call.layer < EH.CFG.txt_layers
    if call.dropped_seed is not None:
        assert a["dropped"].shape == (B, EH.CFG.grid ** 2) and (a["dropped"].sum(1) == 10).all()


@pytest.mark.parametrize("case", EH.CASES, ids=[c.name for c in EH.CASES])
def test_before_and_probe_inputs_differ(case):
    p = EH.inputs(case.probe, case.cap)
    for b in case.before:
        assert b.seed != case.probe.seed
        if b.kind == "project":
            continue
        a = EH.inputs(b, case.cap)
        rows = min(len(b.lens), len(case.probe.lens))
        assert not np.array_equal(a["ids"][:rows], p["ids"][:rows])
        for r in range(rows):                                  # every caption, not just one of them
            n = min(b.lens[r], case.probe.lens[r]) - 1
            assert n <= 4 or not np.array_equal(a["ids"][r, 4:n], p["ids"][r, 4:n])
        if "imgs" in a and "imgs" in p:
            for r in range(rows):
                assert np.abs(a["imgs"][r] - p["imgs"][r]).max() > 0.5
    last = case.before[-1]
    same = last.kind == case.probe.kind and EH.shape_of(last) == EH.shape_of(case.probe)
    assert case.same_shape == same


def test_the_table_is_the_stated_one():
    by = {c.name: c for c in EH.CASES}
    assert len(by) == len(EH.CASES) == 12
    sh = lambda call: EH.shape_of(call)                        # noqa: E731
    assert sh(by["b4_then_b1"].before[0]) == (4, 12) and sh(by["b4_then_b1"].probe) == (1, 12)
    assert sh(by["b4_then_b3"].before[0]) == (4, 12) and sh(by["b4_then_b3"].probe) == (3, 12)
    assert sh(by["l25_then_l7"].before[0]) == (3, 25) and sh(by["l25_then_l7"].probe) == (3, 7)
    assert sh(by["l7_then_l25"].before[0]) == (3, 7) and sh(by["l7_then_l25"].probe) == (3, 25)
    assert sh(by["l200_then_l25"].before[0]) == (2, 200) and sh(by["l200_then_l25"].probe) == (2, 25)
    assert by["l200_then_l25"].cap == EH.CAP_LONG and all(c.cap == EH.CAP_SHORT for c in EH.CASES if c.name != "l200_then_l25")
    r = by["full_then_ragged"]
    assert r.before[0].lens == (25, 25, 25) and r.probe.lens == (5, 11, 25) and r.same_shape
    assert all(n < r.cap + EH.LD_EXTRA for n in r.probe.lens)  # rows shorter than ld
    o = by["other_entry_points"]
    assert [b.kind for b in o.before] == ["gradcam", "text", "project", "project", "gradcam"]
    assert sh(o.before[0]) == (4, 12) and sh(o.before[1]) == (6, 9) and 6 % EH.MAX_BATCH == 2 and 6 > EH.MAX_BATCH
    assert {b.which for b in o.before if b.kind == "project"} == {0, 1}
    # the bf16 engine casts the rows into the ViT's xn scratch, max_batch * N * D / K rows at a time: text_proj takes two rounds
    assert o.before[3].rows > EH.MAX_BATCH * EH.CFG.n_img_tokens * EH.CFG.vit_dim // EH.CFG.txt_hidden
    assert o.before[4].layer == 9 and o.probe.layer is None and sh(o.probe) == (2, 12)
    for n, kind, it in (("loop_then_gradcam", "gradcam", None), ("loop_then_loop4", "drop_loop", 4), ("loop_then_loop1", "drop_loop", 1)):
        c = by[n]
        assert c.before[0].kind == "drop_loop" and sh(c.before[0]) == (4, 12) and c.before[0].drop_iter == 4
        assert c.probe.kind == kind and c.probe.drop_iter == it and sh(c.probe) == (2, 12) and c.probe.dropped_seed is None
    d = by["dropped_then_none"]
    assert d.before[0].dropped_seed is not None and d.probe.dropped_seed is None and sh(d.before[0]) == sh(d.probe) == (3, 12)
    t = by["gradcam_then_text"]
    assert sh(t.before[0]) == (4, 25) and t.before[0].kind == "gradcam" and t.probe.kind == "text" and sh(t.probe) == (3, 6)


def test_probes_are_shared_and_modes_are_the_four():
    ps = EH.probes()
    assert len(ps) == len(set(ps)) == 10 and {(c.cap, c.probe) for c in EH.CASES} == set(ps)
    assert all(p.seed == EH.PROBE_SEED for _, p in ps)
    assert EH.MODES == (("f32", 1), ("bf16", 1), ("bf16x3", 1), ("bf16x3", 2))
    sd = EH.state_dict()
    assert {"vision_proj.weight", "text_proj.weight", "itm_head.weight"} <= set(sd)
