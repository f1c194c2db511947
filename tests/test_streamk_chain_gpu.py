"""GPU: the launcher invariant of the split-bf16 GEMM's stream-K tail (csrc/gemm_x3.hip, streamk_chain_launch): a stream-K launch
on one stream is ordered behind the previous stream-K launch on ANY other stream of the device, whatever the two epilogues.  An
owner workgroup of such a launch spins on partial tiles of lower-numbered workgroups of its own launch; two launches resident
together can starve each other's producers, so the launcher chains all of them through one event per device.

The ordering is checked directly, never by letting two tails race:

    stream A: a long blocker kernel that waits on nothing (torch.cuda._sleep) | event `blk` | stream-K launch X
    stream B: (issued afterwards, same host thread) stream-K launch Y | event `done`
    host    : done.synchronize(); assert blk.query()

With one chain Y waits for the event recorded behind X, X sits behind the blocker in stream order, so `done` implies `blk` --
by stream-order semantics, no timing involved.  With a chain per epilogue and X != Y, Y waits for nothing and completes beside
the running blocker: `blk` is still pending.  Either way no two stream-K kernels are resident together (Y runs beside the
blocker alone, or after X).

Premises, so that a case cannot pass vacuously (a case that misses one fails as inconclusive):
  - the blocker (calibrated once to ~100 ms) lasts at least 20 times as long as launch Y takes alone from issue to completion on
    the host clock;
  - stream B really runs beside the blocked stream A.  HIP maps streams onto a few hardware queues, and two streams that share
    one are serialised by the queue: Y would then sit behind the blocker on a library with no chain at all.  The streams are
    chosen once per module among new ones by that very probe (a tiny kernel on B completes while a short blocker holds A), and
    every case repeats it in place: the tiny kernel goes onto B between the blocker and Y and must complete with `blk` pending.
Run on the MI355X box:  python -m pytest tests/test_streamk_chain_gpu.py -m gpu -x -q
"""
import time

import pytest

torch = pytest.importorskip("torch")

import _gemm_refs as R          # noqa: E402
from _stream_gate import BLOCKER_MS, _runs_beside, blocker_cycles          # noqa: E402, F401  (the blocker and the queue probe: shared with test_stream_order_gpu.py)
from test_hip_parity import _x3_prepare, streamk_forced          # noqa: E402, F401  (the fixture: pnp_set_tuning("streamk", 2), restored to 1)

pytestmark = pytest.mark.gpu

# the smallest problem that still takes the tail: a forced tail cuts even one tile.  4 tiles (2 x 2) of 4 slab pairs each, M
# ragged, N % 4 == 0 and even (every epilogue accepts it; token columns: 442 + 70 tokens of two images)
SHAPE = (300, 512, 256)
RING = ("bias_f32", "resid_f32", "gelu_split", "plain_split", "tokcols_f32")

CASES = [(RING[i], RING[(i + 1) % 5]) for i in range(5)]                    # each epilogue once as X and once as Y
CASES += [(RING[(i + 1) % 5], RING[i]) for i in range(5)]                   # the ring reversed
CASES += [("bias_f32", "bias_f32")]                                        # same epilogue: ordered by a per-epilogue chain as well
CASES += [("resid_f32", "gelu_split", "tokcols_f32")]                      # three streams: fc2 | fc1 | cross-K/V of three pipelines


@pytest.fixture(scope="module")
def free_streams(blocker_cycles):
    """Three streams of which each runs beside each other one while that one is blocked (~5 ms blockers), i.e. on hardware
    queues of their own.  Candidates that share a queue with a chosen stream are passed over; their number is reported."""
    tick = torch.zeros(1, device="cuda")
    short = max(1, blocker_cycles // 20)
    chosen, tried = [], 0
    while len(chosen) < 3 and tried < 16:
        s = torch.cuda.Stream()
        tried += 1
        if all(_runs_beside(c, s, short, tick) and _runs_beside(s, c, short, tick) for c in chosen):
            chosen.append(s)
    R.measure("gpu/streamk_chain/stream_candidates_tried", tried)
    if len(chosen) < 3:
        pytest.fail(f"inconclusive: {tried} new streams hold only {len(chosen)} that run beside one another")
    return chosen, tick


@pytest.mark.parametrize("kinds", CASES, ids="-".join)
def test_stream_k_launch_waits_for_the_previous_one_on_another_stream(streamk_forced, blocker_cycles, free_streams, kinds):
    """kinds[0] is X (stream A, behind the blocker), kinds[1:] are Y (and Z), each on a stream of its own, issued in that order.
    Every `done` event implies `blk`; each launch took the tail (launch counter of the op-level workspace + 1 each: a launch
    adds at most one, so + len(kinds) over len(kinds) launches is one each -- reading the counter synchronises the device, so
    it is read before the blocker and after the last event only); give-up word 0; every output against float64 with the
    _x3_case budget."""
    hip = streamk_forced
    tag = "gpu/streamk_chain/" + "-".join(kinds)
    warm = [_x3_prepare(k, *SHAPE, seed=50 + i) for i, k in enumerate(kinds)]
    cases = [_x3_prepare(k, *SHAPE, seed=60 + i) for i, k in enumerate(kinds)]
    streams, tick = free_streams[0][:len(kinds)], free_streams[1]
    torch.cuda.synchronize()                                                # operands and zero fills were made on the null stream
    # ---- premise: Y alone, issue to completion on the host clock (kernels loaded and opted in by a first launch of every kind)
    for c, s in zip(warm, streams):
        c.launch(s)
        torch.cuda.synchronize()
    t_alone = 0.0
    for c, s in zip(warm[1:], streams[1:]):
        ev = torch.cuda.Event()
        t0 = time.perf_counter()
        c.launch(s)
        ev.record(s)
        ev.synchronize()
        t_alone = max(t_alone, time.perf_counter() - t0)
    n0 = hip.streamk_status_ops()[0]                                        # (device idle from here on)
    # ---- the case
    t_start, blk = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(streams[0]):
        t_start.record()
        torch.cuda._sleep(blocker_cycles)
        blk.record()
    cases[0].launch(streams[0])
    dones, beside = [], []
    for c, s in zip(cases[1:], streams[1:]):
        free = torch.cuda.Event()
        with torch.cuda.stream(s):
            tick.add_(1)
            free.record()
        free.synchronize()
        beside.append(not blk.query())                                      # premise: this stream is not held up by the blocker itself
        c.launch(s)
        dones.append(torch.cuda.Event())
        dones[-1].record(s)
    blocker_done_first = []
    for d in dones:
        d.synchronize()
        blocker_done_first.append(blk.query())
    torch.cuda.synchronize()
    t_blk = t_start.elapsed_time(blk) * 1e-3
    n1, gave_up = hip.streamk_status_ops()
    R.measure(tag + "/t_blk_s", t_blk)
    R.measure(tag + "/t_alone_s", t_alone)
    assert t_blk >= 20 * t_alone, f"inconclusive: blocker {t_blk:.3e} s against {t_alone:.3e} s for the launch alone"
    assert all(beside), f"inconclusive: stream(s) of {[k for k, ok in zip(kinds[1:], beside) if not ok]} did not run beside the blocked one"
    assert n1 - n0 == len(kinds), (n0, n1, "a launch did not take the stream-K path")
    assert gave_up == 0
    for c in cases:
        c.check()
    assert all(blocker_done_first), (
        f"stream-K launch(es) {[k for k, ok in zip(kinds[1:], blocker_done_first) if not ok]} completed while the blocker in "
        f"front of launch {kinds[0]} on another stream was still running: not ordered behind it")
