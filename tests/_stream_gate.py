"""The stream gate shared by test_stream_order_gpu.py and test_streamk_chain_gpu.py: does every launch, memset and copy of an
entry point go onto the stream the caller passed (include/pnp_hip.h: "`stream` is a hipStream_t (NULL = default stream)")?

A gated call of an entry point, on a stream S that provably runs on a hardware queue of its own:

    S   : blocker (torch.cuda._sleep, ~100 ms, waits on nothing) | event `blk` | device-to-device copies of the REAL inputs over
          the early contents | the call under test, stream = S | event `done`
    NULL: one tiny kernel right after the blocker was issued -- it must complete with `blk` pending (the default stream is not
          held up by S in this very case)
    P   : after the call returned: copies of every output and workspace to pinned host memory; P is then synchronised

Three checks:
  early write  -- with P synchronised `blk` must still be pending (else the case is inconclusive) and every copy must hold its
                  sentinel bit for bit: nothing of the call ran in front of the blocker.  A stage that escaped S has either
                  written by now or will read the early contents, which is what the next check sees;
  late inputs  -- after `done`, every output, workspace and guard block equals, bit for bit, what the same call left when it
                  was issued on the default stream with the real inputs in place from the start;
  host return  -- `blk` is still pending when the call returns, unless the header says the call may hold the host (MAY_BLOCK).
                  A call that did hold the host has nothing left to probe early: its launches were issued after the blocker
                  had ended, so for it the late-input check is the only one that applies.

Premises (a case that misses one fails as inconclusive): the blocker lasts at least 20 times as long as the call takes alone,
issue to completion on the host clock in the ungated run (it is scaled up for a slow call); S, P and the default stream run
beside one another (chosen once per module among at most 16 new streams, by blocking each and running a tiny kernel on the other).

The gate opens by itself: one blocker per case, no host action is needed to end it, no retries, no extra host threads.  Early
contents are finite values that steer no address and no loop bound; descriptors, ids, masks, tables and entropy-coded bytes are
valid from the start.  Buffers follow tests/_gpu_guard.py (a live region between two guard blocks), on bytes so that every
dtype and the 256-byte aligned workspaces of the codecs fit: the sentinel is the byte 0xA5 (a finite float in every width).
"""
import math
import time

import pytest
import torch

import _gemm_refs as R
from _gpu_guard import _bits

BLOCKER_MS = 100.0
BLOCKER_CAP_MS = 3000.0         # a call so slow that 25x its time passes this is refused as inconclusive, not waited for
SENTINEL_BYTE = 0xA5
GUARD_BYTES = 512

# Entry points that may hold the host until the stream has drained, each with the sentence of include/pnp_hip.h that says so
# (tests/test_stream_order_cpu.py holds every quote against the header).
MAY_BLOCK = {
    "pnp_post_prepare": "Synchronises once (range check).",
    "pnp_crf_set_batch": "Synchronises (lattice size + key-range flag, once per lattice built).",
    "pnp_crf_set_batch_aniso": "Synchronises as pnp_crf_set_batch does.",
    "pnp_crf_set_batch_terms": "synchronises once per lattice.",
    "pnp_crf_kl": "the value is deterministic and does not depend on the launch grid.  Synchronises.",
    "pnp_op_sort_pairs": "Both operator forms allocate their scratch per call and synchronise the stream before they free it",
    "pnp_op_scan_i32": "Both operator forms allocate their scratch per call and synchronise the stream before they free it",
    "pnp_jpeg_decode_scans": "every group's launch is timed between two events and the call synchronises",
}


@pytest.fixture(scope="module")
def blocker_cycles():
    """torch.cuda._sleep cycle count of a ~100 ms kernel: two counts timed with events, scaled linearly."""
    def ms(cycles):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(cycles)
        b.record()
        b.synchronize()
        return a.elapsed_time(b)
    ms(100_000)                                                             # first launch: module load
    c1, c2 = 1_000_000, 5_000_000
    t1, t2 = ms(c1), ms(c2)
    assert t2 > t1 > 0, (t1, t2)
    cycles = int(c2 + (BLOCKER_MS - t2) * (c2 - c1) / (t2 - t1))
    assert cycles > 0, (t1, t2)
    return cycles


def _runs_beside(blocked, other, cycles, tick):
    """Does a tiny kernel on `other` complete while a blocker of `cycles` holds `blocked`?"""
    blk, free = torch.cuda.Event(), torch.cuda.Event()
    with torch.cuda.stream(blocked):
        torch.cuda._sleep(cycles)
        blk.record()
    with torch.cuda.stream(other):
        tick.add_(1)
        free.record()
    free.synchronize()
    beside = not blk.query()
    torch.cuda.synchronize()
    return beside


def early_of(real):
    """Finite but wrong contents of the shape and type of `real` (bytes: the complement; numbers: scaled and shifted)."""
    if real.dtype == torch.uint8:
        return 255 - real
    if real.dtype.is_floating_point:
        return (real.float() * -0.5 + 0.25).to(real.dtype)
    raise TypeError(f"no early contents for {real.dtype}: integer inputs steer addresses and are valid from the start")


class Probe:
    """An output or workspace of the call under test.  Caller-owned (`Probe.new`): a live region between two guard blocks, all
    of it the sentinel byte before a run -- or, for a buffer the call reads and updates, `init` in the live region.
    Library-owned (`Probe.of`, an Engine.buffer): the buffer itself, no guards, filled with `fill` before a run; fill = None: a
    table of indices that must stay valid -- it is not armed and takes part in the late-input comparison alone."""

    def __init__(self, name, buf, live, fill, owned):
        self.name, self.buf, self.live, self.fill, self.owned = name, buf, live, fill, owned
        self.init = None
        self.host = torch.empty(buf.numel(), dtype=torch.uint8).pin_memory()

    @classmethod
    def new(cls, name, shape, dtype, init=None):
        n = int(math.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        pad = -n % 256
        buf = torch.empty(2 * GUARD_BYTES + n + pad, dtype=torch.uint8, device="cuda")
        pr = cls(name, buf, buf[GUARD_BYTES:GUARD_BYTES + n].view(dtype).view(shape), SENTINEL_BYTE, True)
        if init is not None:
            pr.init = torch.full_like(buf, SENTINEL_BYTE)
            pr.init[GUARD_BYTES:GUARD_BYTES + n].view(dtype).view(shape).copy_(init.to(dtype))
            pr.init_host = pr.init.cpu()
        return pr

    @classmethod
    def of(cls, name, tensor, fill=SENTINEL_BYTE):
        flat = tensor.reshape(-1)
        return cls(name, flat.view(torch.uint8), tensor, fill, False)

    @property
    def ptr(self):
        return self.live.data_ptr()

    def arm(self):
        if self.fill is None:
            return                                                          # compared only: it keeps what the library left
        if self.init is None:
            self.buf.fill_(self.fill)
        else:
            self.buf.copy_(self.init)

    def snapshot(self):
        return self.buf.cpu()

    def untouched(self, host_bytes):
        if self.fill is None:
            return True
        if self.init is not None:
            return torch.equal(host_bytes, self.init_host)
        return bool((host_bytes == self.fill).all())


class Case:
    """One entry point (or a short sequence of them) and what the gate needs to know about it.

    late(real[, early]) -> the device tensor the call reads: it holds `early` until the copy behind the blocker brings `real`;
    out(name, shape, dtype) / own(name, tensor) -> a probed output;  call(stream) -> 0 on success, stream a torch stream or None
    (the default stream);  setup() (optional): brings a stateful solver or engine to the state the call starts from, on the
    default stream, before each of the runs (after the inputs have been set, before the probed buffers get their sentinels);
    readout(stream) (optional): a further call on the same stream behind the one under test that is NOT under test -- it turns
    state the call left inside the library (a lattice) into a probed output.  Whatever it launches is issued after the host
    return has been judged, so a case never counts it as gated."""

    def __init__(self, name, may_block=()):
        self.name, self.may_block = name, tuple(may_block)
        self.lates, self.probes = [], []
        self.call = None
        self.setup = lambda: None
        self.readout = None

    def late(self, real, early=None):
        real = real.contiguous()
        early = early_of(real) if early is None else early.to(real.dtype).contiguous()
        assert early.shape == real.shape and not torch.equal(_bits(early.reshape(-1)), _bits(real.reshape(-1)))
        work = early.clone()
        self.lates.append((work, real, early))
        return work

    def out(self, name, shape, dtype=torch.float32, init=None, may_stay=False):
        """may_stay: a flag the call writes only when something went wrong; it need not change in the default-stream run."""
        self.probes.append(Probe.new(name, shape, dtype, init))
        self.probes[-1].may_stay = may_stay
        return self.probes[-1].live

    def own(self, name, tensor, fill=SENTINEL_BYTE):
        self.probes.append(Probe.of(name, tensor, fill))
        return tensor

    def arm(self, real):
        """Inputs early or real, then the state the call starts from, then the sentinels (setup may write what is probed)."""
        for work, r, e in self.lates:
            work.copy_(r if real else e)
        self.setup()
        for p in self.probes:
            p.arm()


def sptr(stream):
    """The hipStream_t of a torch stream for ctypes (None: the default stream)."""
    return None if stream is None else stream.cuda_stream


class Report:
    def __init__(self, name):
        self.name = name
        self.inconclusive, self.early_writes, self.late_mismatch, self.errors = [], [], [], []
        self.held_host = False
        self.t_alone = self.t_blk = 0.0

    @property
    def ordered(self):
        return not (self.early_writes or self.late_mismatch)

    def check(self, may_block=False):
        assert not self.errors, (self.name, self.errors)
        assert not self.inconclusive, f"{self.name}: inconclusive: " + "; ".join(self.inconclusive)
        assert may_block or not self.held_host, (
            f"{self.name}: the call returned only after the blocker in front of it had ended: it holds the host, and "
            f"include/pnp_hip.h does not say so")
        assert not self.early_writes, f"{self.name}: written while the blocker still held the stream: {self.early_writes}"
        assert not self.late_mismatch, (
            f"{self.name}: differs from the same call on the default stream with the inputs in place from the start "
            f"(a stage read its inputs before the stream brought them): {self.late_mismatch}")


class Gate:
    """The streams of a module (S: the gated stream, P: the prober) and the blocker, see the module docstring."""

    def __init__(self, cycles, tag):
        self.cycles, self.tag = cycles, tag
        self.tick = torch.zeros(1, device="cuda")
        null = torch.cuda.default_stream()
        assert null.cuda_stream == 0, "torch's default stream is not the NULL stream"
        short = max(1, cycles // 20)

        def both(a, b):
            return _runs_beside(a, b, short, self.tick) and _runs_beside(b, a, short, self.tick)
        chosen, tried = [], 0
        while len(chosen) < 2 and tried < 16:
            s = torch.cuda.Stream()
            tried += 1
            if both(null, s) and all(both(c, s) for c in chosen):
                chosen.append(s)
        self.tried = tried
        R.measure(f"{tag}/stream_candidates_tried", tried)
        if len(chosen) < 2:
            pytest.fail(f"inconclusive: {tried} new streams hold only {len(chosen)} that run beside the default stream and one another")
        self.S, self.P = chosen

    def run(self, case):
        rep = Report(case.name)
        tag = f"{self.tag}/{case.name}"

        def alone(timed):
            case.arm(real=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rc = case.call(None)
            if case.readout is not None:
                rc = rc or case.readout(None)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if rc:
                rep.errors.append(f"default-stream run returned {rc}")
            return dt if timed else None
        alone(False)                                                        # kernels loaded, lazy allocations made
        rep.t_alone = alone(True)
        ref = [p.snapshot() for p in case.probes]
        idle = [p.untouched(r) for p, r in zip(case.probes, ref)]          # the call writes nothing there: no early write to look for
        for p, quiet in zip(case.probes, idle):
            if quiet and p.owned and not getattr(p, "may_stay", False):
                rep.inconclusive.append(f"{p.name} still holds its initial contents after the default-stream run: nothing to probe")
            elif quiet and p.fill is not None:
                R.measure(f"{tag}/not_written/{p.name}", 1.0)
        if all(q for p, q in zip(case.probes, idle) if p.fill is not None):
            rep.inconclusive.append("the call wrote to none of the probed buffers")
        # ---- the gated run
        scale = max(1, math.ceil(25.0 * rep.t_alone / (BLOCKER_MS * 1e-3)))
        if scale * BLOCKER_MS > BLOCKER_CAP_MS:
            rep.inconclusive.append(f"the call takes {rep.t_alone:.3e} s alone: no blocker of {BLOCKER_CAP_MS} ms covers 20x that")
            return rep
        case.arm(real=False)
        torch.cuda.synchronize()
        t_start, blk, done = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True), torch.cuda.Event()
        with torch.cuda.stream(self.S):
            t_start.record()
            torch.cuda._sleep(self.cycles * scale)
            blk.record()
            for work, real, _ in case.lates:
                work.copy_(real)
        free = torch.cuda.Event()
        self.tick.add_(1)                                                   # (default stream)
        free.record()
        free.synchronize()
        null_beside = not blk.query()
        rc = case.call(self.S)
        rep.held_host = blk.query()
        if case.readout is not None:
            rc = rc or case.readout(self.S)
        done.record(self.S)
        with torch.cuda.stream(self.P):
            for p in case.probes:
                p.host.copy_(p.buf, non_blocking=True)
        self.P.synchronize()
        pending = not blk.query()
        early = [p.host.clone() for p in case.probes]
        done.synchronize()
        torch.cuda.synchronize()
        rep.t_blk = t_start.elapsed_time(blk) * 1e-3
        R.measure(tag + "/t_blk_s", rep.t_blk)
        R.measure(tag + "/t_alone_s", rep.t_alone)
        R.measure(tag + "/held_host", float(rep.held_host))
        if rc:
            rep.errors.append(f"gated run returned {rc}")
        if not null_beside:
            rep.inconclusive.append("the default stream did not run beside the blocked stream")
        if rep.t_blk < 20 * rep.t_alone:
            rep.inconclusive.append(f"blocker {rep.t_blk:.3e} s against {rep.t_alone:.3e} s for the call alone")
        if not rep.held_host:
            if not pending:
                rep.inconclusive.append("the blocker ended before the outputs had been copied out")
            rep.early_writes = [p.name for p, e, quiet in zip(case.probes, early, idle) if not quiet and not p.untouched(e)]
        rep.late_mismatch = [p.name for p, r in zip(case.probes, ref) if not torch.equal(p.snapshot(), r)]
        return rep
