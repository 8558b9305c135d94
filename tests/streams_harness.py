"""The held-back stream of tests/test_gpu_streams.py and tests/gpu_dist_streams_worker.py.

A call that is "asynchronous on `stream`" (include/crpspmm_hip.h, "Streams") must do all its device work on that stream and
nowhere else.  On the null stream that cannot be seen, so the calls run here on a NON-BLOCKING side stream S that is held back:

    with torch.cuda.stream(S):
        a delay                      torch.cuda._sleep
        a marker event
        the late fill                every dense input is copied from a staging copy; until then it holds NaN
        the sentinel fill            every output
        the call under test          without a stream= argument: the wrapper's default (torch's current stream) is under test
        the read of the outputs

Order: the outputs equal the same call made earlier on the default stream with real inputs -- a launch that went to another
stream has read NaN, or its result lies under the sentinel.  Asynchrony: the marker is still pending when the call returns.
Control: the same call with stream=0 under the same hold-back must NOT give the reference: the harness sees a mis-streamed launch.

S comes from crp_stream_create (hipStreamNonBlocking) and is wrapped in torch.cuda.ExternalStream, so that the null stream does
not wait for it whatever torch's own pool would hand out.  Only dense VALUE operands are poisoned: index arrays (row pointers,
row indices, out_pos, segment lists, the handles' structure, row maps) are valid from the start and never change, so that a
mis-ordered kernel computes with NaN and never addresses with garbage.

The delay is calibrated, not guessed: torch.cuda._sleep counts a device clock whose rate is not documented, so the first use times
_sleep with events and sizes the cycle count for DELAY_MS.  Measured on the MI355X (MEASURED below): _sleep counts 2.39e6 cycles per
ms; the slowest steady-state host call of the table, hip.gatv2_attention forward + backward with dropout (four library calls
and col_sum), takes 0.39 ms as the least of three, which is what Held.reference records and the rule is held against; the
delay is 120 ms -- at least 100 times that call, at most 250 ms."""
import ctypes as C

import numpy as np

SENTINEL = -77.25                    # what every output holds before the call (finite: a reference never holds it by accident)
# measured on an MI355X: torch.cuda._sleep counts 2.385e6 cycles per ms (the 2.4 GHz shader clock); the slowest steady-state host
# call of the table is hip.gatv2_attention forward + backward with dropout, 0.391 ms on the default stream as the least of three,
# which is what Held.reference records (before the GAT rows: hip.sparse_attention forward + backward, 0.28 ms by that measure and
# 0.52 ms as one timing)
MEASURED = dict(sleep_cycles_per_ms=2.385e6, slowest_host_call_ms=0.391,
                slowest_host_call="hip.gatv2_attention forward + backward with dropout")
DELAY_MS = 120.0                     # >= 100 * 0.391 ms with a factor of three to spare, <= 250 ms
DELAY_MAX_MS = 250.0


def bits(t):
    """the tensor's bytes as a numpy integer array (NaN-safe, sign-of-zero-safe equality)"""
    a = t.detach().cpu().contiguous().numpy()
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same(got, want):
    return len(got) == len(want) and all(np.array_equal(bits(g), bits(w)) for g, w in zip(got, want))


class Operands:
    """The dense inputs (with two data sets in staging copies) and the outputs of one call."""

    def __init__(self, gpu):
        self.gpu = gpu
        self.ins, self.outs, self.inouts = [], [], []

    def _stage(self, a):
        import torch
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
        return t.detach().to(self.gpu).clone()

    def dense(self, a0, a1=None, inout=False):
        """a dense value operand: data set 0 and data set 1 (default: set 0 negated and halved -- exact, and different)"""
        import torch
        s0 = self._stage(a0)
        s1 = self._stage(a1) if a1 is not None else s0 * -0.5
        t = torch.full_like(s0, float("nan"))
        self.ins.append((t, s0, s1))
        if inout:
            self.inouts.append(t)
        return t

    def out(self, shape, dtype):
        import torch
        t = torch.full(tuple(shape), SENTINEL, dtype=dtype, device=self.gpu)
        self.outs.append(t)
        return t

    def poison(self):
        for t, _, _ in self.ins:
            t.fill_(float("nan"))

    def load(self, k):
        for t, s0, s1 in self.ins:
            t.copy_(s1 if k else s0)

    def clear(self):
        for t in self.outs:
            t.fill_(SENTINEL)

    def snapshot(self):
        return [t.clone() for t in self.outs + self.inouts]


class Held:
    """The non-blocking side stream, the calibrated delay and the runs on it."""

    def __init__(self, lib):
        import torch
        self.lib = lib
        self.raw = []
        self.S = self._stream()
        self.cycles = None
        self.delay_ms = None
        self.host_ms = {}                # name -> host time of the steady-state call on the default stream

    def _stream(self):
        import torch
        p = C.c_void_p()
        rc = self.lib.crp_stream_create(C.byref(p))
        assert rc == 0 and p.value, rc
        self.raw.append(p)
        return torch.cuda.ExternalStream(p.value)

    def second(self):
        """a free stream of the same kind (the cross-stream cases)"""
        return self._stream()

    def close(self):
        import torch
        torch.cuda.synchronize()
        for p in self.raw:
            self.lib.crp_stream_destroy(p)
        self.raw = []

    def calibrate(self):
        """cycles of torch.cuda._sleep for DELAY_MS, from one timed _sleep on this device"""
        import torch
        if self.cycles is not None:
            return
        probe = 2 * 10 ** 6
        with torch.cuda.stream(self.S):
            torch.cuda._sleep(1000)                         # (the kernel's code object is loaded before it is timed)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            torch.cuda._sleep(probe)
            e1.record()
        e1.synchronize()
        per_ms = probe / e0.elapsed_time(e1)
        self.cycles_per_ms = per_ms
        self.cycles = int(DELAY_MS * per_ms)
        with torch.cuda.stream(self.S):
            e0.record()
            torch.cuda._sleep(self.cycles)
            e1.record()
        e1.synchronize()
        self.delay_ms = e0.elapsed_time(e1)
        print("streams_harness: _sleep runs %.4g cycles per ms; %d cycles hold S back for %.1f ms" % (per_ms, self.cycles, self.delay_ms))
        assert 0.8 * DELAY_MS <= self.delay_ms <= DELAY_MAX_MS, self.delay_ms

    def hold(self):
        """inside `with torch.cuda.stream(S)`: the delay and the marker"""
        import torch
        self.calibrate()
        torch.cuda._sleep(self.cycles)
        marker = torch.cuda.Event()
        marker.record()
        return marker

    def reference(self, ops, call, k=0, name=None):
        """the call on the default stream with data set k: the outputs (this is also the warm-up that builds the formats); the
        timed repeats give the steady-state host time"""
        import time
        import torch
        ops.load(k)
        ops.clear()
        call(None)
        torch.cuda.synchronize()
        got = ops.snapshot()
        dt = float("inf")
        for _ in range(3):                                  # (the least of three: a steady-state time, not a hiccup of the host)
            ops.load(k)
            ops.clear()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call(None)
            dt = min(dt, (time.perf_counter() - t0) * 1e3)
            torch.cuda.synchronize()
            assert same(ops.snapshot(), got), "the call does not repeat bit for bit on the default stream"
        if name is not None:
            self.host_ms[name] = dt
        assert not any(bool(torch.isnan(t).any()) for t in got if t.is_floating_point()), "the reference holds NaN"
        return got

    def warm(self, ops, call, k=0):
        """the call on S without a hold-back (torch's allocator and the runtime have served S once)"""
        import torch
        with torch.cuda.stream(self.S):
            ops.load(k)
            ops.clear()
            call(None)
        self.S.synchronize()

    def run(self, ops, call, k=0, stream=None):
        """The call on the held-back S with data set k -> (outputs read on S, whether the marker was still pending when the call
        returned).  stream=0: the control, the same call told to use the null stream."""
        import torch
        ops.poison()
        ops.clear()
        torch.cuda.synchronize()
        with torch.cuda.stream(self.S):
            marker = self.hold()
            ops.load(k)
            ops.clear()
            call(stream)
            pending = not marker.query()
            got = ops.snapshot()
        self.S.synchronize()
        torch.cuda.synchronize()
        return got, pending

    def heal(self, ops, call):
        """after a control: the call once more on the default stream with real data (a control of a value update has left NaN
        in the handle or engine, which other rows share)"""
        import torch
        ops.load(0)
        call(None)
        torch.cuda.synchronize()

    def replay(self, ops, call, k_capture=0, k_replay=1):
        """capture the call on S (one linear graph, one stream), overwrite the inputs in place with the other data set, replay"""
        import torch
        with torch.cuda.stream(self.S):
            ops.load(k_capture)
            ops.clear()
        self.S.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=self.S):
            call(None)
        with torch.cuda.stream(self.S):
            ops.load(k_replay)
            ops.clear()
            g.replay()
            got = ops.snapshot()
        self.S.synchronize()
        torch.cuda.synchronize()
        del g
        return got
