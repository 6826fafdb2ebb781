"""Device batches with calls in flight on a caller's stream (include/dsd2dxd_amd.h: d2d_translate_batch_device is asynchronous, frames_out is
known at return, successive calls need only be ordered on the device, d2d_peak / d2d_reset / d2d_seek wait for the engine's work themselves).

Every other test of the device entry points waits for the device after each call, so the host-side machinery that exists only for calls in
flight (dsd2dxd_amd/csrc/d2d_engine.cpp: the ring of JOB_SLOTS pinned job tables and its slot-reuse wait, the single device job table, the
ping-pong state flipped on the host at enqueue time, buffers that regrow between two enqueued calls, last_stream, the profiling event pool,
the null-stream fills of create / reset / seek) never ran the way bench.py and the many-file path drive it.  Here it does.

The harness.  The caller's streams are made with hipStreamCreateWithFlags(hipStreamNonBlocking) through ctypes on the HIP runtime torch has
loaded (the null stream orders nothing against them) and wrapped in torch.cuda.ExternalStream.  Every buffer exists before the first call:
the inputs in one pinned tensor, a slot per call and file; two device input and two device output buffers per file, used round-robin; a
pinned result tensor with a slot per call and file.  Call k's bytes go up with a non-blocking copy on the call's stream, its frames come
down on the same stream, so call k + 2 overwrites what call k read and wrote and only stream order protects the bytes.  The reference is the
oracle fed the same calls, computed before the first enqueue and shared by the runs of a test.  Between the first and the last enqueue of a
sequence the test waits for nothing; after every enqueue it checks what the header says is known without a wait (frames_out, tell(),
next_frames() of the call that follows).  Frames are compared with np.array_equal, peaks and positions with ==.

Proof that calls were pending.  A call of a few KiB finishes faster than the host enqueues the next, so each sequence starts with a call made
before the blocker (it sizes the buffers that are allocated on first use, whose allocation waits for the stream), then puts a blocker on the
stream -- torch.cuda._sleep for BLOCK_MS, its cycles calibrated once with events -- records an event behind it, enqueues exactly JOB_SLOTS
calls and asserts that the event has not completed: eight calls pending, every ring slot taken.  The call after them waits inside
enqueue_jobs for its slot.  A blocker that has ended by then fails the test with a message that says so; nothing skips or retries.
Measured on an MI355X: the host needs 0.45 ms for eight enqueues of the largest case (cascade_config5_8ch_il, three files of eight channels,
each call with its three uploads and three downloads), between 0.35 and 0.51 ms for every other case, 1.0 ms for the eight rounds of the
three interleaved engines; BLOCK_MS = 5 ms is about ten times that (three times as long for the three engines).  The blockers then
measured 5.0 ms: _sleep counts shader clocks, calibrated with the clock up, so a lower clock only lengthens them.

Every sequence is also run once on an engine of its own with a wait after each call (Driver's wait=True): it loads the kernels before the
timed stretch, tells a route that is wrong anyway from one that is wrong only in flight, and is test 6's reference for the launch count.

The harness itself was tried on the GPU: with two per-call result slots swapped in Driver the comparison fails and names the first of
the two calls."""
import ctypes as C
import time

import numpy as np
import pytest

from helpers import pack_layout, random_bytes
from test_gpu_long_streams import ENGINE_ONLY, MONO, MONO_KERNEL, NS_ROUTES, PAIR_KERNEL, ROUTES

pytestmark = pytest.mark.gpu

JOB_SLOTS = 8                       # dsd2dxd_amd/csrc/d2d_engine.cpp
DBG_NO_COOP = 1 << 2                # dsd2dxd_amd/_capi.py (asserted against it in Ref)
ENQUEUE_MS_MEASURED = 0.45         # host time of JOB_SLOTS enqueues of the largest case, measured (see the module's text)
BLOCK_MS = 5.0                      # the blocker: about ten times that
NB = 4096                           # the nominal block of a call's length
STREAM = 1 << 19                    # bytes per channel of every file's stream
EMPTY = np.zeros(0, dtype=np.uint8)
SENTINEL = 12345                    # frames_out before a call: the call must write it


# ---- the caller's streams: non-blocking, made on the runtime torch has loaded ----

_HIP = None


def hip_runtime():
    global _HIP
    if _HIP is None:
        import torch
        torch.cuda.init()
        with open("/proc/self/maps") as f:
            paths = sorted({ln.split()[-1] for ln in f if "libamdhip64" in ln})
        assert len(paths) == 1, paths                    # one HIP runtime in the process (dsd2dxd_amd/_capi.py: lib())
        L = C.CDLL(paths[0])
        L.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
        L.hipStreamGetFlags.argtypes = [C.c_void_p, C.POINTER(C.c_uint)]
        L.hipStreamDestroy.argtypes = [C.c_void_p]
        L.hipHostMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_uint]
        L.hipHostFree.argtypes = [C.c_void_p]
        _HIP = L
    return _HIP


class Session:
    """n non-blocking streams (at most four alive), the engines and the pinned memory of a test; on the way out, whatever happened: wait for
    every stream, close the engines, destroy the streams, free the pinned memory.
    The pinned memory is hipHostMalloc's own, not torch's: torch's pinned-memory cache remembers the streams a block was copied on and records
    an event on each of them when the block is freed -- for a tensor that outlives the test's streams, on a destroyed stream."""
    HIP_STREAM_NON_BLOCKING = 1

    def __init__(self, n):
        assert 1 <= n <= 4
        self.n, self.handles, self.streams, self.engines, self.host = n, [], [], [], []

    def __enter__(self):
        import torch
        L = hip_runtime()
        calibrate()
        for _ in range(self.n):
            h, flags = C.c_void_p(), C.c_uint(0)
            assert L.hipStreamCreateWithFlags(C.byref(h), self.HIP_STREAM_NON_BLOCKING) == 0 and h.value
            assert L.hipStreamGetFlags(h, C.byref(flags)) == 0 and flags.value & self.HIP_STREAM_NON_BLOCKING
            self.handles.append(h)
            self.streams.append(torch.cuda.ExternalStream(h.value))
            assert self.streams[-1].cuda_stream == h.value
        return self

    def engine(self, d, **kw):
        e = d.Engine(**kw)
        self.engines.append(e)
        return e

    def pinned(self, nbytes, fill):
        """(tensor, numpy array) over nbytes of pinned host memory"""
        import torch
        p = C.c_void_p()
        assert hip_runtime().hipHostMalloc(C.byref(p), nbytes, 0) == 0 and p.value and p.value % 16 == 0
        self.host.append(p)
        a = np.ctypeslib.as_array((C.c_uint8 * nbytes).from_address(p.value))
        a[:] = fill
        t = torch.from_numpy(a)
        assert t.is_pinned() and t.data_ptr() == p.value
        return t, a

    def __exit__(self, *exc):
        for s in self.streams:
            s.synchronize()
        for e in self.engines:
            e.close()
        for h in self.handles:
            assert hip_runtime().hipStreamDestroy(h) == 0
        for p in self.host:
            assert hip_runtime().hipHostFree(p) == 0
        return False


_CYCLES_PER_MS = None


def calibrate():
    """cycles of torch.cuda._sleep per millisecond: once per process, on torch's own stream, with events, before any sequence (Session)"""
    global _CYCLES_PER_MS
    import torch
    if _CYCLES_PER_MS is None:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(2_000_000)        # (clocks up before the timed one)
        a.record()
        torch.cuda._sleep(4_000_000)
        b.record()
        b.synchronize()
        _CYCLES_PER_MS = 4_000_000 / a.elapsed_time(b)
        print(f"blocker: {_CYCLES_PER_MS:.0f} cycles of torch.cuda._sleep per ms")


class Blocker:
    """BLOCK_MS of device work on `stream` between two events; ms(): how long it really was, once the stream has been waited for"""

    def __init__(self, stream, ms=BLOCK_MS):
        import torch
        self.begin, self.end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.begin.record(stream)
        with torch.cuda.stream(stream):
            torch.cuda._sleep(int(ms * _CYCLES_PER_MS))
        self.end.record(stream)

    def ms(self):
        return self.begin.elapsed_time(self.end)


def still_pending(blockers, what, host_ms):
    for b in blockers:
        assert not b.end.query(), (f"{what}: the blocker (BLOCK_MS = {BLOCK_MS}) had ended when {JOB_SLOTS} calls were enqueued (the host took {host_ms:.2f} ms "
                                   f"for them, {ENQUEUE_MS_MEASURED} ms when the blocker was sized): it is too short to prove that the calls were pending")
    print(f"enqueue: {what}: {JOB_SLOTS} calls each on {len(blockers)} stream(s) in {host_ms:.3f} ms of host time, the blocker still running")


# ---- the reference: one oracle per file, fed the same calls ----

class Call:
    def __init__(self, prime, lens):
        self.prime, self.lens = prime, list(lens)
        self.inputs, self.want, self.nfr, self.would, self.tell = [], [], [], [], []


class Ref:
    """n files of random bytes, one oracle each; feed() a call's lengths in the order the engine will get them, seek() / reset() in between.
    calls[k]: every file's input in the engine's layout, its frames, their count (would: the count a translate yields -- what next_frames
    answers; nfr: 0 for a prime) and where the file stands once the call is enqueued; peaks: of the frames fed since the last seek / reset"""

    def __init__(self, d, O, kw, n_files, seed):
        assert d.DBG_NO_COOP == DBG_NO_COOP
        self.kw = dict(kw, filter="E", seed=seed)
        self.okw = {k: v for k, v in self.kw.items() if k not in ENGINE_ONLY}
        self.O, self.n, self.C = O, n_files, kw["channels"]
        self.o = [O.Oracle(**self.okw) for _ in range(n_files)]
        self.o0 = O.Oracle(**self.okw)                    # never fed, never sought: F(position)
        self.F = self.o0.max_frames
        self.fb = self.o0.frame_bytes
        self.chans = [[random_bytes(STREAM, 1000 * seed + 10 * f + c) for c in range(self.C)] for f in range(n_files)]
        self.at, self.frames = [0] * n_files, [0] * n_files
        self.peaks = [[0.0] * self.C for _ in range(n_files)]
        self.calls = []

    def feed(self, lens, prime=False):
        call = Call(prime, lens)
        for f, L in enumerate(lens):
            a = self.at[f]
            assert a + L <= STREAM
            buf, w, fr = EMPTY, EMPTY, 0
            if L:
                buf = pack_layout([c[a:a + L] for c in self.chans[f]], self.kw["fmt"], self.kw["block_size"])
                w, fr, y = self.o[f].translate(buf, want_f64=True)
                if fr and not prime:
                    self.peaks[f] = [max(p, float(np.abs(y[:fr, c]).max())) for c, p in enumerate(self.peaks[f])]
            self.at[f] += L
            self.frames[f] += fr
            call.inputs.append(buf)
            call.would.append(fr)
            call.nfr.append(0 if prime else fr)
            call.want.append(EMPTY if prime else w[:fr * self.fb].copy())
            call.tell.append((self.at[f], self.frames[f]))
        self.calls.append(call)
        return call

    def seek(self, f, pos):
        self.o[f].seek(pos)
        self.at[f], self.frames[f], self.peaks[f] = pos, self.F(pos), [0.0] * self.C

    def reset(self):
        for o in self.o:
            o.close()
        self.o = [self.O.Oracle(**self.okw) for _ in range(self.n)]
        self.at, self.frames = [0] * self.n, [0] * self.n
        self.peaks = [[0.0] * self.C for _ in range(self.n)]

    def close(self):
        for o in self.o + [self.o0]:
            o.close()


def ragged_lens(ref, n_calls, seed, zero_at=None, noframe_at=None, first_longest=True):
    """Call lengths cut as tests/test_gpu_fuzz.py cuts them, at any byte: one to three blocks of NB bytes per channel, every other one with a
    ragged tail, different per file and call.  Call zero_at is 0 bytes for every file; call noframe_at gives file 1 a single byte that
    completes no frame (the call before it grows by a byte where that byte would complete one).  Call 0, which precedes the blocker, holds
    the longest length of all, so that no buffer regrows behind it."""
    rng = np.random.default_rng(seed)
    lens = [[int(rng.integers(1, 4)) * NB + (int(rng.integers(1, NB)) if rng.integers(2) else 0) for _ in range(ref.n)] for _ in range(n_calls)]
    if first_longest:
        lens[0][0] = 3 * NB + NB - 1
    if zero_at is not None:
        lens[zero_at] = [0] * ref.n
    if noframe_at is not None:
        assert noframe_at - 1 not in (0, zero_at)
        pos = sum(l[1] for l in lens[:noframe_at])
        for _ in range(64):
            if ref.F(pos + 1) == ref.F(pos):
                break
            lens[noframe_at - 1][1] += 1
            pos += 1
        assert ref.F(pos + 1) == ref.F(pos)
        lens[noframe_at][1] = 1
    return lens


# ---- the driver: buffers, enqueue, host state at return, the comparison ----

def r16(x):
    return (x + 15) & ~15


class Driver:
    """One engine and the buffers of ref.calls, all allocated here.  enqueue(k, stream): upload, call, download, all on `stream`, then the
    host-state checks; wait=True: the control run, which waits for the stream after each call.  kernel: the FIR kernel every call that
    produces FIR outputs must have launched, or a function of the call."""

    def __init__(self, d, ses, e, ref, kernel=None, wait=False):
        import torch
        self.d, self.e, self.ref, self.calls, self.kernel, self.wait = d, e, ref, ref.calls, kernel, wait
        n, fb = ref.n, e.frame_bytes
        assert fb == ref.fb and e.n_files == n
        self.fb = fb
        self.in_off, self.out_off = [], []
        pi = po = 0
        for call in self.calls:
            self.in_off.append([]); self.out_off.append([])
            for f in range(n):
                self.in_off[-1].append(pi); pi += r16(call.inputs[f].size)
                self.out_off[-1].append(po); po += r16(call.nfr[f] * fb)
        self.pin_in, host_in = ses.pinned(pi + 16, 0)
        self.pin_out, self.host_out = ses.pinned(po + 16, 0xEE)
        for call, offs in zip(self.calls, self.in_off):
            for f, b in enumerate(call.inputs):
                host_in[offs[f]:offs[f] + b.size] = b
        dev = torch.device("cuda", 0)
        cap_in = [r16(max(c.inputs[f].size for c in self.calls)) + 16 for f in range(n)]
        self.cap_out = [r16(max(c.nfr[f] for c in self.calls) * fb) + 16 for f in range(n)]
        self.din = [[torch.zeros(cap_in[f], dtype=torch.uint8, device=dev) for _ in range(2)] for f in range(n)]
        self.dout = [[torch.full((self.cap_out[f],), 0xDD, dtype=torch.uint8, device=dev) for _ in range(2)] for f in range(n)]
        self.rebuild()
        self.names, self.done = [], 0
        torch.cuda.synchronize()                          # (the fills above ran on torch's stream; nothing of a sequence is enqueued yet)

    def rebuild(self):
        """the per-call argument tables and copy lists, from the offsets (the views are made here, not between the enqueues)"""
        n, fb = self.ref.n, self.fb
        self.ios, self.up, self.down = [], [], []
        for k, call in enumerate(self.calls):
            ios = (self.d.FileIO * n)()
            up, down = [], []
            for f in range(n):
                di, do = self.din[f][k % 2], self.dout[f][k % 2]
                nin, nout = call.inputs[f].size, call.nfr[f] * fb
                ios[f].dsd, ios[f].bytes_per_channel = di.data_ptr(), call.lens[f]
                ios[f].pcm, ios[f].pcm_capacity_bytes = do.data_ptr(), self.cap_out[f]
                ios[f].frames_out = SENTINEL
                if nin:
                    up.append((di[:nin], self.pin_in[self.in_off[k][f]:self.in_off[k][f] + nin]))
                if nout:
                    down.append((self.pin_out[self.out_off[k][f]:self.out_off[k][f] + nout], do[:nout]))
            self.ios.append(ios); self.up.append(up); self.down.append(down)

    def enqueue(self, k, stream):
        import torch
        e, call, n = self.e, self.calls[k], self.ref.n
        assert k == self.done
        # what the call that follows the last one yields is known before it is made
        assert [e.next_frames(call.lens[f], file=f) for f in range(n)] == call.would, f"call {k}: next_frames"
        with torch.cuda.stream(stream):
            for dst, src in self.up[k]:
                dst.copy_(src, non_blocking=True)
        (e.prime_batch_device if call.prime else e.translate_batch_device)(self.ios[k], stream.cuda_stream)
        with torch.cuda.stream(stream):
            for dst, src in self.down[k]:
                dst.copy_(src, non_blocking=True)
        # known at return, without a wait
        assert [self.ios[k][f].frames_out for f in range(n)] == call.nfr, f"call {k}: frames_out"
        assert [e.tell(file=f) for f in range(n)] == call.tell, f"call {k}: tell"
        if any(call.would) and not call.prime:
            self.names.append((k, e.kernel_name()))
        self.done = k + 1
        if self.wait:
            stream.synchronize()

    def check(self, what):
        """once every stream has been waited for: every call's frames, the bytes around them in the result tensor, the peaks, the kernels"""
        out = self.host_out
        fb = self.fb
        assert self.done == len(self.calls)
        for k, call in enumerate(self.calls):
            for f, want in enumerate(call.want):
                o = self.out_off[k][f]
                got = out[o:o + want.size]
                if not np.array_equal(got, want):
                    fr = int(np.flatnonzero(got != want)[0]) // fb
                    raise AssertionError(f"{what}: call {k}, file {f}: frame {fr} of {call.nfr[f]} is the first that differs from the oracle's "
                                         f"({int((got != want).sum())} bytes differ)")
                assert np.all(out[o + want.size:o + r16(want.size)] == 0xEE), f"{what}: call {k}, file {f}: bytes behind the frames"
        self.check_peaks(what)
        for k, name in self.names:
            want = self.kernel(self.calls[k]) if callable(self.kernel) else self.kernel
            assert want is None or name == want, f"{what}: call {k} launched {name}"

    def check_peaks(self, what):
        C_ = self.e.out_channels
        assert [[self.e.peak(c, file=f) for c in range(C_)] for f in range(self.ref.n)] == self.ref.peaks, f"{what}: peaks"


def run(drv, stream, what, before=None):
    """the sequence of one engine on one stream: call 0, the blocker, JOB_SLOTS calls, the proof, the rest (before[k](engine): a host call
    made in front of call k, with no wait of the test's own).  The control run (drv.wait) has no blocker."""
    before = before or {}
    assert len(drv.calls) > JOB_SLOTS + 1 and not any(k <= JOB_SLOTS for k in before)
    drv.enqueue(0, stream)
    blocked = None if drv.wait else Blocker(stream)
    t0 = time.perf_counter()
    for k in range(1, JOB_SLOTS + 1):
        drv.enqueue(k, stream)
    if blocked:
        still_pending([blocked], what, (time.perf_counter() - t0) * 1e3)
    for k in range(JOB_SLOTS + 1, len(drv.calls)):
        if k in before:
            before[k](drv.e)
        drv.enqueue(k, stream)
    return blocked


def both_runs(d, ses, ref, kernel, what, before=None):
    """the control run (a wait after each call), then the run in flight, each on a fresh engine; returns the two drivers, everything waited for
    and compared"""
    stream = ses.streams[0]
    drivers = []
    for wait in (True, False):
        e = ses.engine(d, n_files=ref.n, **ref.kw)
        drv = Driver(d, ses, e, ref, kernel, wait=wait)
        label = f"{what}, {'a wait after each call' if wait else 'in flight'}"
        blocked = run(drv, stream, label, before)
        stream.synchronize()
        if blocked:
            print(f"blocker: {label}: {blocked.ms():.1f} ms")
        drv.check(label)
        assert [e.tell(file=f) for f in range(ref.n)] == ref.calls[-1].tell
        drivers.append(drv)
    return drivers


# ---- 1. calls in flight equal the oracle, one route per distinct call structure of launch_call ----

CASCADE = ROUTES["cascade_dsd256_96k"]
INFLIGHT = {k: ROUTES[k] for k in ("fp6_m32_t24", "lut_176k", "two_group_3ch_t20", "fp6_il2", "fp6_taps32_two_pass_mono", "px_kind1_dsd64_96k",
                                   "cascade_dsd256_96k", "cascade_config5_8ch_il")}
INFLIGHT.update({k: NS_ROUTES[k] for k in ("ns_s16_0db", "ns_48k_dsd64_96k")})
INFLIGHT["fp6_il2_no_coop"] = (dict(ROUTES["fp6_il2"][0], debug=DBG_NO_COOP), ROUTES["fp6_il2"][1])      # the de-interleave pre-pass: one d_planar for all calls
INFLIGHT["cascade_dsd256_96k_ns"] = (dict(CASCADE[0], dither="N"), CASCADE[1])                             # d_ys
N_CALLS = 3 * JOB_SLOTS


@pytest.mark.parametrize("route", sorted(INFLIGHT))
def test_calls_in_flight_equal_the_oracle(engine_lib, oracle_mod, route):
    """three files, call 0 and then 24 calls behind the blocker with nothing waited for: ragged lengths, call 10 of 0 bytes for every file,
    call 13 without a frame for file 1"""
    kw, kernel = INFLIGHT[route]
    ref = Ref(engine_lib, oracle_mod, kw, 3, 5000 + sorted(INFLIGHT).index(route))
    for lens in ragged_lens(ref, 1 + N_CALLS, 5000, zero_at=10, noframe_at=13):
        ref.feed(lens)
    assert ref.calls[13].nfr[1] == 0 and ref.calls[13].nfr[0] > 0 and not any(ref.calls[10].nfr)
    with Session(1) as ses:
        both_runs(engine_lib, ses, ref, kernel, route)
    ref.close()


def test_mono_pair_in_flight(engine_lib, oracle_mod):
    """a mono engine of three files: where every file's call is whole 16-byte chunks in both halves the pair kernel runs, the second half's
    history taken from the caller's input buffer of that call; the 0-byte call and the call with a single byte for file 1 go to the mono kernel"""
    ref = Ref(engine_lib, oracle_mod, MONO, 3, 5100)
    rng = np.random.default_rng(5100)
    lens = [[int(rng.integers(1, 4)) * NB + 32 * int(rng.integers(0, NB // 32)) for _ in range(3)] for _ in range(1 + N_CALLS)]
    lens[0][0] = 4 * NB - 32
    lens[10] = [0, 0, 0]
    lens[13][1] = 1
    lens[17][2] += 7                                                       # an odd length: no pair; the calls behind it pair again at an odd position
    for l in lens:
        ref.feed(l)
    assert ref.calls[13].nfr[1] == 0
    pair = lambda call: PAIR_KERNEL if all(L and L % 32 == 0 for L in call.lens) else MONO_KERNEL
    assert sum(pair(c) == PAIR_KERNEL for c in ref.calls) == 1 + N_CALLS - 3
    with Session(1) as ses:
        for drv in both_runs(engine_lib, ses, ref, pair, "the mono pair"):
            assert [k for k, _ in drv.names] == [k for k in range(1 + N_CALLS) if k != 10]
    ref.close()


# ---- 2. regrowth between enqueued calls ----

REGROW = {
    "cascade_scratch": CASCADE,
    "cascade_scratch_and_ys": INFLIGHT["cascade_dsd256_96k_ns"],
    "planar_copy": INFLIGHT["fp6_il2_no_coop"],
}
# the cascade sizes of tests/test_gpu_engine_buffers.py behind eight calls of the first size, and a call twice as long again; file 1 stays short
REGROW_LENS = [NB] * (1 + JOB_SLOTS) + [5 * NB, NB, 10 * NB, NB]


@pytest.mark.parametrize("case", list(REGROW))
def test_buffers_regrow_between_enqueued_calls(engine_lib, oracle_mod, case):
    """the scratch with its P carried stage-A samples (5120, then 10240 outputs outgrow the line), the f64 line next to it under 'N', the planar
    copy of an interleaved call five times longer than its predecessors: each regrows behind calls that are still pending, and the engine's
    own wait for its stream is all that protects the old buffer.  The proof of depth stands in front of the first regrowing call"""
    kw, kernel = REGROW[case]
    ref = Ref(engine_lib, oracle_mod, kw, 2, 5200 + list(REGROW).index(case))
    for k, L in enumerate(REGROW_LENS):
        ref.feed([L, NB // 2 + 100 * k])
    with Session(1) as ses:
        both_runs(engine_lib, ses, ref, kernel, case)
    ref.close()


# ---- 3. two streams ordered with events ----

def test_two_streams_ordered_with_events(engine_lib, oracle_mod):
    """calls alternate between two non-blocking streams; each, with its upload, waits for the event recorded behind the previous call on the
    other stream.  A regrowing call in the middle; d2d_peak right behind the last enqueue, which waits for last_stream alone"""
    import torch
    kw, kernel = CASCADE
    ref = Ref(engine_lib, oracle_mod, kw, 2, 5300)
    lens = ragged_lens(ref, 18, 5300, zero_at=None, noframe_at=None)
    lens[12][0] = 5 * NB + 333
    for l in lens:
        ref.feed(l)
    with Session(2) as ses:
        e = ses.engine(engine_lib, n_files=2, **ref.kw)
        drv = Driver(engine_lib, ses, e, ref, kernel)
        events = [torch.cuda.Event() for _ in ref.calls]
        s = ses.streams
        drv.enqueue(0, s[0])
        blocked = Blocker(s[0])
        t0 = time.perf_counter()
        prev = blocked.end
        for k in range(1, len(ref.calls)):
            if k == JOB_SLOTS + 1:
                still_pending([blocked], "two streams", (time.perf_counter() - t0) * 1e3)
            s[k % 2].wait_event(prev)
            drv.enqueue(k, s[k % 2])
            events[k].record(s[k % 2])
            prev = events[k]
        drv.check_peaks("two streams, right behind the last enqueue")
        for st in s:
            st.synchronize()
        drv.check("two streams")
    ref.close()


# ---- 4. reset and seek with work pending ----

def test_reset_with_work_pending(engine_lib, oracle_mod):
    """a cascade engine whose scratch call 0 has grown; eight calls pending; d2d_reset with no wait of the test's own, then at once the stream
    from byte 0 again on the non-blocking stream: the frames before the reset complete and correct, those behind it a fresh conversion's"""
    kw, kernel = CASCADE
    ref = Ref(engine_lib, oracle_mod, kw, 2, 5400)
    lens = ragged_lens(ref, 1 + JOB_SLOTS, 5400, first_longest=False)
    lens[0][0] = 5 * NB
    for l in lens:
        ref.feed(l)
    ref.reset()
    for l in lens:
        ref.feed(l)
    n = 1 + JOB_SLOTS
    for a, b in zip(ref.calls[:n], ref.calls[n:]):
        assert a.tell == b.tell and all(np.array_equal(x, y) for x, y in zip(a.want, b.want))
    with Session(1) as ses:
        both_runs(engine_lib, ses, ref, kernel, "reset", before={n: lambda e: e.reset()})
    ref.close()


def test_seek_with_work_pending(engine_lib, oracle_mod):
    """three files on a cascade engine; eight calls pending; d2d_seek of file 1 with no wait of the test's own, a prime of its halo (files 0 and 2
    feed nothing), then translate calls: file 1 is a fresh conversion's from the new position, files 0 and 2 carry on (unsynchronised:
    tests/test_gpu_timeslice.py has the same with a wait after each call)"""
    kw, kernel = CASCADE
    ref = Ref(engine_lib, oracle_mod, kw, 3, 5500)
    lens = ragged_lens(ref, 1 + JOB_SLOTS + 5, 5500, first_longest=False)
    lens[0][0] = 5 * NB
    n = 1 + JOB_SLOTS
    for l in lens[:n]:
        ref.feed(l)
    with Session(1) as ses:
        pre = ses.engine(engine_lib, **ref.kw).preroll_bytes()
        p = 300001
        q = p - pre
        assert 0 < pre <= NB and q > ref.at[1]
        ref.seek(1, q)
        ref.feed([0, pre, 0], prime=True)
        assert ref.calls[-1].tell[1] == (p, ref.F(p)) and ref.calls[-1].nfr == [0, 0, 0]
        for l in lens[n + 1:]:
            ref.feed(l)
        both_runs(engine_lib, ses, ref, kernel, "seek", before={n: lambda e: e.seek(q, file=1)})
    ref.close()


# ---- 5. engines interleaved from one thread ----

def test_engines_interleaved_from_one_thread(engine_lib, oracle_mod):
    """three engines, each on a stream of its own, call 0 and then 12 calls each, enqueued in turn with no wait: different engines are fully
    independent (include/dsd2dxd_amd.h)"""
    routes = ["fp6_m32_t24", "px_kind1_dsd64_96k", "cascade_dsd256_96k"]
    refs = []
    for i, r in enumerate(routes):
        ref = Ref(engine_lib, oracle_mod, ROUTES[r][0], 2, 5600 + i)
        for l in ragged_lens(ref, 13, 5600 + i):
            ref.feed(l)
        refs.append(ref)
    with Session(3) as ses:
        drivers = [Driver(engine_lib, ses, ses.engine(engine_lib, n_files=2, **ref.kw), ref, ROUTES[r][1]) for r, ref in zip(routes, refs)]
        for wait in (True, False):
            if not wait:                                    # (the control run has used the drivers: fresh ones for the run in flight)
                drivers = [Driver(engine_lib, ses, ses.engine(engine_lib, n_files=2, **ref.kw), ref, ROUTES[r][1]) for r, ref in zip(routes, refs)]
            for drv in drivers:
                drv.wait = wait
            for drv, st in zip(drivers, ses.streams):
                drv.enqueue(0, st)
            blocked = [] if wait else [Blocker(st, 3 * BLOCK_MS) for st in ses.streams]      # (three times the enqueues in front of the proof)
            t0 = time.perf_counter()
            for k in range(1, 13):
                if k == JOB_SLOTS + 1 and blocked:
                    still_pending(blocked, "three engines", (time.perf_counter() - t0) * 1e3)
                for drv, st in zip(drivers, ses.streams):
                    drv.enqueue(k, st)
            for st in ses.streams:
                st.synchronize()
            for r, drv in zip(routes, drivers):
                drv.check(f"three engines, {r}, {'a wait after each call' if wait else 'in flight'}")
    for ref in refs:
        ref.close()


# ---- 6. profiling brackets with calls pending ----

@pytest.mark.parametrize("route", ["fp6_m32_t24", "cascade_dsd256_96k"])
def test_profiling_brackets_with_calls_pending(engine_lib, oracle_mod, route):
    """d2d_profile_enable, then call 0 and 24 calls behind the blocker, one of them of 0 bytes (no FIR output: no bracket): the pool of event
    pairs grows while earlier brackets are open.  launches equals what the control engine reports for the same calls made one at a time"""
    kw, kernel = ROUTES[route]
    ref = Ref(engine_lib, oracle_mod, kw, 3, 5700)
    for lens in ragged_lens(ref, 1 + N_CALLS, 5700, zero_at=10):
        ref.feed(lens)
    reads = []
    with Session(1) as ses:
        stream = ses.streams[0]
        for wait in (True, False):
            e = ses.engine(engine_lib, n_files=3, **ref.kw)
            e.profile_enable(True)
            drv = Driver(engine_lib, ses, e, ref, kernel, wait=wait)
            label = f"profiling, {route}, {'a wait after each call' if wait else 'in flight'}"
            run(drv, stream, label)
            reads.append(e.profile_read_all())              # (waits for the brackets itself)
            stream.synchronize()
            drv.check(label)
            assert e.profile_read_all() == (0.0, 0.0, 0)
    (fir_w, step_w, n_w), (fir, step, n) = reads
    assert n == n_w == N_CALLS, reads                        # every call but the one of 0 bytes
    assert step >= fir > 0 and step_w >= fir_w > 0, reads
    ref.close()
