"""What tests/test_gpu_stream_order.py shares: the harness that holds one device call to the stream promises of include/qoi_mi355x.h on a
stream that does not synchronise with stream 0, and the names of the calls that take a stream, read from the header (no GPU needed for that).

The harness, for one Case (a call, the device buffers it reads, the guarded device buffers it writes and their expected bytes):
 1. warm: the call once to grow every arena and pinned buffer, then once more, fully synchronised, timed on the host and checked - so the
    checked call below does no hipMalloc / hipFree, which synchronise the device and would hide what is looked for;
 2. every buffer the call reads gets stale content that is valid input of the same sizes (pixels 0x5A; streams their true length, their
    header with the other colorspace byte, over a body of 0x5A - one-byte QOI_OP_DIFF chunks -; length arrays rotated by one place),
    every output 0xA5, guards included; the call is made once on them, synchronised: its answer must differ from the true one (else an
    early read could not be seen), and it is what the context's pinned result words hold from then on, not the true answer the warm
    calls left there;
 3. on the stream s, with no host wait: a delay block (plain tensor copies over 256 MiB, repeated), device-to-device copies that put the
    true inputs in place, an event `ready`;
 4. the call, on s;
 5. asynchronous calls: on s, at once, a copy of every whole output into a snapshot; s is synchronised; the snapshots are compared.
    synchronous calls: on return, the copies are made on a second non-blocking stream that never waited for s; only that one is
    synchronised;
 6. `ready.query()` is False immediately before the call, and for asynchronous calls immediately after it: a case that does not meet this
    FAILS (it is not a test otherwise).
The delay is sized by measurement: the block is timed with events, the warm calls on the host, and the block is repeated until its time
is at least ten times the longest warm call so far.  Correctness never depends on a time: other tenants only lengthen the delay."""
import os
import re
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT_FILL, STALE = 0xA5, 0x5A
GUARD = 64
BLOCK_BYTES = 256 << 20
MARGIN = 10                     # the delay is at least this many times the longest warm call
MIN_BLOCKS = 256                # about 25 ms: the least delay, whatever the warm calls took


def stream_taking_calls():
    """The functions of include/qoi_mi355x.h that have a `void *stream` parameter, among the prototypes of qoi_amd/abi.py."""
    from qoi_amd import abi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qoi_mi355x.h")).read(), flags=re.S)
    declared = re.findall(r"(?m)^[A-Za-z_0-9 ]+?[ \*]+(qoi_[a-z0-9_]+|qoimi_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", hdr)
    taking = {name for name, params in declared if any(" ".join(p.split()) == "void *stream" for p in params.split(","))}
    # every `void *stream` of the header stands in a prototype that was recognised: one the pattern missed would lack a case unnoticed
    assert len(re.findall(r"\bvoid\s*\*\s*stream\b", hdr)) == len(taking) and len(declared) == len(abi.PROTOTYPES)
    assert taking <= set(abi.PROTOTYPES), taking - set(abi.PROTOTYPES)
    return taking


def stale_stream(s):
    """The true length and end marker of stream s and its header with the other colorspace byte (valid; what reads the header early sees
    another one) over a body of one-byte QOI_OP_DIFF chunks"""
    s = bytes(s)
    assert len(s) >= 22 and s[13] in (0, 1)
    return s[:13] + bytes([s[13] ^ 1]) + bytes([STALE]) * (len(s) - 22) + s[-8:]


def u8(a):
    if isinstance(a, (bytes, bytearray)):
        return np.frombuffer(bytes(a), dtype=np.uint8).copy()
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()


def rotated(values):
    v = list(values)
    return v[1:] + v[:1]


class Inp:
    """A device buffer a call reads: `live` is what the call is given; `true` and `stale` are device copies prepared beforehand."""

    def __init__(self, true, stale=None):
        import torch
        true = u8(true)
        stale = np.full(true.size, STALE, dtype=np.uint8) if stale is None else u8(stale)
        assert stale.size == true.size and not np.array_equal(true, stale), "the stale form of an input must differ from the true one"
        self.true, self.stale = torch.from_numpy(true).cuda(), torch.from_numpy(stale).cuda()
        self.live = self.true.clone()

    @property
    def ptr(self):
        return self.live.data_ptr()


class Out:
    """A device buffer a call writes, 0xA5 everywhere with GUARD bytes in front and behind; pieces: (offset behind the front guard, bytes)
    of what the call must leave there - every other byte stays 0xA5."""

    def __init__(self, size, pieces):
        import torch
        self.size = int(size)
        self.want = np.full(self.size + 2 * GUARD, OUT_FILL, dtype=np.uint8)
        for off, data in pieces:
            data = u8(data)
            assert 0 <= off and off + data.size <= self.size, (off, data.size, self.size)
            self.want[GUARD + off:GUARD + off + data.size] = data
        self.buf = torch.full((self.want.size,), OUT_FILL, dtype=torch.uint8, device="cuda")
        self.snap = torch.empty_like(self.buf)
        assert self.buf.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return self.buf.data_ptr() + GUARD

    def differs(self):
        """None, or words for the first byte of the snapshot that is not the expected one"""
        got = self.snap.cpu().numpy()
        bad = np.flatnonzero(got != self.want)
        if not bad.size:
            return None
        k = int(bad[0])
        return f"{bad.size} bytes differ, the first at byte {k - GUARD} of {self.size} behind the front guard: {int(got[k]):#04x}, not {int(self.want[k]):#04x}"


def back_to_back(blobs, gap=3, elem=1):
    """(offsets, total) for blobs laid one behind the other with `gap` guard bytes (rounded up to whole elements) between them"""
    offs, pos = [], 0
    step = -(-gap // elem) * elem
    for b in blobs:
        offs.append(pos)
        pos += len(b) + step
    return offs, max(pos - step, 1)


class Case:
    """One call.  sync: the header calls it synchronous (it returns when its outputs are complete); else it only enqueues.
    call(handle) makes the call on the HIP stream `handle` and returns what the call gives the host; host_ok(result) asserts that."""

    def __init__(self, name, sync, inputs, outputs, call, host_ok=None):
        self.name, self.sync, self.inputs, self.outputs, self.call, self.host_ok = name, sync, inputs, outputs, call, host_ok or (lambda r: None)


class Harness:
    def __init__(self):
        import torch
        self.torch = torch
        self.s = torch.cuda.Stream()            # torch creates its streams with hipStreamNonBlocking: no implicit order with stream 0
        self.s2 = torch.cuda.Stream()           # the consumer of synchronous calls: it never waits for s
        self.a = torch.zeros(BLOCK_BYTES, dtype=torch.uint8, device="cuda")
        self.b = torch.empty_like(self.a)
        torch.cuda.synchronize()
        self.block_ms = min(self._time_blocks(4) / 4 for _ in range(3))
        self.longest_warm_ms, self.longest_warm_of = 0.0, None
        self.delay_ms_at_least = 0.0
        self.met = []                           # (case, blocks) of every checked call that met condition 6

    def _blocks(self, n):
        for _ in range(n):
            self.b.copy_(self.a)

    def _time_blocks(self, n):
        torch = self.torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(self.s):
            e0.record()
            self._blocks(n)
            e1.record()
        self.s.synchronize()
        return e0.elapsed_time(e1)

    def blocks(self):
        return max(MIN_BLOCKS, int(np.ceil(MARGIN * self.longest_warm_ms / self.block_ms)))

    def _reset(self, case, content):
        for i in case.inputs:
            i.live.copy_(getattr(i, content))
        for o in case.outputs:
            o.buf.fill_(OUT_FILL)
            o.snap.fill_(0)
        self.torch.cuda.synchronize()

    def _compare(self, case, result, what):
        for k, o in enumerate(case.outputs):
            d = o.differs()
            assert d is None, f"{case.name}, {what}: output {k}: {d}"
        case.host_ok(result)

    def warm(self, case):
        torch = self.torch
        self._reset(case, "true")
        case.call(self.s.cuda_stream)           # grows the arenas
        self.s.synchronize()
        self._reset(case, "true")
        t0 = time.perf_counter()
        result = case.call(self.s.cuda_stream)
        self.s.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        if ms > self.longest_warm_ms:
            self.longest_warm_ms, self.longest_warm_of = ms, case.name
        for o in case.outputs:
            o.snap.copy_(o.buf)
        torch.cuda.synchronize()
        self._compare(case, result, "the warm call")

    def on_stale_inputs(self, case, s):
        """The call on the stale inputs, synchronised: True if its outputs or host results differ from the true ones (a rejection counts)."""
        from qoi_amd.api import QoiError
        try:
            result = case.call(s.cuda_stream)
        except QoiError:
            s.synchronize()
            return True
        s.synchronize()
        for o in case.outputs:
            o.snap.copy_(o.buf)
        self.torch.cuda.synchronize()
        if any(o.differs() is not None for o in case.outputs):
            return True
        try:
            case.host_ok(result)
        except AssertionError:
            return True
        return False

    def checked(self, case, stream=None, after_stale=None):
        """steps 2 to 6 on `stream` (default: s); after_stale() is called between the call on the stale inputs and the delayed producer"""
        torch = self.torch
        s = self.s if stream is None else stream
        self._reset(case, "stale")
        if case.inputs:
            assert self.on_stale_inputs(case, s), f"{case.name}: the stale inputs give the true answer - an early read could not be seen"
            self._reset(case, "stale")
        if after_stale is not None:
            after_stale()
        n = self.blocks()
        ready = torch.cuda.Event()
        with torch.cuda.stream(s):
            self._blocks(n)
            for i in case.inputs:
                i.live.copy_(i.true)
            ready.record()
        before = ready.query()
        result = case.call(s.cuda_stream)
        after = ready.query()
        assert not before, f"{case.name}: not a test - the producer of the inputs had finished before the call was made ({n} delay blocks of {self.block_ms:.3f} ms)"
        if case.sync:
            with torch.cuda.stream(self.s2):
                for o in case.outputs:
                    o.snap.copy_(o.buf)
            self.s2.synchronize()
        else:
            with torch.cuda.stream(s):
                for o in case.outputs:
                    o.snap.copy_(o.buf)
            assert not after, f"{case.name}: not a test - the producer of the inputs had finished when the asynchronous call returned ({n} delay blocks of {self.block_ms:.3f} ms)"
            s.synchronize()
        self._compare(case, result, "the call behind the delayed producer")
        s.synchronize()
        self.delay_ms_at_least = max(self.delay_ms_at_least, n * self.block_ms)
        self.met.append((case.name, n))
        return result

    def run(self, case):
        self.warm(case)
        return self.checked(case)
