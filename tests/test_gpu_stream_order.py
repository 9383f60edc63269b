"""Every device call that takes a stream, held to the three stream promises of include/qoi_mi355x.h on a NON-BLOCKING stream (-m gpu):
asynchronous calls enqueue on `stream` and nothing else orders them; synchronous calls return when every output byte is written; work and
calls that follow a synchronous call are ordered behind it, on whichever stream they come.

torch.cuda.Stream() creates its streams non-blocking (hipStreamNonBlocking): unlike the legacy default stream the other GPU modules pass,
they have no implicit order with stream 0.  tests/stream_order.py states the harness: a warm call, stale but valid inputs, a delayed
producer on the stream that puts the true inputs in place, the call, and a consumer that reads the whole guarded outputs - on the same
stream at once for an asynchronous call, on a second non-blocking stream that never waited for an asynchronous call's stream for a
synchronous one.  A call that read early gives the clean wrong answer of the stale inputs (asserted per case: the call is made on them
once, synchronised, and must differ; that also leaves the stale answer, not the true one, in the context's pinned result words); a call
that returned early leaves 0xA5 or stale results.  The calls through bounded staging (the gathers, verify, statistics, the seek index)
gather the stream headers and wait for the stream before they launch anything else: what they read behind the delay is the headers
alone - the stale ones carry the other colorspace byte, which such a call rejects or flags - and the promise held for the rest of
their work is the synchronous return.  Every case FAILS unless the producer was still running when the call was made (and, asynchronous calls, when it returned).

Every expectation is an existing definition - the oracle for streams and pixels, the models of qoi_amd/ for everything else - and every
comparison is exact over the whole output and its guards.  CASES maps every stream-taking function of the header to its cases;
test_every_stream_taking_call_has_a_case (no GPU) compares its keys with the header."""
import os

import numpy as np
import pytest

import cases as stream_cases
from qoi_amd import bilinear, crops, resize, tensors, thumbs, tiles, warp
from qoi_amd import pixelstats as ps
from qoi_amd import seekindex as si
from qoi_amd import streaminfo, synth
from qoi_amd.imagediff import DIFF_DTYPE, DIFF_PIXELS, diff
from qoi_amd.packplan import plan as pack_plan
from stream_order import Case, Harness, Inp, Out, back_to_back, rotated, stale_stream, stream_taking_calls, u8
from gpu_pack import IMAGENET
from gpu_pack import api, oracle  # noqa: F401  (fixtures)
from model_cases import pack_offsets

gpu = pytest.mark.gpu
SHAPES = [(160, 120, 4), (97, 61, 3), (130, 70, 4), (64, 48, 3)]
KINDS = ["photo", "noise", "sprite_alpha", "uiflat"]
INTERVALS = [4, 8, 8, 6]
FILL = 0xFF804020
CASES = {}                      # function of the header -> the names of the tests that hold it to the promises
_TESTS = {}


def case(*calls):
    """registers a case function(W) under the functions of the header it makes through the harness"""
    def register(fn):
        name = fn.__name__
        for c in calls:
            CASES.setdefault("qoimi_" + c, []).append(name)
        _TESTS[name] = fn
        return fn
    return register


def image(kind, w, h, ch, frame=0):
    if kind == "noise":
        return np.random.default_rng(w * 7919 + h * 31 + ch + frame).integers(0, 256, size=w * h * ch, dtype=np.uint8)
    return (synth.frame_rgba if ch == 4 else synth.frame_rgb)(kind, w, h, frame).reshape(-1).copy()


class World:
    """One context, the harness, and a pack of four images of mixed shapes and channel counts with the oracle's streams and decodes
    (computed once, never changed)."""

    def __init__(self, api, oracle, ctx=None):
        self.api, self.oracle, self.ctx, self.H = api, oracle, ctx or api.Context(0), Harness()
        self.px = [image(k, w, h, ch, i) for i, ((w, h, ch), k) in enumerate(zip(SHAPES, KINDS))]
        self.streams = [oracle.encode(p, w, h, ch) for p, (w, h, ch) in zip(self.px, SHAPES)]
        self.sizes = [len(s) for s in self.streams]
        self.descs = [api.QoiDesc(w, h, ch, 0) for w, h, ch in SHAPES]
        self.bounds = [api.encode_bound(w, h, ch) for w, h, ch in SHAPES]
        self.so, self.pack_bytes = self.lay(self.streams, front=1)
        self.pack_true, self.pack_stale = self.blob(self.streams, self.so, self.pack_bytes), self.blob([stale_stream(s) for s in self.streams], self.so, self.pack_bytes)
        self.po, self.px_bytes = self.lay(self.px, front=0, gap=1)
        self._D = {}
        self.points = [si.points(s, w, h, K, self.D(i, 4)) for i, (s, (w, h, _), K) in enumerate(zip(self.streams, SHAPES, INTERVALS))]
        self.firsts = [int(x) for x in np.cumsum([0] + [len(p) for p in self.points[:-1]])]
        self.all_points = np.concatenate(self.points)
        self.index = (INTERVALS, self.all_points, self.firsts)
        assert all(len(p) for p in self.points)

    @staticmethod
    def lay(blobs, front=0, gap=3):
        offs, total = back_to_back(blobs, gap)
        return [front + o for o in offs], front + total + 8

    @staticmethod
    def blob(blobs, offs, total, fill=0xEE):
        a = np.full(total, fill, dtype=np.uint8)
        for o, b in zip(offs, blobs):
            a[o:o + len(b)] = u8(b)
        return a

    def D(self, i, och):
        if (i, och) not in self._D:
            w, h, _ = SHAPES[i]
            d = self.oracle.decode(self.streams[i], och)[0].reshape(h, w, och)
            d.setflags(write=False)
            self._D[(i, och)] = d
        return self._D[(i, och)]

    def pack_inp(self):
        return Inp(self.pack_true, self.pack_stale)

    def pixels_inp(self):
        return Inp(self.blob(self.px, self.po, self.px_bytes), None)


@pytest.fixture(scope="module")
def W(api, oracle):
    w = World(api, oracle)
    yield w
    print(f"\nstream order: one delay block of 256 MiB {w.H.block_ms:.3f} ms; the longest warm call {w.H.longest_warm_ms:.3f} ms ({w.H.longest_warm_of}); "
          f"the longest delay at least {w.H.delay_ms_at_least:.1f} ms; {len(w.H.met)} checked calls met their condition")
    w.ctx.close()


# ------------------------------------------------------------------ encode
def strided(W, n, ch=4, w=160, h=120, kinds=("photo", "noise", "sprite_alpha", "uiflat", "constant")):
    """n equally shaped images a stride apart, the oracle's streams, and the pieces of the two outputs of qoimi_encode_batch"""
    px = [image(kinds[i % len(kinds)], w, h, ch, 40 + i) for i in range(n)]
    want = [W.oracle.encode(p, w, h, ch) for p in px]
    bound = W.api.encode_bound(w, h, ch)
    ps_, ss = w * h * ch + 5, bound + 3
    pix = np.full(n * ps_, 0xEE, dtype=np.uint8)
    for i, p in enumerate(px):
        pix[i * ps_:i * ps_ + p.size] = p
    return dict(px=px, want=want, lens=[len(s) for s in want], desc=W.api.QoiDesc(w, h, ch, 0), n=n, pixel_stride=ps_, stream_stride=ss, pix=pix, bound=bound)


def encode_batch_case(W, n, ctx=None):
    b = strided(W, n)
    ctx = ctx or W.ctx
    inp = Inp(b["pix"])
    streams = Out(n * b["stream_stride"], [(i * b["stream_stride"], s) for i, s in enumerate(b["want"])])
    lens = Out(4 * n, [(0, np.array(b["lens"], dtype=np.int32))])
    return Case(f"encode_batch n={n}", False, [inp], [streams, lens],
                lambda st: ctx.encode_batch(inp.ptr, b["pixel_stride"], b["desc"], n, streams.ptr, b["stream_stride"], lens.ptr, st))


@case("encode_batch", "encode_status")
def encode_batch_one_image_twice(W):
    """n = 1: tree placement; the two prezero regions in turn - between the first checked call and the second stand encode_status and the
    harness's own call on the stale inputs, every one the very next user of the workspace, so each skips its memset and runs on the
    region its predecessor's first launch zeroed"""
    c = encode_batch_case(W, 1)
    W.H.run(c)
    W.ctx.encode_status(W.H.s.cuda_stream)
    W.H.checked(c)
    W.ctx.encode_status(W.H.s.cuda_stream)
    assert W.ctx.encode_retries() == 0


@case("encode_batch", "encode_status")
def encode_batch_three_images(W):
    """tree placement by ticket"""
    W.H.run(encode_batch_case(W, 3))
    W.ctx.encode_status(W.H.s.cuda_stream)
    assert W.ctx.encode_retries() == 0


@case("encode_batch", "encode_status")
def encode_batch_nine_images(W):
    """look-back placement"""
    W.H.run(encode_batch_case(W, 9))
    W.ctx.encode_status(W.H.s.cuda_stream)
    assert W.ctx.encode_retries() == 0


@case("encode_batch", "encode_status")
def encode_batch_beside_a_self_test_repeat(W):
    """A context whose LDS-order self-test is repeated at every encode call (the interval at its smallest, through QOIMI_TUNING): every
    call of the case enqueues a repeat on the context's own stream and polls the one before.  The repeat of the checked call is in flight
    when the call is MADE and returns; it has finished long before the call's kernels run behind the delay, so it is the host side - the
    poll, the pinned word, the launch on the other stream - that stands beside the caller's stream here, not the device work.  That the
    repeats ran and passed shows only in what stays 0: a failed one makes the next qoimi_encode_status fail and counts suspect calls."""
    assert os.environ.get("QOIMI_TUNING") == "1"
    os.environ["QOIMI_ENC_RECHECK_EVERY"] = "1"
    try:
        ctx = W.api.Context(0)
    finally:
        del os.environ["QOIMI_ENC_RECHECK_EVERY"]
    try:
        W.H.run(encode_batch_case(W, 3, ctx))
        ctx.encode_status(W.H.s.cuda_stream)
        assert ctx.encode_retries() == 0 and ctx.encode_suspect_calls() == 0
    finally:
        ctx.close()


def mixed_outputs(W):
    so, total = W.lay([b"\0" * b for b in W.bounds], front=1)
    return so, Out(total, list(zip(so, W.streams))), Out(4 * len(SHAPES), [(0, np.array(W.sizes, dtype=np.int32))])


@case("encode_images", "encode_status")
def encode_images_mixed_channels_twice(W):
    """3- and 4-channel images in one call: two channel groups, two error words, the image tables through pinned staging (the call waits
    for the event behind the previous call's tables: after the synchronised warm call that is no wait)"""
    inp = W.pixels_inp()
    so, streams, lens = mixed_outputs(W)
    c = Case("encode_images", False, [inp], [streams, lens], lambda st: W.ctx.encode_images(inp.ptr, W.po, W.descs, streams.ptr, so, lens.ptr, st))
    W.H.run(c)
    W.ctx.encode_status(W.H.s.cuda_stream)
    W.H.checked(c)
    W.ctx.encode_status(W.H.s.cuda_stream)
    assert W.ctx.encode_retries() == 0


def packed_outputs(lens, streams, align):
    off = pack_offsets(lens, align)
    n = len(lens)
    return off, [Out(int(off[-1]), [(int(off[i]), s) for i, s in enumerate(streams)]), Out(8 * (n + 1), [(0, off)]), Out(4 * n, [(0, np.array(lens, dtype=np.int32))])]


def tables_ok(off, lens):
    def ok(result):
        assert np.array_equal(result[0], off) and result[1].tolist() == list(lens), (result[0], off, result[1], lens)
    return ok


@case("encode_packed")
def encode_packed_in_sub_batches(W):
    b = strided(W, 3)
    inp = Inp(b["pix"])
    off, outs = packed_outputs(b["lens"], b["want"], 4)
    staging = (b["bound"] + 255) // 256 * 256          # one slot: a sub-batch per image
    assert len(pack_plan([b["bound"]] * 3, staging)) == 3
    W.H.run(Case("encode_packed", True, [inp], outs,
                 lambda st: W.ctx.encode_packed(inp.ptr, b["pixel_stride"], b["desc"], 3, 4, outs[0].ptr, int(off[-1]), outs[1].ptr, outs[2].ptr, staging, st),
                 tables_ok(off, b["lens"])))


@case("encode_images_packed")
def encode_images_packed_in_sub_batches(W):
    inp = W.pixels_inp()
    off, outs = packed_outputs(W.sizes, W.streams, 1)
    staging = max(W.bounds) + 256
    assert len(pack_plan(W.bounds, staging)) >= 2
    W.H.run(Case("encode_images_packed", True, [inp], outs,
                 lambda st: W.ctx.encode_images_packed(inp.ptr, W.po, W.descs, 1, outs[0].ptr, int(off[-1]), outs[1].ptr, outs[2].ptr, staging, st),
                 tables_ok(off, W.sizes)))


TILES = [(0, 0, 0, 160, 120, 2, 0), (2, 3, 5, 120, 64, 3, 1), (1, 1, 2, 90, 51, 1, 2), (3, 0, 0, 64, 48, 4, 3)]


@case("encode_tiles")
def encode_tiles_in_sub_batches(W):
    inp = W.pixels_inp()
    images = [p.reshape(h, w, ch) for p, (w, h, ch) in zip(W.px, SHAPES)]
    px = [tiles.tile(images[t[0]], t, 0, tiles.PLAIN) for t in TILES]
    want = [W.oracle.encode(p.reshape(-1), p.shape[1], p.shape[0], p.shape[2]) for p in px]
    lens = [len(s) for s in want]
    off, outs = packed_outputs(lens, want, 1)
    slots = tiles.plan(SHAPES, TILES, 0, 0)[0]
    staging = max(slots)
    subs = tiles.plan(SHAPES, TILES, 0, staging)[1]
    assert len(subs) >= 2

    def ok(result):
        tables_ok(off, lens)(result[:2])
        assert [(d.width, d.height, d.channels) for d in result[2]] == [(p.shape[1], p.shape[0], p.shape[2]) for p in px]
        assert W.ctx.tile_stats()[0] == len(subs)

    W.H.run(Case("encode_tiles", True, [inp], outs,
                 lambda st: W.ctx.encode_tiles(inp.ptr, W.po, W.descs, 0, TILES, tiles.PLAIN, 1, outs[0].ptr, int(off[-1]), outs[1].ptr, outs[2].ptr, staging, st), ok))


TENSOR_SHAPES = [(160, 120, 4), (97, 61, 3), (130, 70, 4)]


@case("encode_tiles")
def encode_tiles_tensors(W):
    """a tensor call: launch_tensor_ingest stands on another branch of the launch line than the byte call's kernels.  f16 CHW tensors in a
    sub-batch each; the stale inputs are other elements, which convert to other bytes"""
    flags = tiles.source_flags(tiles.F16, tiles.CHW, tiles.UNIT)
    rng = np.random.default_rng(77)
    true, stale = ([rng.uniform(-0.25, 1.25, size=(ch, h, w)).astype(np.float16) for w, h, ch in TENSOR_SHAPES] for _ in range(2))
    ts = [(0, 0, 0, 160, 120, 1, flags), (1, 1, 2, 90, 51, 1, flags | 2), (2, 3, 5, 120, 64, 1, flags | 1), (1, 0, 0, 97, 61, 1, flags | 3)]
    px = [tiles.tile(true[t[0]], t, 0) for t in ts]
    assert all(not np.array_equal(tiles.tile(stale[t[0]], t, 0), p) for t, p in zip(ts, px))
    want = [W.oracle.encode(p.reshape(-1), p.shape[1], p.shape[0], p.shape[2]) for p in px]
    lens = [len(s) for s in want]
    po, total = W.lay([u8(a) for a in true], front=0, gap=2)
    assert all(o % 2 == 0 for o in po)
    inp = Inp(W.blob([u8(a) for a in true], po, total), W.blob([u8(a) for a in stale], po, total))
    off, outs = packed_outputs(lens, want, 1)
    descs = [W.api.QoiDesc(w, h, ch, 0) for w, h, ch in TENSOR_SHAPES]
    staging = max(tiles.plan(TENSOR_SHAPES, ts, 0, 0)[0])
    subs = tiles.plan(TENSOR_SHAPES, ts, 0, staging)[1]
    assert len(subs) >= 2

    def ok(result):
        tables_ok(off, lens)(result[:2])
        assert [(d.width, d.height, d.channels) for d in result[2]] == [(p.shape[1], p.shape[0], p.shape[2]) for p in px]
        assert W.ctx.tile_stats()[:2] == (len(subs), len(subs))

    W.H.run(Case("encode_tiles, tensors", True, [inp], outs,
                 lambda st: W.ctx.encode_tiles(inp.ptr, po, descs, 0, ts, tiles.PLAIN, 1, outs[0].ptr, int(off[-1]), outs[1].ptr, outs[2].ptr, staging, st), ok))


# ------------------------------------------------------------------ decode
def decode_case(W, name, streams, shapes, och, batch):
    """qoimi_decode_batch (streams a stride apart) or qoimi_decode_images (a pack at odd offsets, images back to back)"""
    want = [W.oracle.decode(s, och)[0] for s in streams]
    descs = [W.api.QoiDesc(w, h, ch, 0) for w, h, ch in shapes]
    sizes = [len(s) for s in streams]
    if batch:
        ss, ps_ = max(sizes) + 11, max(x.size for x in want) + 7
        so, po = [i * ss for i in range(len(streams))], [i * ps_ for i in range(len(streams))]
        total_s, total_p = len(streams) * ss, len(streams) * ps_
    else:
        so, total_s = World.lay(streams, front=1)
        po, total_p = World.lay(want, front=0, gap=1)
    inp = Inp(World.blob(streams, so, total_s), World.blob([stale_stream(s) for s in streams], so, total_s))
    out = Out(total_p, list(zip(po, want)))
    if batch:
        call = lambda st: W.ctx.decode_batch(inp.ptr, ss, sizes, descs, och, out.ptr, ps_, st)      # noqa: E731
    else:
        call = lambda st: W.ctx.decode_images(inp.ptr, so, sizes, descs, och, out.ptr, po, st)      # noqa: E731
    return Case(name, True, [inp], [out], call)


def six_noise(W):
    px = [image("noise", 160, 120, 4, 70 + i) for i in range(6)]
    return [W.oracle.encode(p, 160, 120, 4) for p in px], [(160, 120, 4)] * 6


@case("decode_batch")
def decode_batch_one_image(W):
    """the return on pinned result words while the last launch retires"""
    W.H.run(decode_case(W, "decode_batch n=1", W.streams[:1], SHAPES[:1], 4, True))


@case("decode_images")
def decode_images_one_image(W):
    W.H.run(decode_case(W, "decode_images n=1", W.streams[2:3], SHAPES[2:3], 3, False))


@case("decode_batch")
def decode_batch_six_images(W):
    W.H.run(decode_case(W, "decode_batch n=6", W.streams + W.streams[:2], SHAPES + SHAPES[:2], 4, True))


@case("decode_images")
def decode_images_six_images(W):
    W.H.run(decode_case(W, "decode_images n=6", W.streams + W.streams[:2], SHAPES + SHAPES[:2], 4, False))


@case("decode_images")
def decode_images_in_sub_batches(W):
    """a record cap of 1 MiB takes about 258 KB of streams per sub-batch (qoi_host_decode.hip: cap / 4 - cap / 256): six noise streams of
    96 KB run as three.  The library has no counter of decode sub-batches; the plan is restated here from its formula."""
    streams, shapes = six_noise(W)
    cap_stream = (1 << 20) // 4 - (1 << 20) // 4 // 64
    assert 2 * max(len(s) for s in streams) <= cap_stream < 3 * min(len(s) for s in streams)
    ctx, shared = W.api.Context(0), W.ctx            # a context of its own: the cap the shared one was created with is not touched
    ctx.set_decode_record_cap(1 << 20)
    W.ctx = ctx
    try:
        W.H.run(decode_case(W, "decode_images, record cap", streams, shapes, 4, False))
    finally:
        W.ctx = shared
        ctx.close()


@case("decode_images")
def decode_images_flat_beside_photograph(W):
    """the class split: a flat image (run descriptors) beside a photograph"""
    name, flat, w, h = next(x for x in stream_cases.flat_run_streams() if x[0] == "flat_seed1_exact")
    W.H.run(decode_case(W, "decode_images, flat + photo", [flat, W.streams[0]], [(w, h, 4), SHAPES[0]], 4, False))


@case("decode_batch")
def decode_batch_hostile_stream(W):
    """a stream whose INDEX chunks defeat the speculation: the repair rounds read their progress back through a pinned word"""
    name, s, w, h = next(x for x in stream_cases.pair_streams() if x[0] == "pairs_seed5")
    W.H.run(decode_case(W, "decode_batch, hostile", [s], [(w, h, 4)], 4, True))
    assert W.ctx.decode_stats()["rounds"] >= 2, W.ctx.decode_stats()


# ------------------------------------------------------------------ pack, descriptors, inspect, compare, verify, hash, synth
def strided_streams(W):
    """the pack's four streams a stride apart, and their lengths on the device: (streams, lengths) as inputs with their stale forms"""
    ss = max(W.bounds) + 5
    so = [i * ss for i in range(len(W.streams))]
    true, stale = World.blob(W.streams, so, len(so) * ss), World.blob([stale_stream(s) for s in W.streams], so, len(so) * ss)
    return ss, so, Inp(true, stale), Inp(np.array(W.sizes, dtype=np.int32), np.array(rotated(W.sizes), dtype=np.int32))


@case("pack_streams")
def pack_streams_aligned(W):
    ss, so, streams, lens = strided_streams(W)
    off = pack_offsets(W.sizes, 4)
    packed, d_off = Out(int(off[-1]), [(int(off[i]), s) for i, s in enumerate(W.streams)]), Out(8 * 5, [(0, off)])
    W.H.run(Case("pack_streams", False, [streams, lens], [packed, d_off],
                 lambda st: W.ctx.pack_streams(streams.ptr, ss, lens.ptr, 4, 4, packed.ptr, int(off[-1]), d_off.ptr, st)))


@case("hash_streams")
def hash_streams_of_four(W):
    ss, so, streams, lens = strided_streams(W)
    out = Out(8 * 4, [(0, np.array([synth.stream_hash64(s) for s in W.streams], dtype=np.uint64))])
    assert len({synth.stream_hash64(stale_stream(s)[:n]) for s, n in zip(W.streams, rotated(W.sizes))} & {synth.stream_hash64(s) for s in W.streams}) == 0
    W.H.run(Case("hash_streams", False, [streams, lens], [out], lambda st: W.ctx.hash_streams(streams.ptr, ss, lens.ptr, 4, out.ptr, st)))


@case("synth_frames")
def synth_frames_three(W):
    w, h, stride = 97, 61, 97 * 61 * 4 + 12
    out = Out(3 * stride, [(i * stride, synth.frame_rgba("photo", w, h, 5 + i)) for i in range(3)])
    W.H.run(Case("synth_frames", False, [], [out], lambda st: W.ctx.synth_frames(synth.KIND_ID["photo"], synth.DEFAULT_SEED, 5, 3, w, h, out.ptr, stride, st)))


@case("read_descs")
def read_descs_of_the_pack(W):
    inp = W.pack_inp()

    def ok(result):
        descs, bad = result
        assert bad is None and [(d.width, d.height, d.channels, d.colorspace) for d in descs] == [(w, h, ch, 0) for w, h, ch in SHAPES]

    W.H.run(Case("read_descs", True, [inp], [], lambda st: W.ctx.read_descs(inp.ptr, W.so, W.sizes, st), ok))


@case("inspect_streams")
def inspect_streams_of_the_pack(W):
    inp = W.pack_inp()
    want = [streaminfo.info_record(streaminfo.inspect_stream(s)) for s in W.streams]
    assert all(streaminfo.info_record(streaminfo.inspect_stream(stale_stream(s))) != x for s, x in zip(W.streams, want))

    def ok(result):
        infos, first = result
        assert first is None and all(infos[i] == want[i] for i in range(len(want))), (infos, want)

    W.H.run(Case("inspect_streams", True, [inp], [], lambda st: W.ctx.inspect_streams(inp.ptr, W.so, W.sizes, st), ok))


def diffs_of(a, b, shapes, ca, cb):
    out, first = np.zeros(len(a), dtype=DIFF_DTYPE), -1
    for i, (x, y, (w, h)) in enumerate(zip(a, b, shapes)):
        m, f, want, got = diff(x, y, w * h, ca[i], cb[i])
        out[i] = (m, f, want, got, DIFF_PIXELS if m else 0, 0)
        if m and first < 0:
            first = i
    return out, first


def planted(W):
    """the pack's pixels with two bytes of image 2 changed"""
    px = [p.copy() for p in W.px]
    px[2][1001] ^= 0x10
    px[2][-3] ^= 0x01
    return px


def diffs_ok(want, want_first):
    def ok(result):
        got, first = result
        assert first == want_first and all(got[i] == want[i] for i in range(len(want))), (first, want_first, got, want)
    return ok


@case("compare_images")
def compare_images_with_a_planted_difference(W):
    """side A the pack's pixels, side B the same with two bytes changed; the stale sides are equal (0x5A both): no difference"""
    a, b = W.pixels_inp(), Inp(World.blob(planted(W), W.po, W.px_bytes), None)
    chs = [ch for _, _, ch in SHAPES]
    want, first = diffs_of(W.px, planted(W), [(w, h) for w, h, _ in SHAPES], chs, chs)
    assert first == 2 and int(want[2]["mismatched"]) == 2
    W.H.run(Case("compare_images", True, [a, b], [], lambda st: W.ctx.compare_images(a.ptr, W.po, 0, b.ptr, W.po, 0, W.descs, st), diffs_ok(want, first)))


@case("verify_images")
def verify_images_with_a_planted_difference(W):
    px, pack = Inp(World.blob(planted(W), W.po, W.px_bytes), None), W.pack_inp()
    chs = [ch for _, _, ch in SHAPES]
    want, first = diffs_of(planted(W), [W.D(i, ch).reshape(-1) for i, ch in enumerate(chs)], [(w, h) for w, h, _ in SHAPES], chs, chs)
    assert first == 2 and int(want[2]["mismatched"]) == 2
    staging = max(W.px[i].size for i in range(4)) + 256           # sub-batches of one or two images
    W.H.run(Case("verify_images", True, [px, pack], [], lambda st: W.ctx.verify_images(px.ptr, W.po, W.descs, pack.ptr, W.so, W.sizes, staging, st),
                 diffs_ok(want, first)))


# ------------------------------------------------------------------ the gather family
CROPS = [(0, 5, 17, 101, 50, 1), (1, 0, 9, 37, 20, 2), (2, 8, 13, 33, 30, 3), (3, 0, 30, 64, 18, 0)]
ITEMS = [(0, 8, 17, 120, 90, 43, 23, 1), (1, 0, 9, 90, 40, 50, 40, 2), (2, 3, 13, 100, 50, 40, 30, 3), (3, 0, 0, 64, 48, 9, 5, 0)]
FACTORS = [3, 2, 5, 4]
MAPS = [(0, (20, 17, 100, 50), (33, 18), 30.0, 0.3), (1, (3, 9, 30, 20), (17, 16), 30.0, 0.5), (2, (0, 13, 64, 35), (41, 29), -20.0, 0.4)]
assert all(it[2] >= INTERVALS[it[0]] for it in CROPS[:3] + ITEMS[:3]) and all(m[1][1] >= INTERVALS[m[0]] for m in MAPS)   # (indexed: below a seek row)


def warps(flags, projective=False):
    out = []
    for i, rect, size, degrees, scale in MAPS:
        if projective:
            cw, rh = rect[2:]
            m, gh, _ = warp.perspective((cw, rh), size, [(0.1 * cw, 0.05 * rh), (0.9 * cw, 0.15 * rh), (0.85 * cw, 0.9 * rh), (0.05 * cw, 0.8 * rh)])
            out.append(warp.item(i, rect, size, m, flags, FILL, proj=gh))
        else:
            out.append(warp.item(i, rect, size, warp.rotation(rect[2:], size, degrees, scale), flags, FILL))
    return out


def warped(W, it, och, mode):
    _, x, y, cw, rh, ow, oh, flags, a, b, d, e, fill, reserved, c, f = it
    return warp.warp(W.D(it[0], 4), (x, y, cw, rh), (ow, oh), (a, b, c, d, e, f), flags, fill, mode, och=och, reserved=reserved)


def gather(W, name, want, call, elem=1, staging=0, stats=None):
    """one gather call over the pack: outputs back to back with 3 guard bytes (in whole elements) between them; call(pack, out, offsets,
    staging, stream); staging: one that splits the call into sub-batches; stats: the counters function whose [0] says how many ran"""
    inp = W.pack_inp()
    want = [u8(x) for x in want]
    oo, total = back_to_back(want, 3, elem)
    out = Out(total, list(zip(oo, want)))

    def ok(result):
        if stats is not None and staging:
            assert getattr(W.ctx, stats)()[0] >= 2, (name, getattr(W.ctx, stats)())

    return Case(name, True, [inp], [out], lambda st: call(inp.ptr, out.ptr, oo, staging, st), ok)


STAGING = 1                     # raised to one slot: a sub-batch per referenced image


@case("decode_thumbnails")
def decode_thumbnails_of_the_pack(W):
    want = [thumbs.thumbnail(W.D(i, 4), f, thumbs.ALPHA_WEIGHTED) for i, f in enumerate(FACTORS)]
    W.H.run(gather(W, "decode_thumbnails", want, lambda p, o, oo, sb, st: W.ctx.decode_thumbnails(p, W.so, W.sizes, W.descs, 4, FACTORS, thumbs.ALPHA_WEIGHTED, o, oo, sb, st),
                   staging=STAGING, stats="thumbnail_stats"))


def crops_case(W, index=None):
    want = [crops.crop(W.D(c[0], 3), c[1:5], c[5]) for c in CROPS]
    if index is None:
        return gather(W, "decode_crops", want, lambda p, o, oo, sb, st: W.ctx.decode_crops(p, W.so, W.sizes, W.descs, 3, CROPS, o, oo, sb, st), staging=STAGING, stats="crop_stats")
    return gather(W, "decode_crops_indexed", want, lambda p, o, oo, sb, st: W.ctx.decode_crops_indexed(p, W.so, W.sizes, W.descs, 3, CROPS, o, oo, *index, sb, st))


@case("decode_crops")
def decode_crops_of_the_pack(W):
    W.H.run(crops_case(W))


@case("decode_crops_indexed")
def decode_crops_indexed_of_the_pack(W):
    W.H.run(crops_case(W, W.index))
    assert W.ctx.seek_stats()[1] == len({c[0] for c in CROPS})


def resampled_case(W, kind, index=None):
    f = {"resized": resize.resize, "bilinear": bilinear.bilinear}[kind]
    want = [f(W.D(it[0], 4), it[1:5], it[5:7], it[7], resize.ALPHA_WEIGHTED) for it in ITEMS]
    method = getattr(W.ctx, "decode_" + kind + ("_indexed" if index else ""))
    return gather(W, method.__name__, want, lambda p, o, oo, sb, st: method(p, W.so, W.sizes, W.descs, 4, ITEMS, resize.ALPHA_WEIGHTED, o, oo, *(index or ()), sb, st),
                  staging=0 if index else STAGING, stats=None if index else kind.replace("resized", "resize") + "_stats")


@case("decode_resized")
def decode_resized_of_the_pack(W):
    W.H.run(resampled_case(W, "resized"))


@case("decode_bilinear")
def decode_bilinear_of_the_pack(W):
    W.H.run(resampled_case(W, "bilinear"))


@case("decode_resized_indexed")
def decode_resized_indexed_of_the_pack(W):
    W.H.run(resampled_case(W, "resized", W.index))


@case("decode_bilinear_indexed")
def decode_bilinear_indexed_of_the_pack(W):
    W.H.run(resampled_case(W, "bilinear", W.index))


WARP_FLAGS = {"bilinear": 0, "nearest": warp.NEAREST, "bicubic": warp.BICUBIC, "reflect": warp.REFLECT, "super2": warp.SUPER2, "vote2": warp.VOTE2, "projective": 0}


def warped_case(W, sampling, index=None):
    """one flag per kernel of the warp family: each is a launch site of its own"""
    items = warps(WARP_FLAGS[sampling], sampling == "projective")
    want = [warped(W, it, 4, warp.PLAIN) for it in items]
    method = W.ctx.decode_warped_indexed if index else W.ctx.decode_warped
    return gather(W, f"{method.__name__}, {sampling}", want, lambda p, o, oo, sb, st: method(p, W.so, W.sizes, W.descs, 4, items, warp.PLAIN, o, oo, *(index or ()), sb, st),
                  staging=0 if index else STAGING, stats=None if index else "warp_stats")


@case("decode_warped")
def decode_warped_bilinear(W):
    W.H.run(warped_case(W, "bilinear"))


@case("decode_warped")
def decode_warped_nearest(W):
    W.H.run(warped_case(W, "nearest"))


@case("decode_warped")
def decode_warped_bicubic(W):
    W.H.run(warped_case(W, "bicubic"))


@case("decode_warped")
def decode_warped_reflect(W):
    W.H.run(warped_case(W, "reflect"))


@case("decode_warped")
def decode_warped_super2(W):
    W.H.run(warped_case(W, "super2"))


@case("decode_warped")
def decode_warped_vote2(W):
    W.H.run(warped_case(W, "vote2"))


@case("decode_warped")
def decode_warped_projective(W):
    W.H.run(warped_case(W, "projective"))


@case("decode_warped_indexed")
def decode_warped_indexed_of_the_pack(W):
    W.H.run(warped_case(W, "bilinear", W.index))


FILTER_FORMATS = {"area": (tensors.FILTER_AREA, tensors.F32, tensors.CHW), "bicubic": (tensors.FILTER_BICUBIC, tensors.F16, tensors.HWC),
                  "lanczos": (tensors.FILTER_LANCZOS, tensors.BF16, tensors.CHW), "nearest": (tensors.FILTER_NEAREST, tensors.I64, tensors.HW),
                  "mode": (tensors.FILTER_MODE, tensors.I32, tensors.CHW)}


def tensors_case(W, name):
    filt, dtype, layout = FILTER_FORMATS[name]
    f = tensors.fmt(dtype, layout) if dtype in (tensors.U8, tensors.I32, tensors.I64) else (dtype, layout, *IMAGENET)
    want = [tensors.tensors(W.D(it[0], 4), it[1:5], it[5:7], it[7], filt, tensors.PLAIN, f) for it in ITEMS]
    return gather(W, "decode_tensors, " + name, want, lambda p, o, oo, sb, st: W.ctx.decode_tensors(p, W.so, W.sizes, W.descs, 4, ITEMS, filt, tensors.PLAIN, f, o, oo, sb, st),
                  elem=tensors.elem(dtype), staging=STAGING, stats="tensor_stats")


@case("decode_tensors")
def decode_tensors_area(W):
    W.H.run(tensors_case(W, "area"))


@case("decode_tensors")
def decode_tensors_bicubic(W):
    W.H.run(tensors_case(W, "bicubic"))


@case("decode_tensors")
def decode_tensors_lanczos(W):
    W.H.run(tensors_case(W, "lanczos"))


@case("decode_tensors")
def decode_tensors_nearest(W):
    W.H.run(tensors_case(W, "nearest"))


@case("decode_tensors")
def decode_tensors_mode(W):
    W.H.run(tensors_case(W, "mode"))


@case("decode_warped_tensors")
def decode_warped_tensors_f16(W):
    items, f = warps(0), (tensors.F16, tensors.CHW, *IMAGENET)
    want = [tensors.convert(warped(W, it, 4, warp.ALPHA_WEIGHTED), f) for it in items]
    W.H.run(gather(W, "decode_warped_tensors", want, lambda p, o, oo, sb, st: W.ctx.decode_warped_tensors(p, W.so, W.sizes, W.descs, 4, items, warp.ALPHA_WEIGHTED, f, o, oo, sb, st),
                   elem=2, staging=STAGING, stats="tensor_stats"))


# ------------------------------------------------------------------ pixel statistics
def pixel_stats_case(W, index=None):
    inp = W.pack_inp()
    want = [ps.stats(W.D(r[0], 4), r) for r in CROPS]
    hist = Out(4096 * len(CROPS), [(4096 * j, ps.hist(W.D(r[0], 4), r)) for j, r in enumerate(CROPS)])

    def ok(result):
        assert [ps.of_struct(s) for s in result] == want

    if index:
        return Case("pixel_stats_indexed", True, [inp], [hist], lambda st: W.ctx.pixel_stats_indexed(inp.ptr, W.so, W.sizes, W.descs, CROPS, *index, hist.ptr, 0, st), ok)
    return Case("pixel_stats", True, [inp], [hist], lambda st: W.ctx.pixel_stats(inp.ptr, W.so, W.sizes, W.descs, CROPS, hist.ptr, STAGING, st), ok)


@case("pixel_stats")
def pixel_stats_with_histograms(W):
    """the histograms are zeroed by a memset of the call's"""
    W.H.run(pixel_stats_case(W))
    assert W.ctx.pixel_stats_counters()[0] >= 2


@case("pixel_stats_indexed")
def pixel_stats_indexed_with_histograms(W):
    W.H.run(pixel_stats_case(W, W.index))


# ------------------------------------------------------------------ the seek index
def points_ok(W):
    def ok(result):
        points, firsts = result
        assert firsts == W.firsts and points.tobytes() == W.all_points.tobytes()
    return ok


@case("build_seek_index")
def build_seek_index_of_the_pack(W):
    inp = W.pack_inp()
    W.H.run(Case("build_seek_index", True, [inp], [], lambda st: W.ctx.build_seek_index(inp.ptr, W.so, W.sizes, W.descs, INTERVALS, STAGING, st), points_ok(W)))


@case("seek_index_from_pixels")
def seek_index_from_pixels_of_the_pack(W):
    px, pack = W.pixels_inp(), W.pack_inp()
    assert all(si.points_from_pixels(s, w, h, K, p, ch).tobytes() == pts.tobytes() for s, (w, h, ch), K, p, pts in zip(W.streams, SHAPES, INTERVALS, W.px, W.points))
    W.H.run(Case("seek_index_from_pixels", True, [px, pack], [], lambda st: W.ctx.seek_index_from_pixels(px.ptr, W.po, pack.ptr, W.so, W.sizes, W.descs, INTERVALS, st),
                 points_ok(W)))


@case("make_band_streams")
def make_band_streams_of_the_pack(W):
    inp = W.pack_inp()
    bands = [(0, 0, 4), (0, 40, 80), (1, 8, 1), (2, 32, 38), (3, 6, 12)]
    want = [si.band_stream(W.streams[i], SHAPES[i][0], SHAPES[i][1], SHAPES[i][2], 0, INTERVALS[i], W.points[i], first, rows) for i, first, rows in bands]
    blobs = [s for s, _ in want]
    oo, total = back_to_back(blobs, 3)
    out = Out(total, list(zip(oo, blobs)))

    def ok(infos):
        for (i, first, rows), (s, pad), info in zip(bands, want, infos):
            assert (info.size, info.pad_rows, info.desc.width, info.desc.height, info.desc.channels) == (len(s), pad, SHAPES[i][0], pad + rows, SHAPES[i][2])

    W.H.run(Case("make_band_streams", True, [inp], [out], lambda st: W.ctx.make_band_streams(inp.ptr, W.so, W.sizes, W.descs, *W.index, bands, out.ptr, oo, st), ok))


# ------------------------------------------------------------------ the tests
@gpu
@pytest.mark.parametrize("name", list(_TESTS))
def test_stream_order(W, name):
    _TESTS[name](W)


@gpu
def test_one_context_across_streams(W):
    """The staged family on one context - crops, tensors, pixel_stats, decode_images of one image, crops - in turn on two non-blocking
    streams and stream 0, 30 calls with no wait on the caller's side between them: every result exact (the context orders a call behind
    the tail of its predecessor on another stream by itself).  Outputs are read on a stream that never waited for the call's."""
    import torch
    H = W.H
    family = [crops_case(W), tensors_case(W, "area"), pixel_stats_case(W), decode_case(W, "decode_images n=1", W.streams[:1], SHAPES[:1], 4, False), crops_case(W)]
    for c in family:
        H.warm(c)
    streams = [torch.cuda.Stream(), torch.cuda.Stream(), None]
    for c in family:
        for i in c.inputs:
            i.live.copy_(i.true)
    torch.cuda.synchronize()
    for it in range(30):
        c, st = family[it % len(family)], streams[it % 3]
        result = c.call(st.cuda_stream if st is not None else 0)
        with torch.cuda.stream(H.s2):
            for o in c.outputs:
                o.snap.copy_(o.buf)
            for o in c.outputs:
                o.buf.fill_(0xA5)
        H.s2.synchronize()
        H._compare(c, result, f"call {it} of the alternation")


@gpu
def test_encode_batch_across_streams(W):
    """qoimi_encode_batch on s1, qoimi_encode_status(s1), qoimi_encode_batch on s2: the rule the header states for the asynchronous
    encoder - both results exact, no retry"""
    import torch
    H = W.H
    a, b = encode_batch_case(W, 3), encode_batch_case(W, 1)
    H.warm(a)
    H.warm(b)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    before = W.ctx.encode_retries()
    H.checked(a, s1)
    W.ctx.encode_status(s1.cuda_stream)
    H.checked(b, s2)
    W.ctx.encode_status(s2.cuda_stream)
    assert W.ctx.encode_retries() == before == 0


PROFILED = {"encode": lambda W: encode_batch_case(W, 9), "decode": lambda W: decode_case(W, "decode_batch n=6", W.streams + W.streams[:2], SHAPES + SHAPES[:2], 4, True),
            "gather": lambda W: crops_case(W)}


@gpu
@pytest.mark.parametrize("family", list(PROFILED))
def test_stream_order_with_profiling(W, family):
    """The same harness with the per-kernel timers on (events on the caller's stream around every launch): the results are exact, and the
    profile taken behind the checked call - the counts are reset right in front of its delayed producer - holds the launches of that one
    call.  Encode, nine images of mixed content: look-back placement in two passes, so one `enc_slabs`, one `enc_slabs_generic` and one
    `encode_total`, nothing else (qoi_encode.hip: launch_encode).  Decode and crops: kernels of the decoder alone (the gather kernels have
    no timer), every round one `dec_fill` and one `decode_total`, at least one round per sub-batch."""
    c = PROFILED[family](W)
    st = W.H.s.cuda_stream
    try:
        W.ctx.set_profiling(True)
        W.H.warm(c)                                 # (grows what the timers need as well)
        if not c.sync:
            W.ctx.encode_status(st)
        W.H.checked(c, after_stale=lambda: (W.ctx.get_profile(st), W.ctx.set_profiling(True)))      # (folds what stands, resets the counts)
        if not c.sync:
            W.ctx.encode_status(st)
        prof = W.ctx.get_profile(st)
    finally:
        W.ctx.set_profiling(False)
    counts = {k: v[1] for k, v in prof.items() if v[1]}
    print(family, counts)
    if family == "encode":
        assert counts == {"enc_slabs": 1, "enc_slabs_generic": 1, "encode_total": 1}, counts
    else:
        subs = W.ctx.crop_stats()[0] if family == "gather" else 1
        assert subs == (len({c[0] for c in CROPS}) if family == "gather" else 1)
        assert all(k.startswith("dec_") or k == "decode_total" for k in counts), counts
        assert counts["decode_total"] == counts["dec_fill"] >= subs, (counts, subs)


CASES.setdefault("qoimi_get_profile", []).append("test_stream_order_with_profiling")


def test_every_stream_taking_call_has_a_case():
    """(no GPU) the functions of the header with a `void *stream` parameter are exactly the keys of CASES: a call added later without a
    stream-order case fails here"""
    taking = stream_taking_calls()
    assert len(taking) >= 30 and "qoimi_decode_crops_indexed" in taking and "qoimi_ctx_create" not in taking
    assert taking == set(CASES), (sorted(taking - set(CASES)), sorted(set(CASES) - taking))
    assert all(names for names in CASES.values())
