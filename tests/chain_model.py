"""A plain model of the batch transcoder's run-up (dec_transcode's look-back synchronisation) and the streams
built against it - no GPU, no kernel text.  A chunk's length is a function of its first byte (qoi.h:547-575), so parse chains that
meet stay together: a lane starts five chains on five consecutive bytes `back` bytes in front of its segment (64, and once more
192 bytes back when they have not met) - or ONE chain from byte 14 where the stream's first chunk is in reach - and takes their
common continuation as the stream's chain.  The model walks the same chains and gives a verdict that is conservative in both
directions, so that it never depends on how a kernel treats a tie at the segment start:

    meets   all five chains share a position at least 16 bytes in front of the segment
    apart   at least two chains enter the segment at different positions
    unsure  anything else (the tests never count it)

tests/test_chain_model.py checks the model against the reference decoder and certifies, on the CPU, what every stream of
tests/test_gpu_line_reader_hostile.py is built to reach; the cases of that module are assembled here so that both see the same."""
import math
import struct

import numpy as np
from model_cases import line_stream as _stream, line_walk as _walk


HEADER = 14
TRAILER = 8
SYNC_BYTES = 64            # the first run-up of segments of 1 KiB and above
RETRY_BYTES = 192          # the second one
MARGIN = 16                # "meets": a common position at least this far in front of the segment
WAVE = 64                  # a wavefront covers 64 consecutive segments of a call
RETRY_PERIOD = 121         # 24 five-byte chunks and a one-byte chunk

_LEN = np.ones(256, dtype=np.int64)
_LEN[0x80:0xC0] = 2
_LEN[0xFE] = 4
_LEN[0xFF] = 5
_PIX = np.ones(256, dtype=np.int64)
_PIX[0xC0:0xFE] = np.arange(1, 63)


def len_of(tag):
    """a chunk's length from its first byte (qoi.h:547-575)"""
    return 4 if tag == 0xFE else 5 if tag == 0xFF else 2 if (tag >> 6) == 2 else 1


def pixels_of(tag):
    """the pixels a chunk leaves (qoi.h:573-575: a run of 1..62)"""
    return (tag & 0x3F) + 1 if (tag >> 6) == 3 and tag < 0xFE else 1


def entry(body, start, base):
    """the first chain position at or after `base`, walking from `start` (positions count from the stream's first byte)"""
    p = start
    while p < base:
        p += len_of(body[p])
    return p


def walk(stream, stop=None):
    """the stream's own chain from byte 14: (chunk starts below `stop`, the position it lands on, the pixels of those chunks);
    `stop` defaults to the end marker's first byte"""
    stop = len(stream) - TRAILER if stop is None else stop
    lens = _LEN[np.frombuffer(stream, dtype=np.uint8)].tolist()
    starts = []
    p = HEADER
    while p < stop:
        starts.append(p)
        p += lens[p]
    tags = np.frombuffer(stream, dtype=np.uint8)[np.asarray(starts, dtype=np.int64)] if starts else np.zeros(0, dtype=np.uint8)
    return starts, p, int(_PIX[tags].sum())


def n_segments(stream, B):
    return (len(stream) - HEADER - TRAILER + B - 1) // B


def verdict(stream, base, back):
    """'meets' / 'apart' / 'unsure' for the segment that starts at `base` and a run-up of `back` bytes"""
    t0 = max(HEADER, base - back)
    if t0 == HEADER:
        return "meets"                                    # one chain from the stream's first chunk: nothing to meet
    seen, ends = [], []
    for s in range(t0, t0 + 5):
        at = set()
        p = s
        while p < base:
            at.add(p)
            p += len_of(stream[p])
        seen.append(at)
        ends.append(p)
    common = set.intersection(*seen)
    if common and min(common) <= base - MARGIN:
        return "meets"
    if len(set(ends)) > 1:
        return "apart"
    return "unsure"


def verdicts(stream, B):
    """per segment: (verdict at 64 bytes, verdict at 192 bytes)"""
    return [(verdict(stream, HEADER + j * B, SYNC_BYTES), verdict(stream, HEADER + j * B, RETRY_BYTES)) for j in range(n_segments(stream, B))]


def count_apart(stream, B):
    """segments certain to fail both run-ups (apart at 64 AND at 192 bytes), and the segments apart at 192 bytes"""
    v = verdicts(stream, B)
    return sum(1 for a, b in v if a == "apart" and b == "apart"), sum(1 for _, b in v if b == "apart")


def wave_images(nsegs):
    """how many images have segments in each wavefront of a call whose images have `nsegs` segments (64 consecutive ones per wavefront)"""
    owner = np.repeat(np.arange(len(nsegs)), nsegs)
    return [len(set(owner[k:k + WAVE].tolist())) for k in range(0, len(owner), WAVE)]


def sub_batches(lens, B, cap_mb=1):
    """the sub-batches of a call under a record cap (the rule of decode_offsets: stream bytes plus B per image against cap / 4 - cap / 256)"""
    cap = (cap_mb << 20) // 4 - (cap_mb << 20) // 256
    out, n, acc = [], 0, 0
    for ln in lens:
        if n > 0 and acc + ln + B > cap:
            out.append(n)
            n, acc = 0, 0
        acc += ln + B
        n += 1
    out.append(n)
    return out


def repeats_for_sub_batches(lens, B, want=3):
    """how often a call's streams are listed so that it splits into `want` sub-batches or more under a 1 MiB record cap"""
    rep = 1
    while len(sub_batches(list(lens) * rep, B)) < want:
        rep += 1
    return rep


def phase_stride(streams):
    """the stride of the phase case: the longest stream rounded up to 16, plus one - odd, as the straddle test of test_transcode_line_fetch.py"""
    return (max(len(s) for s in streams) + 15) // 16 * 16 + 1


# ---------------------------------------------------------------------------------------------------------------------------------
# streams.  An item is (stream, width, height); every builder is deterministic.
# ---------------------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def _sprite(w, h, seed):
    """opaque blobs with alpha steps on a transparent ground, short runs only (the stream stays far from the flat rule)"""
    rng = np.random.default_rng(seed)
    px = _walk(w, h, seed).reshape(h, w, 4)
    a = np.full((h, w), 255, dtype=np.uint8)
    for y in range(h):
        x0 = int(rng.integers(0, w - 24))
        a[y, x0:x0 + int(rng.integers(4, 20))] = 0
        x1 = int(rng.integers(0, w - 8))
        a[y, x1:x1 + 6] = rng.choice(np.array([64, 128, 192], dtype=np.uint8))
    px[:, :, 3] = a
    px[a == 0] = 0
    return px.reshape(-1, 4)


def clean(oracle, B, nseg, seed=0, sprite=False):
    """an encoder-made stream of exactly `nseg` segments of B bytes: the first rows of a 64-pixel wide photograph-like walk (or sprite)"""
    key = ("clean", B, nseg, seed, sprite)
    if key not in _CACHE:
        w, hmax = 64, (nseg * B) // 64 + 8                # a row never takes less than 64 / 62 + 1 bytes ... nor this many rows
        px = _sprite(w, hmax, 7000 + seed) if sprite else _walk(w, hmax, 5000 + seed)
        lo, hi = 1, hmax
        while lo < hi:                                    # the smallest height that reaches nseg segments (a row adds less than a segment)
            mid = (lo + hi) // 2
            if n_segments(oracle.encode(px[:w * mid], w, mid, 4), B) >= nseg:
                hi = mid
            else:
                lo = mid + 1
        s = oracle.encode(px[:w * lo], w, lo, 4)
        assert n_segments(s, B) == nseg, (B, nseg, seed, n_segments(s, B))
        _CACHE[key] = (s, w, lo)
    return _CACHE[key]


def retry(B, nseg, seed=0):
    """QOI_OP_RGBA chunks with a one-byte chunk every 25th (period 121 bytes).  An ordinary chunk is FF x FF y FF with one-byte x, y:
    chains on its bytes 0, 2 and 4 each go on five bytes at a time and never meet.  The first chunk behind the one-byte chunk is
    FF FE z (luma tag) w: the chains that the one-byte chunk shifted to its bytes 1 and 3 leave it at its end, where the stream's own
    chain stands.  So a run-up meets only across such a place: 64 bytes often hold none, 192 bytes always do."""
    key = ("retry", B, nseg, seed)
    if key not in _CACHE:
        rng = np.random.default_rng(9000 + seed)
        nbytes = (nseg - 1) * B + B // 2 + 1 + 2 * seed % 97
        groups = nbytes // RETRY_PERIOD + 3
        g = np.empty((groups, RETRY_PERIOD), dtype=np.uint8)
        ch = g[:, :120].reshape(groups, 24, 5)
        ch[:, :, 0] = 0xFF
        ch[:, :, 2] = 0xFF
        ch[:, :, 4] = 0xFF
        ch[:, :, 1] = rng.integers(0, 0x80, (groups, 24))           # one-byte chunks as colour bytes (INDEX / DIFF)
        ch[:, :, 3] = rng.integers(0xC0, 0xFE, (groups, 24))         # ... and QOI_OP_RUN
        ch[:, 0, 1] = 0xFE
        ch[:, 0, 2] = rng.integers(0, 0x80, groups)
        ch[:, 0, 3] = rng.integers(0x80, 0xC0, groups)
        ch[:, 0, 4] = rng.integers(0x40, 0x80, groups)
        d = rng.integers(0x40, 0x80, groups)
        d[d == 0x6A] = 0x6B
        g[:, 120] = d
        phase = (5 * seed) % RETRY_PERIOD // 5 * 5                    # start on a chunk of the period that differs from stream to stream
        body = g.reshape(-1)[phase:]
        body = bytes(body[:entry(bytes(body[:nbytes + 8]), 0, nbytes)])
        s = _stream(1, 1, body)
        npx = walk(s)[2]
        s = _stream(npx, 1, body)
        assert n_segments(s, B) == nseg, (B, nseg, seed, n_segments(s, B))
        _CACHE[key] = (s, npx, 1)
    return _CACHE[key]


def never(nbytes=60 * 1024):
    """the stream of test_small_calls_adapt_to_the_previous_call (QOI_OP_RGBA chunks whose alpha byte reads as a QOI_OP_RGBA tag: five
    chains that never meet, whatever the run-up) at `nbytes`"""
    key = ("never", nbytes)
    if key not in _CACHE:
        n = (nbytes - HEADER - TRAILER) // 5
        i = np.arange(n)
        body = np.stack([np.full(n, 0xFF), (i * 7) & 0xFF, np.full(n, 0xFF), (i * 13) & 0xFF, np.full(n, 0xFF)], axis=1).astype(np.uint8).tobytes()
        _CACHE[key] = (_stream(n, 1, body), n, 1)
    return _CACHE[key]


def rgba_literal(n, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (n, 5), dtype=np.uint8)
    a[:, 0] = 0xFF
    return a.tobytes()


def by_pixels(body, extra=0):
    """a stream whose header asks for the pixels its chunks leave, and `extra` more (the last pixel repeats there, qoi.h:544), one row"""
    npx = walk(_stream(1, 1, body))[2] + extra
    return _stream(npx, 1, body), npx, 1


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_line_reader_hostile.py.  A case is a list of (kind, item); kind 'c' clean, 'r' retry, 'h' never meeting ...
# ---------------------------------------------------------------------------------------------------------------------------------
RETRY_LAYOUT = [("c", 18), ("r", 21), ("c", 18), ("r", 21), ("c", 18), ("r", 22), ("c", 18), ("r", 21), ("c", 18), ("r", 21), ("c", 19), ("r", 22), ("c", 19)]
# (the 60 KiB stream is 60 / 30 / 15 segments: at 1 KiB a wavefront holds three images only where it begins on the wavefront's lanes 1 .. 3)
NEVER_LAYOUT = {
    1024: [("c", 10), ("c", 28), ("c", 28), ("h", 60), ("c", 22), ("c", 23), ("c", 23), ("h", 60), ("c", 22), ("c", 22), ("c", 22)],
    2048: [("c", 17), ("h", 30), ("c", 17), ("h", 30), ("c", 17), ("c", 17)],
    4096: [("c", 14), ("h", 15), ("c", 14), ("h", 15), ("c", 14), ("h", 15), ("c", 14), ("h", 15), ("c", 12)],
}
MIXED_LAYOUT = {
    1024: [("c", 10), ("r", 28), ("c", 28), ("h", 60), ("r", 22), ("c", 23), ("r", 23), ("h", 60), ("c", 22), ("r", 22), ("c", 22)],
    2048: [("c", 17), ("h", 30), ("r", 17), ("h", 30), ("c", 17), ("r", 17)],
    4096: [("c", 14), ("h", 15), ("r", 14), ("h", 15), ("c", 14), ("h", 15), ("r", 14), ("h", 15), ("c", 12)],
}


def assemble(oracle, B, layout):
    """the (kind, item) list of a layout of (kind, segments): every stream of a call its own (seeds count up), sprites among the clean ones"""
    out = []
    for k, (kind, nseg) in enumerate(layout):
        if kind == "c":
            item = clean(oracle, B, nseg, seed=k, sprite=(k % 4 == 2))
        elif kind == "r":
            item = retry(B, nseg, seed=k)
        else:
            item = never()
            assert n_segments(item[0], B) == nseg
        out.append((kind, item))
    return out


def retry_case(oracle, B):
    return assemble(oracle, B, RETRY_LAYOUT)


def never_case(oracle, B):
    return assemble(oracle, B, NEVER_LAYOUT[B])


def mixed_case(oracle, B):
    return assemble(oracle, B, MIXED_LAYOUT[B])


def phase_case(oracle, B):
    """every chunk length at every phase: streams of 3000 chunks each (kind 'p', the same for every segment size), and clean streams
    behind them that fill the call's last wavefront"""
    case = list(_phase_streams())
    fill = -sum(n_segments(it[0], B) for _, it in case) % WAVE
    for k, p in enumerate(_pads(fill) if fill >= 20 else []):
        case.append(("c", clean(oracle, B, p, seed=400 + k)))
    return case


def _phase_streams():
    if "phase" in _CACHE:
        return _CACHE["phase"]
    rng = np.random.default_rng(77)
    n = 3000
    one = lambda: bytes([0x40 | int(rng.integers(0, 64))])                                     # noqa: E731
    rgb = lambda: bytes([0xFE]) + rng.integers(0, 256, 3, dtype=np.uint8).tobytes()           # noqa: E731
    rgba = lambda: bytes([0xFF]) + rng.integers(0, 256, 4, dtype=np.uint8).tobytes()          # noqa: E731
    luma = lambda: bytes([0x80 | int(rng.integers(0, 64)), int(rng.integers(0, 256))])        # noqa: E731
    bodies = []
    for k in range(4):                                     # QOI_OP_RGB only, behind 0 .. 3 one-byte chunks: the four phases mod 4
        bodies.append(b"".join([one() for _ in range(k)] + [rgb() for _ in range(n - k)]))
    for k in range(8):                                     # RGB, LUMA, RGBA, DIFF: 12 bytes, behind 0 .. 7 one-byte chunks (two segment ends at 4 KiB: 4 and 8 mod 12)
        bodies.append(b"".join([one() for _ in range(k)] + [(rgb, luma, rgba, one)[i % 4]() for i in range(n - k)]))
    body = bytearray()                                     # INDEX and short runs between RGBA chunks
    for i in range(n):
        r = i % 7
        body += rgba() if r in (0, 2, 3, 5) else bytes([int(rng.integers(0, 64))]) if r in (1, 6) else bytes([0xC0 | int(rng.integers(0, 3))])
    bodies.append(bytes(body))
    noise = rng.integers(0, 256, 12000, dtype=np.uint8).tobytes()                              # uniform random bytes: 3000 chunks of them
    starts = walk(_stream(1, 1, noise + bytes(8)))[0]
    bodies.append(noise[:starts[n] - HEADER])
    # (the order in the call: with the RGB streams on the places 1 .. 4 of an odd stride from byte 1 their chunks begin on even addresses too)
    bodies = bodies[13:] + bodies[:4] + bodies[12:13] + bodies[4:12]
    case = [("p", by_pixels(b)) for b in bodies]
    for _, (s, _, _) in case:
        assert len(walk(s)[0]) == n
    _CACHE["phase"] = case
    return case


def straddles(streams, addrs, B):
    """{(chunk length, distance)} over the streams' own chains: a chunk that begins `distance` bytes in front of a 128-byte line end
    (the stream's first byte at address addrs[i]) - and the same in front of a segment end"""
    line, seg = set(), set()
    for s, a in zip(streams, addrs):
        arr = np.frombuffer(s, dtype=np.uint8)
        st = np.asarray(walk(s)[0], dtype=np.int64)
        ln = _LEN[arr[st]]
        dl = (-(st + a)) % 128                            # bytes from the chunk's first byte to the next line end
        ds = (HEADER - st) % B                            # ... to the next segment end
        ds[ds == 0] = B
        dl[dl == 0] = 128
        line |= {(int(x), int(d)) for x, d in zip(ln[dl < ln], dl[dl < ln])}
        inside = (ds < ln) & (st + ds < len(s) - TRAILER)  # (a segment end inside the stream: a lane begins there)
        seg |= {(int(x), int(d)) for x, d in zip(ln[inside], ds[inside])}
    return line, seg


ALL_STRADDLES = {(ln, d) for ln in (2, 4, 5) for d in range(1, ln)}

END_LANES = {"last": 63, "middle": 31, "first": 0}


def _pads(total):
    k = max(2, math.ceil(total / 24))
    return [total // k + (1 if i < total % k else 0) for i in range(k)]


def ends_case(oracle, B, where):
    """stream ends between clean neighbours: kinds 'x1' .. 'x4' (a clean stream cut after the first 1 .. 4 bytes of a QOI_OP_RGBA chunk),
    'xl' (after the first byte of a QOI_OP_LUMA chunk), 'xa' (another image's chunks behind the last pixel), 'xs' (chunks for 3 % of the
    pixels).  The clean streams in front of each are sized so that the segment with the cut - for 'xa' the one with the last pixel -
    is the wavefront's lane END_LANES[where].  Returns (case, [(index, segment of the cut)])"""
    key = ("ends", B, where)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng(31)
    specials = []
    partial = {"x1": [0xFF], "x2": [0xFF, 0x11], "x3": [0xFF, 0x11, 0x22], "x4": [0xFF, 0x11, 0x22, 0x33], "xl": [0xA5]}
    for k, (kind, part) in enumerate(partial.items()):
        nseg = 10 + k % 3
        s, w, h = clean(oracle, B, nseg + 1, seed=100 + k, sprite=(k == 2))
        starts = walk(s)[0]
        cut = max(p for p in starts if p <= HEADER + (nseg - 1) * B + B // 2 + 7 * k)
        item = by_pixels(s[HEADER:cut] + bytes(part), extra=5)
        assert n_segments(item[0], B) == nseg
        specials.append((kind, item, nseg - 1))
    a, aw, ah = clean(oracle, B, 9, seed=120)
    b, _, _ = clean(oracle, B, 8, seed=121, sprite=True)
    xa = _stream(aw, ah, a[HEADER:-TRAILER] + b[HEADER:-TRAILER])
    specials.append(("xa", (xa, aw, ah), (len(a) - TRAILER - 1 - HEADER) // B))
    nseg = 10
    nch = ((nseg - 1) * B + B // 2) // 5
    body = rgba_literal(nch, int(rng.integers(1 << 30)))
    npx = math.ceil(nch / 0.03)
    specials.append(("xs", (_stream(npx, 1, body), npx, 1), nseg - 1))
    lane = END_LANES[where]
    case, cuts, G, nclean = [], [], 0, 0
    for kind, item, crit in specials:
        pad = (lane - crit - G) % WAVE
        pad += WAVE if pad < 20 else 0
        for p in _pads(pad):
            case.append(("c", clean(oracle, B, p, seed=200 + nclean % 3, sprite=(nclean % 5 == 3))))
            nclean += 1
        G += pad
        cuts.append((len(case), crit))
        case.append((kind, item))
        G += n_segments(item[0], B)
    fill = -G % WAVE
    if fill:
        fill += WAVE if fill < 20 else 0
        for p in _pads(fill):
            case.append(("c", clean(oracle, B, p, seed=200 + nclean % 3)))
            nclean += 1
    _CACHE[key] = (case, cuts)
    return _CACHE[key]


def overlap_pair(oracle, B):
    """a long stream whose chunk bytes hold a whole short stream, header and end marker included: (long item, short item, offset of the
    short one inside the long one).  Any bytes are chunks (qoi.h:544-575), so both are streams the reference decoder accepts."""
    key = ("overlap", B)
    if key not in _CACHE:
        short = clean(oracle, B, 8, seed=300)
        front = retry(B, 6, seed=41)[0][HEADER:-TRAILER]
        back = rgba_literal((5 * B + B // 2) // 5, 43)
        s, w, h = by_pixels(front + short[0] + back)
        _CACHE[key] = ((s, w, h), short, HEADER + len(front))
    return _CACHE[key]
