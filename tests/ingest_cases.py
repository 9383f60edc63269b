"""What the tests of tensor sources of qoimi_encode_tiles share (the kernel tensor_ingest, qoi_amd/csrc/qoi_ingest_core.h): the inputs, built
once and never changed, and the lists of the GPU cases - tensors, placements, tiles, channel counts - which tests/test_gpu_ingest_values.py,
tests/test_gpu_ingest.py and tests/test_gpu_offsets_wide.py run and tests/test_ingest_paths.py replays on the CPU through the host build
of the item arithmetic, so that the certificate of the branches reached and the runs cannot drift apart.  No GPU is needed to import this.

The witnesses.  SYMMETRIC is t = fl(fl(x * 127.5) + 127.5): two roundings.  A build that contracts it to one fused multiply-add computes
fl(x * 127.5 + 127.5).  For binary16 and bfloat16 elements the product is exact and both agree; binary32 elements next to a tie of the
byte can tell them apart.  `f32_witnesses` finds them in exact rational arithmetic (fractions), with a round-to-binary32 written here:
neither the model qoi_amd/tiles.py nor numpy's float arithmetic takes part in the search."""
import functools
from fractions import Fraction

import numpy as np

from qoi_amd import tiles

RANGES = (tiles.UNIT, tiles.SYMMETRIC, tiles.BYTES)
FLOATS = (tiles.F16, tiles.BF16, tiles.F32)
FORMATS = [(d, l, r) for d in (tiles.U8, tiles.F16, tiles.BF16, tiles.F32) for l in (tiles.HWC, tiles.CHW)
           for r in ((tiles.UNIT,) if d == tiles.U8 else RANGES)]
SHAPES = [(1, 1), (5, 3), (37, 23), (70, 9), (300, 17)]
NEIGHBOURS = 9                  # binary32 neighbours searched on either side of every tie


# ------------------------------------------------------------------ exact arithmetic
def _rne(q):
    """the integer nearest to the rational q >= 0, ties to even"""
    n = q.numerator // q.denominator
    r = q - n
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and n % 2):
        n += 1
    return n


def _rn32(q):
    """the rational q rounded to binary32, to nearest, ties to even (|q| < 2^128; subnormals included)"""
    if q == 0:
        return Fraction(0)
    a = abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    assert Fraction(2) ** e <= a < Fraction(2) ** (e + 1) and e < 128
    ulp = Fraction(2) ** (max(e, -126) - 23)
    r = _rne(a / ulp) * ulp
    return r if q > 0 else -r


def _byte(t):
    return 0 if t <= 0 else 255 if t >= 255 else _rne(t)


@functools.lru_cache(maxsize=None)
def f32_witnesses():
    """(x float32[n], two uint8[n], fused uint8[n]): the binary32 elements among the NEIGHBOURS neighbours on either side of each
    (k + 0.5 - 127.5) / 127.5, k = 0..254, whose SYMMETRIC byte differs between two roundings and one"""
    xs, two, fused, seen = [], [], [], set()
    half = Fraction(255, 2)
    for k in range(255):
        c = np.float32((k + 0.5 - 127.5) / 127.5)
        near, up, down = [c], c, c
        for _ in range(NEIGHBOURS):
            up, down = np.nextafter(up, np.float32(2)), np.nextafter(down, np.float32(-2))
            near += [up, down]
        for x in near:
            bits = int(np.float32(x).view(np.uint32))
            if bits in seen:
                continue
            seen.add(bits)
            X = Fraction(float(x))                                     # (a binary32 is a binary64 is a rational: exact)
            b2, b1 = _byte(_rn32(_rn32(X * half) + half)), _byte(_rn32(X * half + half))
            if b1 != b2:
                xs.append(x)
                two.append(b2)
                fused.append(b1)
    out = np.array(xs, np.float32), np.array(two, np.uint8), np.array(fused, np.uint8)
    for a in out:
        a.setflags(write=False)
    return out


# ------------------------------------------------------------------ the patterns
F32_W = 80


@functools.lru_cache(maxsize=None)
def f32_patterns():
    """float32[h, 80, 4]: the set of test_float_patterns of tests/test_ingest_core_host.py - every tie of the three ranges with both
    neighbours, both clamps, the specials, both signs of the smallest subnormal, the smallest normal -, the witnesses, 20000 random bit
    patterns and as many more as fill the last row"""
    r = np.random.default_rng(5)
    t = (np.arange(-2, 258, dtype=np.float32)[:, None] + np.array([0.0, 0.5], np.float32)[None, :]).reshape(-1)
    near = np.concatenate([t, np.nextafter(t, np.float32(1e9)), np.nextafter(t, np.float32(-1e9))])
    x = np.concatenate([near, near / np.float32(255), near / np.float32(127.5) - np.float32(1),
                        np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e30, -1e30, 65504.0, 1e-45, -1e-45, 1.17549435e-38], np.float32),
                        f32_witnesses()[0], r.integers(0, 2 ** 32, size=20000, dtype=np.uint32).view(np.float32)])
    h = -(-x.size // (4 * F32_W))
    bits = np.concatenate([np.ascontiguousarray(x).view(np.uint32), r.integers(0, 2 ** 32, size=h * F32_W * 4 - x.size, dtype=np.uint32)])
    P = bits[np.random.default_rng(6).permutation(bits.size)].view(np.float32).reshape(h, F32_W, 4)
    P.setflags(write=False)
    return P


@functools.lru_cache(maxsize=None)
def half_patterns(dtype):
    """[128, 128, 4]: all 65536 bit patterns of binary16 (as float16) or bfloat16 (as uint16), each once, in a fixed shuffled order"""
    bits = np.random.default_rng(16).permutation(65536).astype(np.uint16).reshape(128, 128, 4)
    assert np.array_equal(np.sort(bits.reshape(-1)), np.arange(65536))
    P = bits.view(np.float16) if dtype == tiles.F16 else bits
    P.setflags(write=False)
    return P


def patterns(dtype):
    return f32_patterns() if dtype == tiles.F32 else half_patterns(dtype)


def ties(P, dtype, rng):
    """the t of the elements of P that are ties of the byte: strictly between 0 and 255, a half above an integer"""
    x = tiles.widen(P, dtype)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        t = x * np.float32(255.0) if rng == tiles.UNIT else x * np.float32(127.5) + np.float32(127.5) if rng == tiles.SYMMETRIC else x
        assert t.dtype == np.float32
        return t[(t > 0) & (t < 255) & (t - np.floor(t) == np.float32(0.5))]


def fused_bytes(x):
    """to_bytes(x, SYMMETRIC) as a kernel would give it that contracted the multiply and the add: the model's bytes with the fused byte
    at every witness"""
    x = np.asarray(x, np.float32)
    out = tiles.to_bytes(x, tiles.SYMMETRIC)
    wx, _, fused = f32_witnesses()
    order = np.argsort(wx.view(np.uint32))
    keys = wx.view(np.uint32)[order]
    flat, res = np.ascontiguousarray(x).view(np.uint32).reshape(-1), out.reshape(-1)
    at = np.searchsorted(keys, flat)
    hit = (at < keys.size) & (keys[np.minimum(at, keys.size - 1)] == flat)
    res[hit] = fused[order][at[hit]]
    return res.reshape(x.shape)


# ------------------------------------------------------------------ placements: tensors in one 256-aligned device buffer
ODD, ALIGNED, ONE = "odd", "aligned", "one"


def offsets(specs, how=ODD):
    """(byte offsets, end) of the tensors specs[i] = (w, h, sch, (dtype, layout, range), ...) laid one behind the other.  ODD: 1 or 3
    elements behind a 16-byte boundary; ALIGNED: at a multiple of 256, where torch hands a tensor over; ONE: one element behind a
    16-byte boundary.  how: one placement, or one per tensor."""
    hows = [how] * len(specs) if isinstance(how, str) else list(how)
    assert len(hows) == len(specs)
    out, cur = [], 0
    for i, (spec, hw) in enumerate(zip(specs, hows)):
        w, h, sch, fmt = spec[:4]
        elem = tiles.ELEM[fmt[0]]
        if hw == ALIGNED:
            off = (cur + 255) // 256 * 256
            assert off % 256 == 0
        else:
            off = (cur + 15) // 16 * 16 + elem * ((1 + 2 * (i & 1)) if hw == ODD else 1)
            assert hw in (ODD, ONE) and off % elem == 0 and off % 16 != 0
        out.append(off)
        cur = off + w * h * sch * elem
    return out, cur


def cases_of(specs, offs, ts, channels):
    """the tiles ts of the tensors specs at the byte offsets offs (of a 256-aligned buffer), at each channel count of the call, as what
    ingest_host_paths replays: (w, h, sch, src_flags, address modulo 256, x, y, cw, ch, flips, och)"""
    out = []
    for c in channels:
        for t in ts:
            w, h, sch, fmt = specs[t[0]][:4]
            assert t[5] == 1 and (t[6] & tiles.SRC_MASK) == tiles.source_flags(*fmt)
            out.append((w, h, sch, t[6] & tiles.SRC_MASK, offs[t[0]] % 256, t[1], t[2], t[3], t[4], t[6] & 3, c or sch))
    return out


# ------------------------------------------------------------------ the values: tests/test_gpu_ingest_values.py
VALUE_CHANNELS = (4, 3)


def value_specs(dtype):
    """(specs, placements): the pattern image of the dtype in every range, HWC and CHW, each at a 256-aligned address and one element
    behind a 16-byte boundary"""
    P = patterns(dtype)
    h, w, _ = P.shape
    planar = np.ascontiguousarray(np.transpose(P, (2, 0, 1)))
    specs, hows = [], []
    for rng in RANGES:
        for layout in (tiles.HWC, tiles.CHW):
            for how in (ALIGNED, ONE):
                specs.append((w, h, 4, (dtype, layout, rng), planar if layout == tiles.CHW else P))
                hows.append(how)
    return specs, hows


def value_tiles(specs):
    """of every tensor: the whole image unflipped and flipped in x, and three rectangles at x = 1 that are three pixels narrower than the
    image (128: cw = 125) - their items cross rows - in the other three flips, of heights at which the last item holds 3, 2 and 1 pixels"""
    ts = []
    for i, (w, h, sch, fmt, _) in enumerate(specs):
        f = tiles.source_flags(*fmt)
        ts += [(i, 0, 0, w, h, 1, f), (i, 0, 0, w, h, 1, f | tiles.FLIP_X)]
        cw = w - 3
        assert cw % 4 == 1
        for k, flips in enumerate((0, tiles.FLIP_Y, tiles.FLIP_X | tiles.FLIP_Y)):
            ch = next(c for c in range(h - k, 0, -1) if cw * c % 4 == 3 - k)
            ts.append((i, 1, k, cw, ch, 1, f | flips))
    return ts


# ------------------------------------------------------------------ mixed tensors: tests/test_gpu_ingest.py
MIXED_CHANNELS = (0, 3, 4)


def mixed_specs(param):
    """every legal dtype x layout x range with sch 3 and 4: 40 tensors of the five shapes"""
    specs = [(*SHAPES[(i + 2 * param + (sch == 4)) % 5], sch, fmt, None) for i, fmt in enumerate(FORMATS) for sch in (3, 4)]
    assert len(specs) == 40
    return specs


def tiles_of(specs, k0=0):
    """every image whole, and where it is wide enough a rectangle at x = 1 and one at the right edge; the four flips go round"""
    ts = []
    for i, spec in enumerate(specs):
        w, h, f = spec[0], spec[1], tiles.source_flags(*spec[3])
        ts.append((i, 0, 0, w, h, 1, f | ((i + k0) & 3)))
        if w > 4:
            ts.append((i, 1, 0, w - 2, h, 1, f | ((i + k0 + 1) & 3)))
            ts.append((i, w - 4, 1, 4, h - 1, 1, f | ((i + k0 + 2) & 3)))
    return ts


ROUND_TRIP_SHAPES = [(37, 23), (70, 9), (300, 17)]
ROUND_TRIP_FORMATS = [(tiles.F16, tiles.CHW, tiles.UNIT), (tiles.F32, tiles.HWC, tiles.SYMMETRIC)]


def round_trip_offsets(nbytes, aligned):
    """out_offsets of the round trip's decode_tensors, which are the pixel_offsets of its second encode: element-aligned and not
    16-aligned, or multiples of 256"""
    if aligned:
        return [int(v) for v in np.cumsum([0] + [(b + 255) // 256 * 256 for b in nbytes[:-1]])]
    return [int(v) + 4 * (k + 1) for k, v in enumerate(np.cumsum([0] + [(b + 15) // 16 * 16 for b in nbytes[:-1]]))]


def round_trip_cases():
    out = []
    for ch in (3, 4):
        for fmt in ROUND_TRIP_FORMATS:
            specs = [(w, h, ch, fmt) for w, h in ROUND_TRIP_SHAPES]
            ts = [(i, 0, 0, w, h, 1, tiles.source_flags(*fmt) | (i & 3)) for i, (w, h) in enumerate(ROUND_TRIP_SHAPES)]
            for aligned in (False, True):
                out += cases_of(specs, round_trip_offsets([w * h * ch * tiles.ELEM[fmt[0]] for w, h in ROUND_TRIP_SHAPES], aligned), ts, (0,))
    return out


# ------------------------------------------------------------------ offsets past 2^32: tests/test_gpu_offsets_wide.py
# part 1: (w, h, sch, format); `layout` of that file places them control, beyond and - the longest, f32 CHW - across byte 2^32 in turn, so
# that every dtype lies beyond or across
WIDE_SPECS = [(70, 45, 4, (tiles.F16, tiles.CHW, tiles.UNIT)), (64, 48, 3, (tiles.U8, tiles.CHW, tiles.UNIT)), (130, 70, 3, (tiles.F32, tiles.CHW, tiles.SYMMETRIC)),
              (37, 29, 4, (tiles.BF16, tiles.HWC, tiles.BYTES)), (38, 29, 3, (tiles.F16, tiles.CHW, tiles.SYMMETRIC)), (33, 21, 4, (tiles.U8, tiles.CHW, tiles.UNIT)),
              (70, 45, 3, (tiles.BF16, tiles.HWC, tiles.UNIT)), (21, 13, 4, (tiles.F32, tiles.CHW, tiles.BYTES))]
WIDE_ELEM = 4                   # every offset of the call and every tensor's size is a multiple of the largest element
WIDE_CHANNELS = (0, 3)


def wide_tiles():
    """every tensor whole and a rectangle of it at x = 1, y = 1; the flips go round"""
    ts = []
    for i, (w, h, _, fmt) in enumerate(WIDE_SPECS):
        f = tiles.source_flags(*fmt)
        ts += [(i, 0, 0, w, h, 1, f | (i & 3)), (i, 1, 1, w - 2, h - 1, 1, f | ((i + 1) & 3))]
    return ts


# part 2: one f32 source of BIG_SIDE x BIG_SIDE x 4, longer than 4 GiB.  Windows are whole rows [r0, r1) (CHW: of every plane); the rest
# of the image is a constant.  "straddle" holds byte 2^32 of the image, "last" its last rows; the aliases of their elements - 2^30
# elements lower - lie in the decoy windows; "control" is low in the image.
BIG_SIDE = 16400
BIG_WINDOWS = {tiles.HWC: {"control": (100, 108), "straddle": (16364, 16372), "last": (16392, 16400), "decoys": [(0, 40)]},
               tiles.CHW: {"control": (200, 208), "straddle": (16268, 16276), "last": (16392, 16400), "decoys": [(0, 6), (118, 130)]}}
BIG_CHANNELS = (0, 3)


def big_index(layout, y, x, c):
    """the element index of channel c of pixel (x, y)"""
    return (y * BIG_SIDE + x) * 4 + c if layout == tiles.HWC else (c * BIG_SIDE + y) * BIG_SIDE + x


def big_tiles(layout):
    """(name of the window, tile): 400 to 403 x 8 pixels of each of the three true windows - the straddling one around the column that holds
    byte 2^32 -, in every flip, and one tile of the constant"""
    f = tiles.source_flags(tiles.F32, layout, tiles.UNIT)
    out = []
    for name in ("control", "straddle", "last"):
        r0, r1 = BIG_WINDOWS[layout][name]
        for flips in range(4):
            cw = 400 + flips                                           # (odd widths: items of a CHW tile cross rows)
            x = {tiles.HWC: 100, tiles.CHW: 800}[layout] if name == "straddle" else 3 if name == "control" else BIG_SIDE - cw
            out.append((name, (0, x, r0, cw, r1 - r0, 1, f | flips)))
    return out + [("fill", (0, 7, 5000, 400, 8, 1, f))]                 # and one of the constant alone


def big_cases(layout, base_mod=0):
    specs = [(BIG_SIDE, BIG_SIDE, 4, (tiles.F32, layout, tiles.UNIT))]
    return cases_of(specs, [base_mod], [t for _, t in big_tiles(layout)], BIG_CHANNELS)
