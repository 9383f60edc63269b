"""The guarded-output runners of the -m gpu tests, one per call family, and what travels with them: every runner lays the outputs
of one call between guard bytes (gpu_pack.GUARD), makes the call, checks every guard byte and returns the outputs.  The fixtures and
packs are in tests/gpu_pack.py.

No assert here is rewritten by pytest (this is no test module): every assert carries its operands in its message."""
import numpy as np

import ingest_cases
from gpu_pack import GUARD, IMAGENET, dev, filled
from gpu_util import GuardedRegion
from ingest_cases import ODD
from model_cases import pack_offsets
from qoi_amd import resize, tensors, thumbs, tiles, warp
from qoi_amd.tensors import HW, I32, I64, U8


def assert_outputs(got, wants, what):
    """got[j] holds the bytes of wants[j] (an array of any dtype and shape, or a bytes object), for every output of a call"""
    assert len(got) == len(wants), (what, "outputs", len(got), len(wants))
    for j, (g, w) in enumerate(zip(got, wants)):
        w = np.frombuffer(bytes(w), dtype=np.uint8) if isinstance(w, (bytes, bytearray)) else np.ascontiguousarray(w).view(np.uint8).reshape(-1)
        assert g.size == w.size and np.array_equal(g, w), (what, "output", j, "first difference at byte", int(np.argmax(g != w)) if g.size == w.size else None, "of", w.size)


def sizes_of(items, och):
    return [it[5] * it[6] * och for it in items]


def run_warp(ctx, p, channels, items, mode=warp.PLAIN, staging=0, offsets=None, total=None, front=64, call=None):
    """One call; outputs back to back behind `front` guard bytes unless offsets are given.  Returns the outputs."""
    och = channels or p.shapes[items[0][0]][2]
    nbytes = sizes_of(items, och)
    if offsets is None:
        offsets = [front + int(x) for x in np.cumsum([0] + nbytes[:-1])]
    if total is None:
        total = max(o + n for o, n in zip(offsets, nbytes)) + 64
    buf = filled(total, GUARD)
    if call is None:
        ctx.decode_warped(p.packed.data_ptr(), p.so, p.sizes, p.descs, channels, items, mode, buf.data_ptr(), offsets, staging)
    else:
        call(buf.data_ptr(), offsets)
    got = buf.cpu().numpy()
    mask = np.ones(total, dtype=bool)
    for o, n in zip(offsets, nbytes):
        mask[o:o + n] = False
    assert np.all(got[mask] == GUARD), ("a byte outside the outputs was written", int(np.argmax(mask & (got != GUARD))))
    return [got[o:o + n] for o, n in zip(offsets, nbytes)]


def want_warp(p, it, och, mode):
    i, x, y, cw, rh, ow, oh, flags, a, b, d, e, fill, _, c, f = it
    return warp.warp(p.decoded(i, och), (x, y, cw, rh), (ow, oh), (a, b, c, d, e, f), flags, fill, mode).reshape(-1)


def assert_warp_items(p, got, items, och, mode, what):
    for j, it in enumerate(items):
        w = want_warp(p, it, och, mode)
        assert got[j].size == w.size and np.array_equal(got[j], w), (what, j, it, int(np.argmax(got[j] != w)))


def standard(i, w, h, first_flag=0):
    """identity; the whole image to 1 x 1 where the cap allows, else to ceil(w/64) x ceil(h/64); a non-integer downscale (130 x 70 -> 37 x 23,
    smaller images in that proportion); an interior rectangle with odd origin and odd size to an odd size; an upscale of a 1 x 1 and of a
    (up to) 5 x 3 rectangle; down in x with up in y; the flag values take turns"""
    out = [(0, 0, w, h, w, h), (0, 0, w, h, -(-w // 64), -(-h // 64)), (0, 0, w, h, max(1, w * 37 // 130), max(1, h * 23 // 70))]
    if w >= 3 and h >= 4:
        out.append((1, 3, w - 1 if (w - 1) % 2 else w - 2, h - 3 if (h - 3) % 2 else h - 4, 7, 5))
    out.append((w - 1, h - 1, 1, 1, 4, 3))
    out.append((w // 3, h // 3, min(5, w - w // 3), min(3, h - h // 3), 13, 7))
    out.append((0, 0, w, min(h, 3), max(1, w // 3), 8))
    return [(i, x, y, cw, rh, ow, oh, (first_flag + k) & 3) for k, (x, y, cw, rh, ow, oh) in enumerate(out)]


def run_resized(ctx, p, channels, items, mode=resize.PLAIN, staging=0, offsets=None, total=None, sizes=None, packed=None, front=64, descs=None):
    """One call; outputs back to back behind `front` guard bytes unless offsets are given.  Returns the outputs."""
    och = channels or p.shapes[items[0][0]][2]
    nbytes = sizes_of(items, och)
    if offsets is None:
        offsets = [front + int(x) for x in np.cumsum([0] + nbytes[:-1])]
    if total is None:
        total = max(o + n for o, n in zip(offsets, nbytes)) + 64
    buf = filled(total, GUARD)
    ctx.decode_resized((p.packed if packed is None else packed).data_ptr(), p.so, p.sizes if sizes is None else sizes, p.descs if descs is None else descs,
                       channels, items, mode, buf.data_ptr(), offsets, staging)
    got = buf.cpu().numpy()
    mask = np.ones(total, dtype=bool)
    for o, n in zip(offsets, nbytes):
        mask[o:o + n] = False
    assert np.all(got[mask] == GUARD), ("a byte outside the outputs was written", int(np.argmax(mask & (got != GUARD))))
    return [got[o:o + n] for o, n in zip(offsets, nbytes)]


def standard_crops(i, w, h, first_flag=0):
    """the whole image, the 1 x 1 crop at each corner, one column, one row, an interior rectangle with odd origin and odd size; the flag
    values take turns"""
    out = [(0, 0, w, h), (0, 0, 1, 1), (w - 1, 0, 1, 1), (0, h - 1, 1, 1), (w - 1, h - 1, 1, 1), (w // 2, 0, 1, h), (0, h // 2, w, 1)]
    if w >= 3 and h >= 4:
        out.append((1, 3, w - 1 if (w - 1) % 2 else w - 2, h - 3 if (h - 3) % 2 else h - 4))
    return [(i, x, y, cw, ch, (first_flag + k) & 3) for k, (x, y, cw, ch) in enumerate(out)]


WARP = 2                               # the third kind of call, beside FILTER_AREA and FILTER_BILINEAR
# 255 * 300 - 300 is infinity in binary16; v * 2.4e-8 lies in its subnormals; v * 1e-40 in those of binary32 and bfloat16; -0 at v = 0
WILD = (np.array([300.0, -1e-6, 2.4e-8, 1e-40], np.float32), np.array([-300.0, -0.0, -1e-41, 0.0], np.float32))


def tensor_layout(items, och, elem, front=None):
    """(offsets, byte sizes, total): the first output at an odd element-aligned address, 1 to 3 guard bytes - in whole elements - between"""
    nbytes = [it[5] * it[6] * och * elem for it in items]
    pos = {1: 65, 2: 66, 4: 68}[elem] if front is None else front
    offsets = []
    for j, n in enumerate(nbytes):
        offsets.append(pos)
        pos += n + -(-(1 + j % 3) // elem) * elem
    return offsets, nbytes, pos + 64


def run_tensors(ctx, p, kind, channels, items, mode, f, staging=0, front=None):
    """One call; returns the outputs as bytes.  The buffer's base is a multiple of 256 (torch's allocator), so the offsets are the alignment."""
    och = channels or p.shapes[items[0][0]][2]
    offsets, nbytes, total = tensor_layout(items, och, tensors.ELEM[f[0]], front)
    buf = filled(total, GUARD)
    assert buf.data_ptr() % 256 == 0, ("the output buffer's base is no multiple of 256", buf.data_ptr())
    if kind == WARP:
        ctx.decode_warped_tensors(p.packed.data_ptr(), p.so, p.sizes, p.descs, channels, items, mode, f, buf.data_ptr(), offsets, staging)
    else:
        ctx.decode_tensors(p.packed.data_ptr(), p.so, p.sizes, p.descs, channels, items, kind, mode, f, buf.data_ptr(), offsets, staging)
    got = buf.cpu().numpy()
    mask = np.ones(total, dtype=bool)
    for o, n in zip(offsets, nbytes):
        mask[o:o + n] = False
    assert np.all(got[mask] == GUARD), ("a byte outside the outputs was written", int(np.argmax(mask & (got != GUARD))))
    return [got[o:o + n] for o, n in zip(offsets, nbytes)]


def fmt_of(dtype, layout):
    return tensors.fmt(dtype, layout) if dtype in (U8, I32, I64) else (dtype, layout, *IMAGENET)


def label_layout(items, och, f, front=None):
    """(offsets, byte sizes, total): the first output at an odd element-aligned address, 1 to 3 guard bytes - in whole elements - between"""
    elem = tensors.elem(f[0])
    nbytes = [it[5] * it[6] * (1 if f[1] == HW else och) * elem for it in items]
    pos = 64 + elem if front is None else front
    offsets = []
    for j, n in enumerate(nbytes):
        offsets.append(pos)
        pos += n + -(-(1 + j % 3) // elem) * elem
    return offsets, nbytes, pos + 64


def run_label_tensors(ctx, p, filt, channels, items, mode, f, staging=0):
    """One call; returns the outputs as bytes.  The buffer's base is a multiple of 256 (torch's allocator), so the offsets are the alignment."""
    och = channels or p.shapes[items[0][0]][2]
    offsets, nbytes, total = label_layout(items, och, f)
    buf = filled(total, GUARD)
    assert buf.data_ptr() % 256 == 0, ("the output buffer's base is no multiple of 256", buf.data_ptr())
    if filt == "warp":
        ctx.decode_warped_tensors(p.packed.data_ptr(), p.so, p.sizes, p.descs, channels, items, mode, f, buf.data_ptr(), offsets, staging)
    else:
        ctx.decode_tensors(p.packed.data_ptr(), p.so, p.sizes, p.descs, channels, items, filt, mode, f, buf.data_ptr(), offsets, staging)
    got = buf.cpu().numpy()
    mask = np.ones(total, dtype=bool)
    for o, n in zip(offsets, nbytes):
        mask[o:o + n] = False
    assert np.all(got[mask] == GUARD), ("a byte outside the outputs was written", int(np.argmax(mask & (got != GUARD))))
    return [got[o:o + n] for o, n in zip(offsets, nbytes)]


def assert_info(got, want, tag):
    for k in ("pixels", "run_pixels", "repeat_index", "walk_end", "flags"):
        assert int(got[k]) == want[k], (tag, k, int(got[k]), want[k], [int(x) for x in got["ops"]], want["ops"])
    assert [int(x) for x in got["ops"]] == want["ops"], (tag, [int(x) for x in got["ops"]], want["ops"])
    assert not got["reserved"].any(), tag


TILE_FILL = 0xA5
TILE_FRONT = 256


class Sources:
    """Images in one device buffer with gaps, at the byte offsets given; the buffer's host copy never changes."""

    def __init__(self, api, shapes, seed=5):
        rng = np.random.default_rng(seed)
        self.shapes = shapes
        end = max(off + w * h * ch for (w, h, ch, off) in shapes)
        self.host = rng.integers(0, 256, size=end + 64, dtype=np.uint8)
        self.img = []
        for (w, h, ch, off) in shapes:
            v = self.host[off:off + w * h * ch].reshape(h, w, ch)
            if ch == 4:
                v[:, :, 3] = rng.choice(np.array([0, 2, 200, 255], dtype=np.uint8), size=(h, w))
                v[: h // 2, : w // 2, 3] = 0
            if w * h > 64:
                v[h // 3: h // 3 + 4, :, :] = v[h // 3, 0]                 # some runs and repeats: streams of every chunk kind
            self.img.append(v)
        self.off = [s[3] for s in shapes]
        self.descs = [api.QoiDesc(w, h, ch, i & 1) for i, (w, h, ch, _) in enumerate(shapes)]
        self.d = dev(self.host)
        assert self.d.data_ptr() % 256 == 0, ("the source buffer's base is no multiple of 256", self.d.data_ptr())


def tile_model(oracle, src, ts, channels, mode):
    px = [tiles.tile(src.img[t[0]], t, channels, mode) for t in ts]
    streams = [oracle.encode(p.reshape(-1), p.shape[1], p.shape[0], p.shape[2], src.descs[t[0]].colorspace) for p, t in zip(px, ts)]
    return px, streams


def run_tiles(ctx, src, ts, channels, mode, align, streams, staging=0, capacity=None, null_dest=False, shift=0):
    """One call; checks tables, descriptors, bytes and guards.  Returns (offsets, sizes, descs)."""
    import torch
    n = len(ts)
    lens = [len(s) for s in streams]
    want_off = pack_offsets(lens, align)
    cap = int(want_off[-1]) if capacity is None else capacity
    starts = [TILE_FRONT + shift + int(o) for o in want_off[:n]]
    region = GuardedRegion(TILE_FRONT + shift + max(cap, 0) + 512, starts, TILE_FILL)
    buf = torch.full((region.size,), TILE_FILL, dtype=torch.uint8, device="cuda")
    d_off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    d_len = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    dest = 0 if null_dest else buf[TILE_FRONT + shift:].data_ptr()
    got_off, got_len, got_descs = ctx.encode_tiles(src.d.data_ptr(), src.off, src.descs, channels, ts, mode, align, dest, cap, d_off.data_ptr(), d_len.data_ptr(), staging)
    what = (channels, mode, align, staging, cap)
    assert got_len.tolist() == lens, what
    assert np.array_equal(got_off, want_off), what
    assert np.array_equal(d_off.cpu().numpy().astype(np.uint64), want_off) and d_len.cpu().numpy().tolist() == lens, what
    for t, d in zip(ts, got_descs):
        sd = src.descs[t[0]]
        nbytes, tw, th = tiles.size(sd.width, sd.height, sd.channels, t, channels)
        assert (d.width, d.height, d.channels, d.colorspace) == (tw, th, channels or sd.channels, sd.colorspace), (what, t)
    host = buf.cpu().numpy()
    present = [ln if int(o) + ln <= cap else 0 for o, ln in zip(want_off[:n], lens)]         # a stream that does not fit wholly is absent
    for k, s in enumerate(streams):
        if present[k]:
            assert host[starts[k]:starts[k] + lens[k]].tobytes() == s, (what, "stream", k, ts[k])
    region.starts = [min(s, region.size) for s in starts]
    region.assert_untouched(host, present, what)
    ctx.encode_status(0)                                      # QOIMI_OK, and nothing is encoded again
    return got_off, got_len, got_descs


def elements(rng, count, dtype, rng_bits):
    """random elements over [-0.25, 1.25] scaled to the range (both clamps occur), as the dtype's array (BF16: its bits)"""
    if dtype == tiles.U8:
        return rng.integers(0, 256, size=count, dtype=np.uint8)
    x = rng.uniform(-0.25, 1.25, size=count).astype(np.float32)
    x = {tiles.UNIT: x, tiles.SYMMETRIC: x * 2 - 1, tiles.BYTES: x * 255}[rng_bits]
    if dtype == tiles.F32:
        return x
    return x.astype(np.float16) if dtype == tiles.F16 else tensors.bf16_bits(x)


class Tensors:
    """Tensors of different formats in one device buffer, each at an element-aligned byte offset that is no multiple of 16 - or, how=ALIGNED,
    each at a multiple of 256; how may name a placement per tensor (ingest_cases.offsets) -; the interface of
    Sources as far as run_tiles looks at it (d, off, descs).  specs: (w, h, sch, (dtype, layout, range), elements or None)."""

    def __init__(self, api, specs, seed=7, how=ODD):
        rng = np.random.default_rng(seed)
        self.off, self.flags, self.arrays, self.descs, parts = [], [], [], [], []
        placed, cur = ingest_cases.offsets(specs, how)                      # ODD: 1 or 3 elements behind a 16-byte boundary
        for i, (w, h, sch, fmt, given) in enumerate(specs):
            off = placed[i]
            a = np.ascontiguousarray(elements(rng, w * h * sch, fmt[0], fmt[2]) if given is None else given)
            assert a.size == w * h * sch and a.dtype == tiles.SOURCE_ARRAYS[fmt[0]], (i, a.size, w * h * sch, a.dtype, tiles.SOURCE_ARRAYS[fmt[0]])
            self.arrays.append(a.reshape((sch, h, w) if fmt[1] == tiles.CHW else (h, w, sch)))
            self.off.append(off)
            self.flags.append(tiles.source_flags(*fmt))
            self.descs.append(api.QoiDesc(w, h, sch, i & 1))
            parts.append((off, a.view(np.uint8).reshape(-1)))
        self.host = rng.integers(0, 256, size=cur + 64, dtype=np.uint8)
        for off, b in parts:
            self.host[off:off + b.size] = b
        self.d = dev(self.host)
        assert self.d.data_ptr() % 256 == 0, ("the source buffer's base is no multiple of 256", self.d.data_ptr())
        self.specs = specs
        self.bytes = [tiles.convert(a, f) for a, f in zip(self.arrays, self.flags)]         # computed once, never changed


def ingest_model(oracle, src, ts, channels):
    px = [tiles.tile(src.bytes[t[0]], t[:6] + (t[6] & 3,), channels) for t in ts]
    return px, [oracle.encode(p.reshape(-1), p.shape[1], p.shape[0], p.shape[2], src.descs[t[0]].colorspace) for p, t in zip(px, ts)]


def conditions(dtype, specs, ts, bytes_of):
    """what makes the exact comparison a test of the conversion (no GPU): the expected bytes hold 0 and 255, ties that round down to an
    even byte and ties that round up to one, and - binary32, SYMMETRIC - every tile would be another one had the kernel fused the multiply
    and the add.  bytes_of[i]: the model's byte image of tensor i."""
    P = ingest_cases.patterns(dtype)
    parities = set()
    for rng in ingest_cases.RANGES:
        B = tiles.to_bytes(tiles.widen(P, dtype), rng)
        assert B.min() == 0 and B.max() == 255, (dtype, rng)
        t = ingest_cases.ties(P, dtype, rng)
        parities |= set((np.floor(t).astype(np.int64) % 2).tolist())
        assert t.size >= 1 and np.array_equal(tiles.to_bytes(t, tiles.BYTES), (np.floor(t).astype(np.int64) + 1) // 2 * 2), (dtype, rng)     # to even
    assert parities == {0, 1}, dtype
    fused = 0
    for t in ts:
        w, h, sch, fmt, A = specs[t[0]]
        assert np.array_equal(bytes_of[t[0]], tiles.to_bytes(tiles.widen(P, dtype), fmt[2])), ("the model's bytes of tensor", t[0], dtype, fmt)   # (HWC and CHW hold the same pixels)
        if dtype == tiles.F32 and fmt[2] == tiles.SYMMETRIC:
            for och in ingest_cases.VALUE_CHANNELS:
                plain = t[:6] + (t[6] & 3,)
                assert not np.array_equal(tiles.tile(ingest_cases.fused_bytes(P), plain, och), tiles.tile(bytes_of[t[0]], plain, och)), (t, och)
                fused += 1
    assert fused == (2 * 2 * 5 * 2 if dtype == tiles.F32 else 0), ("tiles that fusing would change", fused, dtype)


def thumb_bytes(shapes, factors, och):
    return [int(np.prod(thumbs.size(w, h, f))) * och for (w, h, _), f in zip(shapes, factors)]


def run_thumbnails(ctx, p, channels, factors, mode, staging=0, offsets=None, total=None, sizes=None, packed=None):
    """One call; thumbnails back to back behind 64 guard bytes unless offsets are given.  Returns (thumbnails, the whole buffer, offsets)."""
    och = channels or p.shapes[0][2]
    if isinstance(factors, int):
        factors = [factors] * p.n
    nbytes = thumb_bytes(p.shapes, factors, och)
    if offsets is None:
        offsets = [64 + int(x) for x in np.cumsum([0] + nbytes[:-1])]
        total = offsets[-1] + nbytes[-1] + 64
    buf = filled(total, GUARD)
    ctx.decode_thumbnails((p.packed if packed is None else packed).data_ptr(), p.so, p.sizes if sizes is None else sizes, p.descs, channels, factors, mode,
                          buf.data_ptr(), offsets, staging)
    got = buf.cpu().numpy()
    mask = np.ones(total, dtype=bool)
    for o, n in zip(offsets, nbytes):
        mask[o:o + n] = False
    assert np.all(got[mask] == GUARD), ("a byte outside the thumbnails was written", int(np.argmax(mask & (got != GUARD))))
    return [got[o:o + n] for o, n in zip(offsets, nbytes)], got, offsets
