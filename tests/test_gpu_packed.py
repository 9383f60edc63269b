"""Packed streams on the GPU (-m gpu): qoimi_pack_streams against the numpy model of tests/test_packed_api.py and the reference
encoder's bytes, qoimi_decode_images on tight, unaligned, unordered placement against the reference decoder's pixels (guard bytes
around every image), qoimi_read_descs, and the three-call round trip.  Expected streams and pixels come from the `ref` / `port`
oracles and the golden file."""
import ctypes

import numpy as np
import pytest

import cases
from gpu_pack import E_ARG, GUARD, Item, dev, filled, packed_image as image
from gpu_pack import api, ctx, oracle  # noqa: F401  (fixtures)
from model_cases import pack_offsets as offsets

pytestmark = pytest.mark.gpu


def mixed_items(api, oracle):
    """44 images: 1x1, 1xN, Nx1, odd widths, flat and non-flat classes interleaved, one of 1024 x 1024; 4-channel sources."""
    shapes = [(1, 1), (1, 97), (131, 1), (37, 23), (257, 9), (64, 48), (333, 7), (640, 360), (5, 5), (101, 77), (1920, 3)]
    kinds = ["photo", "uiflat", "sprite_alpha", "noise", "constant"]
    items = []
    for i in range(43):
        w, h = shapes[i % len(shapes)]
        items.append(Item(api, oracle, kinds[i % len(kinds)], w, h, 4, frame=i))
    items.insert(20, Item(api, oracle, "photo", 1024, 1024, 4, frame=3))
    return items


def pack_host(streams, gap=0):
    """streams back to back (gap bytes of 0x5C between them) -> (bytes, offsets)"""
    offs, blob = [], bytearray()
    for s in streams:
        offs.append(len(blob))
        blob += s + b"\x5c" * gap
    return bytes(blob), offs


def decode_tight(ctx, oracle, items, channels, gap=0, perm_in=None, perm_out=None, front=64):
    """Decodes `items` from a host-made pack into tightly placed images; checks every image against the oracle and every guard byte.
    perm_in / perm_out: the order in which streams / images lie in their buffers.  Returns the pixel buffer (numpy)."""
    n = len(items)
    perm_in = list(range(n)) if perm_in is None else perm_in
    perm_out = list(range(n)) if perm_out is None else perm_out
    blob, offs_p = pack_host([items[i].stream for i in perm_in], gap=0)
    so = [0] * n
    for k, i in enumerate(perm_in):
        so[i] = offs_p[k]
    d_streams = dev(np.frombuffer(blob, dtype=np.uint8).copy())
    och = [channels or it.ch for it in items]
    size = [it.w * it.h * o for it, o in zip(items, och)]
    po, at = [0] * n, front
    for i in perm_out:
        po[i] = at
        at += size[i] + gap
    out = filled(at + 64)
    ctx.decode_images(d_streams.data_ptr(), so, [len(it.stream) for it in items], [it.desc for it in items], channels, out.data_ptr(), po)
    got = out.cpu().numpy()
    rounds = ctx.decode_stats()["rounds"]
    mask = np.ones(got.size, dtype=bool)
    for i, it in enumerate(items):
        want, _ = oracle.decode(it.stream, channels)
        assert np.array_equal(got[po[i]:po[i] + size[i]], want), (i, it.w, it.h, channels, gap, f"rounds={rounds}")
        mask[po[i]:po[i] + size[i]] = False
    assert np.all(got[mask] == GUARD), ("a byte beside the images was written", int(np.argmax(mask & (got != GUARD))), f"rounds={rounds}")
    return got


# ------------------------------------------------------------------ 0: rejections
def test_rejections(api, ctx, oracle):
    lib = api.load_library()
    it = Item(api, oracle, "photo", 64, 48, 4)
    n = 2
    stride = len(it.stream) + 3
    src = filled(n * stride, 0)
    for i in range(n):
        src[i * stride:i * stride + len(it.stream)].copy_(dev(np.frombuffer(it.stream, dtype=np.uint8).copy()))
    lens = dev(np.array([len(it.stream)] * n, dtype=np.int32))
    packed, off, out = filled(4096 * 8), filled(8 * (n + 1)), filled(2 * 64 * 48 * 4 + 64)
    h, S, P, L, O, X = ctx._h, src.data_ptr(), packed.data_ptr(), lens.data_ptr(), off.data_ptr(), out.data_ptr()
    so = (ctypes.c_size_t * n)(0, stride)
    sz = (ctypes.c_int * n)(len(it.stream), len(it.stream))
    ds = (api.QoiDesc * n)(it.desc, it.desc)
    po = (ctypes.c_size_t * n)(0, 64 * 48 * 4)
    short = (ctypes.c_int * n)(len(it.stream), 21)
    bad_ds = (api.QoiDesc * n)(it.desc, api.QoiDesc(0, 4, 4, 0))
    lap = (ctypes.c_size_t * n)(0, 64 * 48 * 4 - 1)
    calls = {
        "pack: NULL source": lambda: lib.qoimi_pack_streams(h, None, stride, L, n, 1, P, packed.numel(), O, None),
        "pack: NULL lengths": lambda: lib.qoimi_pack_streams(h, S, stride, None, n, 1, P, packed.numel(), O, None),
        "pack: NULL destination": lambda: lib.qoimi_pack_streams(h, S, stride, L, n, 1, None, packed.numel(), O, None),
        "pack: NULL offsets": lambda: lib.qoimi_pack_streams(h, S, stride, L, n, 1, P, packed.numel(), None, None),
        "pack: n 0": lambda: lib.qoimi_pack_streams(h, S, stride, L, 0, 1, P, packed.numel(), O, None),
        "pack: align 0": lambda: lib.qoimi_pack_streams(h, S, stride, L, n, 0, P, packed.numel(), O, None),
        "pack: align 3": lambda: lib.qoimi_pack_streams(h, S, stride, L, n, 3, P, packed.numel(), O, None),
        "pack: align 512": lambda: lib.qoimi_pack_streams(h, S, stride, L, n, 512, P, packed.numel(), O, None),
        "pack: overlap": lambda: lib.qoimi_pack_streams(h, S, stride, L, n, 1, S + stride, stride, O, None),
        "decode: NULL streams": lambda: lib.qoimi_decode_images(h, None, so, sz, ds, n, 4, X, po, None),
        "decode: NULL offsets": lambda: lib.qoimi_decode_images(h, S, None, sz, ds, n, 4, X, po, None),
        "decode: NULL pixel offsets": lambda: lib.qoimi_decode_images(h, S, so, sz, ds, n, 4, X, None, None),
        "decode: NULL pixels": lambda: lib.qoimi_decode_images(h, S, so, sz, ds, n, 4, None, po, None),
        "decode: n 0": lambda: lib.qoimi_decode_images(h, S, so, sz, ds, 0, 4, X, po, None),
        "decode: size 21": lambda: lib.qoimi_decode_images(h, S, so, short, ds, n, 4, X, po, None),
        "decode: descriptor": lambda: lib.qoimi_decode_images(h, S, so, sz, bad_ds, n, 4, X, po, None),
        "decode: channels 5": lambda: lib.qoimi_decode_images(h, S, so, sz, ds, n, 5, X, po, None),
        "decode: outputs overlap": lambda: lib.qoimi_decode_images(h, S, so, sz, ds, n, 4, X, lap, None),
        "read_descs: NULL out": lambda: lib.qoimi_read_descs(h, S, so, sz, n, None, None, None),
        "read_descs: n 0": lambda: lib.qoimi_read_descs(h, S, so, sz, 0, ds, None, None),
    }
    import torch
    for name, call in calls.items():
        assert call() == E_ARG, name
        assert api.last_error() != "", name
    torch.cuda.synchronize()
    for buf in (packed, off, out):
        assert bool((buf == GUARD).all()), "a rejected call wrote to the caller's buffers"
    decode_tight(ctx, oracle, [it, it], 4)


# ------------------------------------------------------------------ 1: pack, bytes
def encode_strided(api, ctx, oracle, kind, w, h, ch, n, extra):
    import torch
    desc = api.QoiDesc(w, h, ch, 0)
    ps = w * h * ch
    stride = (api.encode_bound(w, h, ch) + extra) | 1        # odd, whatever the parity of the bound
    px = torch.empty(n * ps, dtype=torch.uint8, device="cuda")
    want = []
    for i in range(n):
        a = image(kind if i % 3 else "rand", w, h, ch, frame=i)
        px[i * ps:(i + 1) * ps].copy_(dev(a))
        want.append(oracle.encode(a, w, h, ch))
    streams = filled(n * stride, 0x3C)
    lens = torch.zeros(n, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    ctx.encode_batch(px.data_ptr(), ps, desc, n, streams.data_ptr(), stride, lens.data_ptr(), st)
    return streams, stride, lens, want


def check_pack(ctx, streams, stride, lens, want, align, capacity=None):
    """pack -> offsets equal the model on the reference's lengths, streams byte-identical, 0xA5 everywhere else"""
    import torch
    n = len(want)
    model = offsets([len(s) for s in want], align)
    cap = int(model[-1]) if capacity is None else capacity
    packed = filled(cap + 512)
    off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    view = packed[1:]                                      # an odd destination address
    ctx.pack_streams(streams.data_ptr(), stride, lens.data_ptr(), n, align, view.data_ptr(), cap, off.data_ptr(), st)
    ctx.encode_status(st)
    got_off = off.cpu().numpy().astype(np.uint64)
    assert np.array_equal(got_off, model), (align, got_off[:8], model[:8])
    got = view.cpu().numpy()
    mask = np.ones(got.size, dtype=bool)
    for i, s in enumerate(want):
        a, b = int(model[i]), int(model[i]) + len(s)
        if b > cap:
            continue                                       # does not fit wholly: not copied, not in part
        assert got[a:b].tobytes() == s, (align, i, len(s))
        mask[a:b] = False
    assert np.all(got[mask] == GUARD), (align, "gap / tail byte written", int(np.argmax(mask & (got != GUARD))))
    assert int(packed[0]) == GUARD
    return model


@pytest.mark.parametrize("n,w,h,ch,kind,extra", [(1, 640, 360, 4, "photo", 1), (3, 257, 9, 3, "uiflat", 3), (65, 37, 23, 4, "sprite_alpha", 1),
                                                 (1000, 5, 3, 4, "photo", 3), (3, 64, 48, 4, "constant", 1)])
def test_pack_bytes(api, ctx, oracle, n, w, h, ch, kind, extra):
    streams, stride, lens, want = encode_strided(api, ctx, oracle, kind, w, h, ch, n, extra)
    assert stride % 2 == 1
    for align in (1, 4, 64, 256):
        check_pack(ctx, streams, stride, lens, want, align)


# ------------------------------------------------------------------ 2, 3: pack, sizes and capacity
def sizes_mix(oracle):
    """hundreds of 23-byte streams (1x1 images) around one noise stream of several MB"""
    tiny = [oracle.encode(np.array([i & 255, 3, 200, 255], dtype=np.uint8), 1, 1, 4) for i in range(700)]
    big = oracle.encode(image("rand", 1024, 768, 4), 1024, 768, 4)
    want = tiny[:400] + [big] + tiny[400:]
    stride = len(big) + 1
    return want, stride


def upload_strided(want, stride):
    import torch
    streams = filled(len(want) * stride, 0x3C)
    for i, s in enumerate(want):
        streams[i * stride:i * stride + len(s)].copy_(dev(np.frombuffer(s, dtype=np.uint8).copy()))
    lens = dev(np.array([len(s) for s in want], dtype=np.int32))
    return streams, lens


def test_pack_sizes(ctx, oracle):
    want, stride = sizes_mix(oracle)
    assert len(want[400]) > 2 << 20
    streams, lens = upload_strided(want, stride)
    for align in (1, 64):
        check_pack(ctx, streams, stride, lens, want, align)


def test_pack_capacity(ctx, oracle):
    want, stride = sizes_mix(oracle)
    streams, lens = upload_strided(want, stride)
    model = offsets([len(s) for s in want], 1)
    for k in (400, 650):                                   # cut in the middle of the large stream / of a tiny one
        cap = int(model[k]) + len(want[k]) // 2
        got = check_pack(ctx, streams, stride, lens, want, 1, capacity=cap)
        assert int(got[-1]) > cap


# ------------------------------------------------------------------ 4: decode_images == decode_batch
@pytest.mark.parametrize("kind", ["photo", "uiflat", "sprite_alpha", "noise"])
@pytest.mark.parametrize("n", [1, 4, 5, 40])
def test_decode_images_equals_decode_batch(api, ctx, oracle, kind, n):
    w, h = 320, 200
    its = [Item(api, oracle, kind if (n < 40 or i % 2) else "uiflat", w, h, 4, frame=i) for i in range(n)]
    ss = (max(len(it.stream) for it in its) + 255) // 256 * 256
    ps = w * h * 4
    streams = filled(n * ss, 0)
    for i, it in enumerate(its):
        streams[i * ss:i * ss + len(it.stream)].copy_(dev(np.frombuffer(it.stream, dtype=np.uint8).copy()))
    a, b = filled(n * ps), filled(n * ps)
    sizes, descs = [len(it.stream) for it in its], [it.desc for it in its]
    ctx.decode_batch(streams.data_ptr(), ss, sizes, descs, 4, a.data_ptr(), ps)
    ctx.decode_images(streams.data_ptr(), [i * ss for i in range(n)], sizes, descs, 4, b.data_ptr(), [i * ps for i in range(n)])
    assert bool((a == b).all())
    for i, it in enumerate(its):
        assert np.array_equal(b[i * ps:(i + 1) * ps].cpu().numpy(), oracle.decode(it.stream, 4)[0]), i


# ------------------------------------------------------------------ 5, 6, 9: packed and tight, unordered, sub-batches
@pytest.mark.parametrize("channels", [0, 3, 4])
def test_decode_images_packed_tight(api, ctx, oracle, channels):
    items = mixed_items(api, oracle)
    assert len(items) >= 40
    decode_tight(ctx, oracle, items, channels)
    decode_tight(ctx, oracle, items, channels, gap=7)


def test_decode_images_three_channel_sources(api, ctx, oracle):
    items = [Item(api, oracle, k, w, h, 3, frame=i) for i, (k, w, h) in enumerate(
        [("photo", 37, 23), ("uiflat", 257, 9), ("noise", 1, 1), ("constant", 64, 48), ("photo", 333, 7), ("sprite_alpha", 1, 97), ("photo", 640, 360)] * 6)]
    for channels in (0, 3, 4):
        decode_tight(ctx, oracle, items, channels)
        decode_tight(ctx, oracle, items, channels, gap=7)


def test_decode_images_unordered(api, ctx, oracle):
    items = mixed_items(api, oracle)
    n = len(items)
    base = decode_tight(ctx, oracle, items, 4)
    rev = list(range(n))[::-1]
    shuf_a = list(np.random.default_rng(11).permutation(n))
    shuf_b = list(np.random.default_rng(12).permutation(n))
    for perm_in, perm_out in [(rev, None), (None, rev), (rev, rev), (shuf_a, shuf_b)]:
        decode_tight(ctx, oracle, items, 4, perm_in=perm_in, perm_out=perm_out)
    assert base is not None


def test_decode_images_sub_batches(api, oracle):
    c = api.Context(0)
    try:
        c.set_decode_record_cap(1 << 20)
        decode_tight(c, oracle, mixed_items(api, oracle), 4)
    finally:
        c.close()


# ------------------------------------------------------------------ 7: hostile streams
def test_decode_images_hostile_streams(api, ctx, oracle, golden, encoded_streams):
    plain = Item(api, oracle, "photo", 64, 48, 4)
    items, want = [plain], [oracle.decode(plain.stream, 4)[0]]
    for case in cases.decode_cases(encoded_streams):
        if not bool(golden[f"dec/{case['name']}/ok"][0]) or case["channels"] not in (0, 4):
            continue
        d = golden[f"dec/{case['name']}/desc"]
        if case["channels"] == 0 and int(d[2]) != 4:
            continue
        it = Item(api, oracle, None, int(d[0]), int(d[1]), int(d[2]), stream=case["stream"])
        it.desc = api.QoiDesc(int(d[0]), int(d[1]), int(d[2]), int(d[3]))
        items.append(it); want.append(golden[f"dec/{case['name']}/pixels"])
        # right behind it a stream whose first chunks would change the picture if a truncated reader took them for its own
        follower = Item(api, oracle, "noise", 9, 5, 4, frame=len(items))
        items.append(follower); want.append(oracle.decode(follower.stream, 4)[0])
    assert len(items) > 100
    blob, so = pack_host([it.stream for it in items])
    d_streams = dev(np.frombuffer(blob, dtype=np.uint8).copy())
    size = [it.w * it.h * 4 for it in items]
    po = [64 + int(x) for x in np.cumsum([0] + size[:-1])]
    out = filled(po[-1] + size[-1] + 64)
    ctx.decode_images(d_streams.data_ptr(), so, [len(it.stream) for it in items], [it.desc for it in items], 4, out.data_ptr(), po)
    got = out.cpu().numpy()
    for i in range(len(items)):
        assert np.array_equal(got[po[i]:po[i] + size[i]], want[i]), i
    assert np.all(got[:64] == GUARD) and np.all(got[po[-1] + size[-1]:] == GUARD)


# ------------------------------------------------------------------ 8: beyond 4 GiB
def test_decode_images_beyond_4gib(api, ctx, oracle):
    big = (4 << 30) + (64 << 20)
    its = [Item(api, oracle, "photo", 640, 360, 4, frame=i) for i in range(3)]
    streams, out = filled(big, 0), filled(big)
    so = [5, (4 << 30) + 12345, (8 << 20) + 1]
    po = [3, (4 << 30) + 777, 640 * 360 * 4 + 9]
    for it, o in zip(its, so):
        streams[o:o + len(it.stream)].copy_(dev(np.frombuffer(it.stream, dtype=np.uint8).copy()))
    ctx.decode_images(streams.data_ptr(), so, [len(it.stream) for it in its], [it.desc for it in its], 4, out.data_ptr(), po)
    sz = 640 * 360 * 4
    for it, o in zip(its, po):
        assert np.array_equal(out[o:o + sz].cpu().numpy(), oracle.decode(it.stream, 4)[0]), o
        assert int(out[o - 1]) == GUARD and int(out[o + sz]) == GUARD


# ------------------------------------------------------------------ 10: round trip
def test_round_trip(api, ctx, oracle):
    import torch
    shapes = [(64, 48, 4), (37, 23, 3), (1, 1, 4), (640, 360, 4), (257, 9, 3), (1, 97, 4), (333, 7, 4)]
    px = [image(("photo", "uiflat", "noise")[i % 3], w, h, ch, frame=i) for i, (w, h, ch) in enumerate(shapes)]
    descs = [api.QoiDesc(w, h, ch, 0) for (w, h, ch) in shapes]
    n = len(shapes)
    pix_off = [int(x) for x in np.cumsum([0] + [p.size for p in px[:-1]])]
    d_px = dev(np.concatenate(px))
    stride = max(api.encode_bound(w, h, ch) for (w, h, ch) in shapes) + 1
    streams, lens = filled(n * stride, 0x3C), torch.zeros(n, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    ctx.encode_images(d_px.data_ptr(), pix_off, descs, streams.data_ptr(), [i * stride for i in range(n)], lens.data_ptr(), st)
    off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    packed = filled(n * stride)
    ctx.pack_streams(streams.data_ptr(), stride, lens.data_ptr(), n, 1, packed.data_ptr(), packed.numel(), off.data_ptr(), st)
    ctx.encode_status(st)
    so, sizes = [int(x) for x in off.cpu().numpy()[:n]], [int(x) for x in lens.cpu().numpy()]
    assert sizes == [len(oracle.encode(p, w, h, ch)) for p, (w, h, ch) in zip(px, shapes)]
    got_descs, bad = ctx.read_descs(packed.data_ptr(), so, sizes)
    assert bad is None
    assert [(d.width, d.height, d.channels, d.colorspace) for d in got_descs] == [(w, h, ch, 0) for (w, h, ch) in shapes]
    # decoded with the headers' channel counts: two calls, one per count (a call shares its output channel count)
    for ch in (3, 4):
        idx = [i for i in range(n) if shapes[i][2] == ch]
        po = [64 + int(x) for x in np.cumsum([0] + [px[i].size for i in idx[:-1]])]
        out = filled(po[-1] + px[idx[-1]].size + 64)
        ctx.decode_images(packed.data_ptr(), [so[i] for i in idx], [sizes[i] for i in idx], [got_descs[i] for i in idx], 0, out.data_ptr(), po)
        got = out.cpu().numpy()
        for k, i in enumerate(idx):
            assert np.array_equal(got[po[k]:po[k] + px[i].size], px[i]), i
        assert np.all(got[:64] == GUARD) and np.all(got[po[-1] + px[idx[-1]].size:] == GUARD)


def test_read_descs_bad_headers(api, ctx, oracle):
    good = Item(api, oracle, "photo", 37, 23, 4).stream
    bad_magic = cases.header(2, 3, 4, 1, magic=b"qoig") + bytes([0xC3]) + cases.END
    zero_w = cases.header(0, 9, 3, 0) + bytes([0xC3]) + cases.END
    streams = [good, bad_magic, good, zero_w]
    blob, so = pack_host(streams)
    d = dev(np.frombuffer(blob, dtype=np.uint8).copy())
    lib = api.load_library()
    n = len(streams)
    descs, first = (api.QoiDesc * n)(), ctypes.c_int(-2)
    rc = lib.qoimi_read_descs(ctx._h, d.data_ptr(), (ctypes.c_size_t * n)(*so), (ctypes.c_int * n)(*[len(s) for s in streams]), n, descs, ctypes.byref(first), None)
    assert rc == E_ARG and first.value == 1 and api.last_error() != ""
    assert [(x.width, x.height, x.channels, x.colorspace) for x in descs] == [(37, 23, 4, 0), (2, 3, 4, 1), (37, 23, 4, 0), (0, 9, 3, 0)]
    got, bad = ctx.read_descs(d.data_ptr(), [so[0], so[2]], [len(good)] * 2)
    assert bad is None and got[1].width == 37
