"""qoimi_inspect_streams on the GPU (-m gpu): every expectation is streaminfo.inspect_stream, the plain-Python model of the walk and
the flags.  The streams of a test go into ONE call, packed back to back on the host (align 1), so blocks of different streams, tiny
and large ones, sit side by side in the kernels' tables."""
import ctypes

import numpy as np
import pytest

import cases
from qoi_amd import streaminfo as si
from gpu_calls import assert_info
from gpu_pack import E_ARG, dev
from gpu_pack import api, ctx, oracle  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
BLOCK = 16384          # bytes of a stream's body one wavefront takes (qoi_inspect.hip: kInsBlock)


def image(kind, w, h, ch, frame=0):
    from qoi_amd import synth
    return (synth.frame_rgba if ch == 4 else synth.frame_rgb)(kind, w, h, frame).reshape(-1)


def pack_host(streams):
    offs, blob = [], bytearray()
    for s in streams:
        offs.append(len(blob))
        blob += s
    return bytes(blob), offs


def check_call(ctx, streams, sizes=None, order=None, models=None, stream=0):
    """One inspect_streams call on `streams` packed back to back (listed in `order`); every info against the model."""
    n = len(streams)
    sizes = [len(s) for s in streams] if sizes is None else sizes
    models = [si.inspect_stream(s, z) for s, z in zip(streams, sizes)] if models is None else models
    blob, offs = pack_host(streams)
    d = dev(np.frombuffer(blob + b"\x5c", dtype=np.uint8).copy())
    order = list(range(n)) if order is None else order
    infos, first = ctx.inspect_streams(d.data_ptr(), [offs[i] for i in order], [sizes[i] for i in order], stream)
    assert infos.dtype == si.INFO_DTYPE and len(infos) == n
    for k, i in enumerate(order):
        assert_info(infos[k], models[i], (k, i, sizes[i]))
    flagged = [k for k, i in enumerate(order) if models[i]["flags"]]
    assert first == (flagged[0] if flagged else None)
    return infos, models


# ------------------------------------------------------------------ 1: reference streams, mixed shapes
@pytest.fixture(scope="module")
def mixed(oracle):
    """The 44 images of test_gpu_packed.py::mixed_items (its shape and kind lists), every third one 3-channel: (stream, w, h, ch) and
    the model's infos, computed once."""
    shapes = [(1, 1), (1, 97), (131, 1), (37, 23), (257, 9), (64, 48), (333, 7), (640, 360), (5, 5), (101, 77), (1920, 3)]
    kinds = ["photo", "uiflat", "sprite_alpha", "noise", "constant"]
    items = []
    for i in range(43):
        w, h = shapes[i % len(shapes)]
        ch = 3 if i % 3 == 2 else 4
        items.append((oracle.encode(image(kinds[i % len(kinds)], w, h, ch, frame=i), w, h, ch), w, h, ch))
    items.insert(20, (oracle.encode(image("photo", 1024, 1024, 4, frame=3), 1024, 1024, 4), 1024, 1024, 4))
    return items, [si.inspect_stream(s) for (s, _, _, _) in items]


def test_reference_streams_mixed_shapes(ctx, mixed):
    items, models = mixed
    assert len(items) == 44
    order = [int(x) for x in np.random.default_rng(21).permutation(len(items))]
    infos, _ = check_call(ctx, [s for (s, _, _, _) in items], order=order, models=models)
    assert not infos["flags"].any()
    for k, i in enumerate(order):
        assert int(infos[k]["pixels"]) == items[i][1] * items[i][2] and int(infos[k]["walk_end"]) == len(items[i][0]) - 8


# ------------------------------------------------------------------ 2: hostile and dense streams
def test_hostile_streams(ctx, encoded_streams):
    cs = cases.decode_cases(encoded_streams)
    streams = [c["stream"] for c in cs]
    sizes = [len(c["stream"]) if c["size"] is None else c["size"] for c in cs]
    _, models = check_call(ctx, streams, sizes=sizes)
    seen = 0
    for m in models:
        seen |= m["flags"]
    assert seen == 127                                   # every flag occurs among them


@pytest.mark.parametrize("family", ["dense", "pairs", "flat"])
def test_dense_streams(ctx, family):
    if family == "dense":
        streams = [s for (_, _, s, _, _) in cases.dense_record_streams()]
    else:
        streams = [s for (_, s, _, _) in (cases.pair_streams() if family == "pairs" else cases.flat_run_streams())]
    assert len(streams) >= 6
    check_call(ctx, streams)


# ------------------------------------------------------------------ 3: phases that never synchronise
def test_phases_never_synchronise(ctx):
    lengths = list(range(61, 70)) + list(range(4093, 4100)) + [5 * 4096 + r for r in range(5)] + list(range(BLOCK - 3, BLOCK + 4))
    streams = []
    for n in lengths:
        for unit in (b"\xff", b"\xfe", b"\xbf\xff", b"\xfe\xff"):
            streams.append(cases.header(640, 360) + (unit * n)[:n] + cases.END)
    for seed in range(8):
        body = np.random.default_rng(300 + seed).integers(0, 256, size=300000, dtype=np.uint8).tobytes()
        streams.append(cases.header(640, 360) + body + cases.END)
    check_call(ctx, streams)


# ------------------------------------------------------------------ 4: region lengths at the edges
def test_region_lengths(ctx, oracle):
    rng = np.random.default_rng(5)
    full = oracle.encode(rng.integers(0, 256, size=64 * 64 * 4, dtype=np.uint8), 64, 64, 4)
    assert len(full) > 22 + 4097
    lengths = list(range(0, 7)) + [63, 64, 65, 4095, 4096, 4097]
    streams = [full[:14 + n] + cases.END for n in lengths]
    assert [len(s) for s in streams] == [22 + n for n in lengths]
    _, models = check_call(ctx, streams)
    assert any(m["flags"] & si.SI_LAST_CHUNK_CUT for m in models)          # an RGBA chunk of the noise cut by the end marker


# ------------------------------------------------------------------ 5: repeated INDEX across edges
def test_repeated_index_across_edges(ctx):
    streams = []
    for shift in range(5):
        body = bytearray(0x15 if k % 2 == 0 else 0x2A for k in range(8192))
        for k in (63, 64, 65, 255, 256, 4095, 4096, 4097):
            body[k] = body[k - 1]
        streams.append(cases.header(128, 64) + b"\xc0" * shift + bytes(body) + cases.END)
    for shift in range(5):                                                  # ... and across the edge between two blocks
        body = bytearray(0x15 if k % 2 == 0 else 0x2A for k in range(2 * BLOCK + 100))
        for k in (BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK):
            body[k] = body[k - 1]
        streams.append(cases.header(128, 64) + b"\xc0" * shift + bytes(body) + cases.END)
    _, models = check_call(ctx, streams)
    assert all(m["repeat_index"] >= 4 for m in models)


# ------------------------------------------------------------------ 6: placement
def test_placement(ctx, oracle):
    s = oracle.encode(image("uiflat", 257, 9, 4), 257, 9, 4)
    want = si.inspect_stream(s)
    assert want["flags"] == 0
    pitch = (len(s) + 15) // 16 * 16 + 16
    offs = [k * pitch + k for k in range(16)]                               # 16 copies in one buffer, start addresses at 16 consecutive alignments
    buf = bytearray(b"\x5c" * (16 * pitch + 64))
    for o in offs:
        buf[o:o + len(s)] = s
    listed = offs + [offs[6], offs[9]]                                      # ... two of them listed twice: ranges that coincide
    d = dev(np.frombuffer(bytes(buf), dtype=np.uint8).copy())
    infos, first = ctx.inspect_streams(d.data_ptr(), listed, [len(s)] * len(listed))
    assert first is None and len(infos) == 18
    for k in range(len(listed)):
        assert_info(infos[k], want, k)
    assert np.all(infos == infos[0])


# ------------------------------------------------------------------ 7: rejections and trivia
def test_rejections_and_trivia(api, ctx, oracle):
    lib = api.load_library()
    good = oracle.encode(image("photo", 37, 23, 4), 37, 23, 4)
    bad_magic = cases.header(2, 3, 4, 1, magic=b"qoig") + bytes([0xC3, 0x15, 0xFE, 1, 2, 3]) + cases.END
    zero_w = cases.header(0, 9, 3, 0) + bytes([0xC3]) + cases.END
    ch5 = cases.header(2, 2, 5) + bytes([0xC3, 0x40]) + cases.END
    streams = [good, b"", good[:1], good[:21], bad_magic, zero_w, ch5]
    infos, models = check_call(ctx, streams)
    for k in (1, 2, 3):
        assert int(infos[k]["flags"]) == si.SI_TOO_SHORT and int(infos[k]["pixels"]) == 0 and int(infos[k]["walk_end"]) == 0 and not infos[k]["ops"].any()
    for k in (4, 5, 6):
        assert int(infos[k]["flags"]) & si.SI_HEADER_BAD and int(infos[k]["pixels"]) > 0 and int(infos[k]["walk_end"]) == len(streams[k]) - 8
    assert int(infos[4]["flags"]) == si.SI_HEADER_BAD                      # no pixel comparison without a header
    # n_streams = 0
    d = dev(np.frombuffer(good, dtype=np.uint8).copy())
    first = ctypes.c_int(7)
    none = (api.StreamInfo * 1)()
    assert lib.qoimi_inspect_streams(ctx._h, d.data_ptr(), (ctypes.c_size_t * 1)(0), (ctypes.c_int * 1)(0), 0, none, ctypes.byref(first), None) == 0
    assert first.value == -1
    assert lib.qoimi_inspect_streams(ctx._h, None, (ctypes.c_size_t * 1)(0), (ctypes.c_int * 1)(0), 0, none, None, None) == 0
    # rejected calls leave infos_out as it was
    out = np.full(2 * 64, 0xA5, dtype=np.uint8)
    p_out = out.ctypes.data_as(ctypes.POINTER(api.StreamInfo))
    so, sz = (ctypes.c_size_t * 2)(0, 0), (ctypes.c_int * 2)(len(good), len(good))
    neg = (ctypes.c_int * 2)(len(good), -1)
    D = d.data_ptr()
    calls = {
        "negative size": lambda: lib.qoimi_inspect_streams(ctx._h, D, so, neg, 2, p_out, None, None),
        "NULL offsets": lambda: lib.qoimi_inspect_streams(ctx._h, D, None, sz, 2, p_out, None, None),
        "NULL sizes": lambda: lib.qoimi_inspect_streams(ctx._h, D, so, None, 2, p_out, None, None),
        "NULL infos": lambda: lib.qoimi_inspect_streams(ctx._h, D, so, sz, 2, None, None, None),
        "NULL ctx": lambda: lib.qoimi_inspect_streams(None, D, so, sz, 2, p_out, None, None),
        "NULL streams": lambda: lib.qoimi_inspect_streams(ctx._h, None, so, sz, 2, p_out, None, None),
        "n -1": lambda: lib.qoimi_inspect_streams(ctx._h, D, so, sz, -1, p_out, None, None),
    }
    for name, call in calls.items():
        assert call() == E_ARG, name
        assert api.last_error() != "", name
        assert np.all(out == 0xA5), name
    check_call(ctx, [good, good])


# ------------------------------------------------------------------ 8: many tiny streams
def test_many_tiny_streams(ctx, oracle):
    size22 = cases.header(5, 3) + cases.END
    small = oracle.encode(image("photo", 5, 3, 4), 5, 3, 4)
    models = [si.inspect_stream(size22), si.inspect_stream(small)]
    assert models[1]["flags"] == 0
    n = 20000
    blob = (size22 + small) * n
    offs = np.arange(2 * n, dtype=np.int64) // 2 * (len(size22) + len(small)) + (np.arange(2 * n) % 2) * len(size22)
    sizes = np.where(np.arange(2 * n) % 2 == 0, len(size22), len(small))
    d = dev(np.frombuffer(blob + b"\x5c", dtype=np.uint8).copy())
    infos, first = ctx.inspect_streams(d.data_ptr(), offs, sizes)
    assert first == 0
    for parity in (0, 1):
        want = si.info_record(models[parity])
        got = infos[parity::2]
        assert len(got) == n and np.all(got == want), (parity, got[got != want][:1], want)


# ------------------------------------------------------------------ 9: the product's round trip
def test_round_trip_of_our_encoder(api, ctx):
    import torch
    w, h, n = 640, 360, 8
    desc = api.QoiDesc(w, h, 4, 0)
    ps = w * h * 4
    px = dev(np.concatenate([image("photo" if i % 2 == 0 else "sprite_alpha", w, h, 4, frame=i) for i in range(n)]))
    stride = api.encode_bound(w, h, 4) + 1
    streams = torch.full((n * stride,), 0x3C, dtype=torch.uint8, device="cuda")
    lens = torch.zeros(n, dtype=torch.int32, device="cuda")
    off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    packed = torch.full((n * stride,), 0x5C, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    ctx.encode_batch(px.data_ptr(), ps, desc, n, streams.data_ptr(), stride, lens.data_ptr(), st)
    ctx.pack_streams(streams.data_ptr(), stride, lens.data_ptr(), n, 1, packed.data_ptr(), packed.numel(), off.data_ptr(), st)
    ctx.encode_status(st)
    so, sizes = [int(x) for x in off.cpu().numpy()[:n]], [int(x) for x in lens.cpu().numpy()]
    host = packed.cpu().numpy().tobytes()
    infos, first = ctx.inspect_streams(packed.data_ptr(), so, sizes)
    assert first is None and not infos["flags"].any()
    for i in range(n):
        assert_info(infos[i], si.inspect_stream(host[so[i]:so[i] + sizes[i]]), i)
        assert int(infos[i]["pixels"]) == 230400 and int(infos[i]["walk_end"]) == sizes[i] - 8 and int(infos[i]["repeat_index"]) == 0
    cut = list(sizes)
    cut[3] -= 9
    want3 = si.inspect_stream(host[so[3]:so[3] + cut[3]])
    assert want3["flags"] & ~si.SI_LAST_CHUNK_CUT == si.SI_PIXELS_SHORT | si.SI_NO_END_MARKER
    again, first = ctx.inspect_streams(packed.data_ptr(), so, cut)
    assert first == 3
    assert_info(again[3], want3, "cut")
    keep = [i for i in range(n) if i != 3]
    assert np.all(again[keep] == infos[keep])


# ------------------------------------------------------------------ 10: beside decode calls on one context
def test_beside_decode_calls(api, oracle, mixed):
    import torch
    items, models = mixed
    items4 = [(s, w, h, ch) for (s, w, h, ch) in items]
    c = api.Context(0)
    try:
        blob, so = pack_host([s for (s, _, _, _) in items4])
        d = dev(np.frombuffer(blob + b"\x5c", dtype=np.uint8).copy())
        sizes = [len(s) for (s, _, _, _) in items4]
        descs = [api.QoiDesc(w, h, ch, 0) for (_, w, h, ch) in items4]
        nbytes = [w * h * 4 for (_, w, h, _) in items4]
        po = [64 + int(x) for x in np.cumsum([0] + nbytes[:-1])]
        want = [oracle.decode(s, 4)[0] for (s, _, _, _) in items4]
        side = torch.cuda.Stream()
        torch.cuda.synchronize()

        def decode():
            out = torch.full((po[-1] + nbytes[-1] + 64,), 0xA5, dtype=torch.uint8, device="cuda")
            c.decode_images(d.data_ptr(), so, sizes, descs, 4, out.data_ptr(), po)
            got = out.cpu().numpy()
            for i in range(len(items4)):
                assert np.array_equal(got[po[i]:po[i] + nbytes[i]], want[i]), i

        decode()
        infos, first = c.inspect_streams(d.data_ptr(), so, sizes, side.cuda_stream)
        assert first is None
        for i in range(len(items4)):
            assert_info(infos[i], models[i], i)
        decode()
    finally:
        c.close()
