"""qoimi_encode_packed / qoimi_encode_images_packed on the GPU (-m gpu): pixels in, pack out through bounded staging.  The result is
defined as encode_batch + pack_streams over all streams, so everything is compared with the oracle's streams laid out by the numpy model of
tests/model_cases.py (pack_offsets) - the pack's bytes, both device tables, both host tables, 0xA5 in every gap and around the pack - and
the sub-batch boundaries are forced through staging_bytes by the plan of qoi_amd/packplan.py (the launch count of the append scan says
that the call really ran that many sub-batches)."""
import ctypes

import numpy as np
import pytest
from gpu_pack import E_ARG, GUARD, KINDS, Batch, dev, filled
from gpu_pack import api, ctx, oracle  # noqa: F401  (fixtures)
from model_cases import pack_offsets as offsets


pytestmark = pytest.mark.gpu
FRONT = 256                                  # guard bytes in front of the pack; the pack begins at a 256-aligned address + shift


@pytest.fixture(scope="module")
def equal(api, oracle):
    """13 RGBA images of 64 x 48, classes interleaved: streams from tens of bytes (constant) to near the bound (noise)"""
    b = Batch(api, oracle, [(64, 48, 4)] * 13, [KINDS[i % 5] for i in range(13)])
    assert min(b.lens) < 100 and max(b.lens) > 0.95 * b.bounds[0]
    return b


@pytest.fixture(scope="module")
def mixed(api, oracle):
    shapes = [(1, 1, 4), (1, 97, 4), (131, 1, 3), (37, 23, 3), (257, 9, 4), (64, 48, 3), (333, 7, 4), (130, 70, 4), (130, 70, 3)]
    return Batch(api, oracle, shapes, [KINDS[(i + 2) % 5] for i in range(len(shapes))])


def run(ctx, b, align, staging, shift=0, capacity=None, null_dest=False, is_mixed=False):
    """One call on batch b; checks tables, bytes, guards, the number of sub-batches.  Returns (offsets, sizes) as the call gave them."""
    import torch
    from qoi_amd.packplan import plan
    model = offsets(b.lens, align)
    cap = int(model[-1]) if capacity is None else capacity
    buf = filled(FRONT + shift + cap + 512)
    assert buf.data_ptr() % 256 == 0
    view = buf[FRONT + shift:]
    off = torch.full((b.n + 1,), -1, dtype=torch.int64, device="cuda")
    lens = torch.full((b.n,), -1, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    dest = 0 if null_dest else view.data_ptr()
    ctx.set_profiling(True)
    if is_mixed:
        got_off, got_len = ctx.encode_images_packed(b.d_px.data_ptr(), b.pix_off, b.descs, align, dest, cap, off.data_ptr(), lens.data_ptr(), staging, st)
    else:
        ps = b.px[0].size
        got_off, got_len = ctx.encode_packed(b.d_px.data_ptr(), ps, b.descs[0], b.n, align, dest, cap, off.data_ptr(), lens.data_ptr(), staging, st)
    prof = ctx.get_profile(st)
    ctx.set_profiling(False)
    what = (align, staging, shift, cap)
    assert got_len.tolist() == b.lens, what
    assert np.array_equal(got_off, model), (what, got_off, model)
    assert np.array_equal(off.cpu().numpy().astype(np.uint64), model), what
    assert lens.cpu().numpy().tolist() == b.lens, what
    subs = plan(b.bounds, staging)
    assert prof["pack_offsets_append"][1] == len(subs), (what, prof["pack_offsets_append"], subs)
    assert prof["pack_copy_append"][1] == (len(subs) if cap else 0), (what, prof["pack_copy_append"], subs)
    assert prof["pack_offsets"][1] == 0 and prof["pack_copy"][1] == 0
    got = buf.cpu().numpy()
    mask = np.ones(got.size, dtype=bool)
    base = FRONT + shift
    for i, s in enumerate(b.want):
        a, e = int(model[i]), int(model[i]) + len(s)
        if e > cap:
            continue                                       # does not fit wholly: not copied, not in part
        assert got[base + a:base + e].tobytes() == s, (what, i, len(s))
        mask[base + a:base + e] = False
    assert np.all(got[mask] == GUARD), (what, "a byte outside the streams was written", int(np.argmax(mask & (got != GUARD))) - base)
    ctx.encode_status(st)                                  # OK, and nothing is encoded again
    return got_off, got_len


# ------------------------------------------------------------------ 1: sub-batch boundaries
@pytest.mark.parametrize("align", [1, 4, 16, 256])
@pytest.mark.parametrize("slots", [1, 2, 5, 13, 40])
def test_sub_batch_boundaries(ctx, equal, align, slots):
    from qoi_amd.packplan import plan, slot
    staging = slots * slot(equal.bounds[0])
    want_subs = {1: 13, 2: 7, 5: 3, 13: 1, 40: 1}[slots]
    assert len(plan(equal.bounds, staging)) == want_subs
    run(ctx, equal, align, staging)


def test_staging_requests_below_one_slot_and_default(ctx, equal):
    run(ctx, equal, 1, 1)                                  # raised to one slot: 13 sub-batches
    before = ctx.workspace_bytes()["encode"]
    import torch
    off = torch.zeros(equal.n + 1, dtype=torch.int64, device="cuda")
    lens = torch.zeros(equal.n, dtype=torch.int32, device="cuda")
    ctx.set_profiling(True)                                # 0 selects the default, far above 13 small slots: one sub-batch, and no arena of that size
    got_off, got_len = ctx.encode_packed(equal.d_px.data_ptr(), equal.px[0].size, equal.descs[0], equal.n, 1, 0, 0, off.data_ptr(), lens.data_ptr(), 0, 0)
    assert ctx.get_profile(0)["pack_offsets_append"][1] == 1
    ctx.set_profiling(False)
    assert got_len.tolist() == equal.lens and np.array_equal(got_off, offsets(equal.lens, 1))
    assert ctx.workspace_bytes()["encode"] < before + (16 << 20)


# ------------------------------------------------------------------ 2: destination misaligned
@pytest.mark.parametrize("shift", [1, 3, 7])
def test_destination_misaligned(ctx, equal, shift):
    """align 1, one image per sub-batch: every sub-batch boundary falls inside a 16-byte granule of the destination address"""
    from qoi_amd.packplan import slot
    model = offsets(equal.lens, 1)
    assert any((int(o) + shift) % 16 for o in model[1:-1])
    run(ctx, equal, 1, slot(equal.bounds[0]), shift=shift)
    run(ctx, equal, 1, 2 * slot(equal.bounds[0]), shift=shift)


# ------------------------------------------------------------------ 3: capacity
def test_capacity(ctx, equal):
    from qoi_amd.packplan import plan, slot
    staging = 2 * slot(equal.bounds[0])
    for align in (1, 16):
        model = offsets(equal.lens, align)
        exact = int(model[-1])
        run(ctx, equal, align, staging, capacity=0, null_dest=True)           # tables only
        run(ctx, equal, align, staging, capacity=0)
        run(ctx, equal, align, staging, capacity=exact)
        got_off, _ = run(ctx, equal, align, staging, capacity=exact - 1, shift=5)      # the last stream is absent
        assert int(got_off[-1]) == exact > exact - 1
        # ends inside stream 5 (noise, long), the first of the middle sub-batch (4, 2): 5 and everything behind it is absent - stream 6
        # (constant, tens of bytes) is shorter than what is left of the capacity, and is still judged by its own off + len <= cap
        assert (4, 2) in plan(equal.bounds, staging)
        cap = int(model[5]) + equal.lens[5] // 2
        assert equal.lens[6] < cap - int(model[5]) and int(model[6]) + equal.lens[6] > cap
        got_off, got_len = run(ctx, equal, align, staging, capacity=cap, shift=3)
        assert int(got_off[-1]) > cap
        # ... and inside stream 6, the second of that sub-batch, with one image per sub-batch as well
        cap = int(model[6]) + equal.lens[6] // 2
        run(ctx, equal, align, staging, capacity=cap, shift=9)
        run(ctx, equal, align, slot(equal.bounds[0]), capacity=cap, shift=9)


# ------------------------------------------------------------------ 4: mixed shapes
def test_mixed_shapes(ctx, mixed):
    from qoi_amd.packplan import plan, slot
    slots = [slot(x) for x in mixed.bounds]
    staging = 20000
    subs = plan(mixed.bounds, staging)
    assert len({c for _, c in subs}) >= 2, subs            # sub-batches of different counts
    assert max(slots) > staging                            # one image's slot alone exceeds the request
    assert {d.channels for d in mixed.descs} == {3, 4}
    for align in (1, 16, 256):
        run(ctx, mixed, align, staging, is_mixed=True)
    run(ctx, mixed, 1, staging, shift=7, is_mixed=True)
    run(ctx, mixed, 4, 30000, shift=1, is_mixed=True)
    run(ctx, mixed, 1, 1, shift=3, is_mixed=True)          # one image per sub-batch
    run(ctx, mixed, 64, 1 << 20, is_mixed=True)            # one sub-batch
    model = offsets(mixed.lens, 1)
    run(ctx, mixed, 1, staging, capacity=int(model[7]) + mixed.lens[7] // 2, shift=2, is_mixed=True)
    run(ctx, mixed, 1, staging, capacity=0, null_dest=True, is_mixed=True)


# ------------------------------------------------------------------ 5: round trip
def test_round_trip(ctx, equal):
    import torch
    from qoi_amd.packplan import slot
    n, ps = equal.n, equal.px[0].size
    cap = int(offsets(equal.lens, 4)[-1])
    packed = filled(cap + 64)
    off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    lens = torch.zeros(n, dtype=torch.int32, device="cuda")
    so, sizes = ctx.encode_packed(equal.d_px.data_ptr(), ps, equal.descs[0], n, 4, packed.data_ptr(), cap, off.data_ptr(), lens.data_ptr(), 3 * slot(equal.bounds[0]))
    assert int(so[-1]) == cap
    descs, bad = ctx.read_descs(packed.data_ptr(), so[:n], sizes)             # the host tables, as they came
    assert bad is None and all((d.width, d.height, d.channels, d.colorspace) == (64, 48, 4, 0) for d in descs)
    infos, flagged = ctx.inspect_streams(packed.data_ptr(), so[:n], sizes)
    assert flagged is None and not infos["flags"].any() and infos["pixels"].tolist() == [64 * 48] * n
    out = filled(64 + n * ps + 64)
    ctx.decode_images(packed.data_ptr(), so[:n], sizes, descs, 0, out.data_ptr(), [64 + i * ps for i in range(n)])
    got = out.cpu().numpy()
    assert np.array_equal(got[64:64 + n * ps], np.concatenate(equal.px))
    assert np.all(got[:64] == GUARD) and np.all(got[64 + n * ps:] == GUARD)


# ------------------------------------------------------------------ 6: rejections
def test_rejections(api, ctx, equal):
    import torch
    lib = api.load_library()
    n, ps = 2, equal.px[0].size
    packed, off, lens = filled(65536), filled(8 * (n + 1)), filled(4 * n)
    h, X, P, O, L = ctx._h, equal.d_px.data_ptr(), packed.data_ptr(), off.data_ptr(), lens.data_ptr()
    good = api.QoiDesc(64, 48, 4, 0)
    ds = (api.QoiDesc * n)(good, good)
    bad_ds = (api.QoiDesc * n)(good, api.QoiDesc(64, 48, 5, 0))
    po = (ctypes.c_size_t * n)(0, ps)
    h_off = (ctypes.c_ulonglong * (n + 1))(*([7] * (n + 1)))
    h_len = (ctypes.c_int * n)(*([7] * n))
    cap = packed.numel()

    def eq(ctx_=h, px=X, stride=ps, desc=good, n_=n, align=1, dest=P, cap_=cap, o=O, l=L):
        return lib.qoimi_encode_packed(ctx_, px, stride, ctypes.byref(desc) if desc is not None else None, n_, align, dest, cap_, o, l, 0, h_off, h_len, None)

    def mx(ctx_=h, px=X, offs=po, descs=ds, n_=n, align=1, dest=P, cap_=cap, o=O, l=L):
        return lib.qoimi_encode_images_packed(ctx_, px, offs, descs, n_, align, dest, cap_, o, l, 0, h_off, h_len, None)

    calls = {
        "NULL ctx": lambda: eq(ctx_=None), "NULL pixels": lambda: eq(px=None), "NULL desc": lambda: eq(desc=None),
        "NULL offset table": lambda: eq(o=None), "NULL length table": lambda: eq(l=None),
        "n 0": lambda: eq(n_=0), "n -1": lambda: eq(n_=-1),
        "align 0": lambda: eq(align=0), "align 3": lambda: eq(align=3), "align 512": lambda: eq(align=512),
        "descriptor: channels 5": lambda: eq(desc=api.QoiDesc(64, 48, 5, 0)), "descriptor: width 0": lambda: eq(desc=api.QoiDesc(0, 48, 4, 0)),
        "descriptor: pixel cap": lambda: eq(desc=api.QoiDesc(20000, 20000, 4, 0)),
        "pixel_stride below one image": lambda: eq(stride=ps - 1),
        "NULL destination with capacity": lambda: eq(dest=None),
        "images: NULL ctx": lambda: mx(ctx_=None), "images: NULL pixels": lambda: mx(px=None), "images: NULL pixel offsets": lambda: mx(offs=None),
        "images: NULL descs": lambda: mx(descs=None), "images: NULL offset table": lambda: mx(o=None), "images: NULL length table": lambda: mx(l=None),
        "images: n 0": lambda: mx(n_=0), "images: align 6": lambda: mx(align=6), "images: align 1024": lambda: mx(align=1024),
        "images: descriptor": lambda: mx(descs=bad_ds), "images: NULL destination with capacity": lambda: mx(dest=None),
    }
    retries = ctx.encode_retries()
    for name, call in calls.items():
        assert call() == E_ARG, name
        assert api.last_error() != "", name
    torch.cuda.synchronize()
    for buf in (packed, off, lens):
        assert bool((buf == GUARD).all()), "a rejected call wrote to the caller's buffers"
    assert list(h_off) == [7] * (n + 1) and list(h_len) == [7] * n
    ctx.encode_status(0)
    assert ctx.encode_retries() == retries
    # the host tables may be NULL
    off2 = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    len2 = torch.zeros(n, dtype=torch.int32, device="cuda")
    assert lib.qoimi_encode_packed(h, X, ps, ctypes.byref(good), n, 1, P, cap, off2.data_ptr(), len2.data_ptr(), 0, None, None, None) == 0
    assert len2.cpu().numpy().tolist() == equal.lens[:n] and off2.cpu().numpy().tolist() == offsets(equal.lens[:n], 1).tolist()


# ------------------------------------------------------------------ 7: memory, and streams of many tiles
def test_staging_bounds_the_memory(api, oracle):
    """16 RGBA images of 512 x 512 through 2 slots: the context holds the workspace of a 2-image encode plus the staging - nowhere
    near the 16 strided streams a caller of encode_batch must own (the arenas' own slack is a quarter plus 1 MiB: 2 slots stay far
    below half of 16 strides, an arena sized by all 16 would not)."""
    import torch
    from qoi_amd.packplan import plan, slot
    w = h = 512
    n, ps = 16, w * h * 4
    S = slot(api.encode_bound(w, h, 4))
    b = Batch(api, oracle, [(w, h, 4)] * n, ["noise" if i % 4 == 0 else "photo" for i in range(n)])
    assert max(b.lens) > 64 * 16384                        # streams of many copy tiles
    a, c = api.Context(0), api.Context(0)
    try:
        streams, lens2 = filled(2 * S, 0), torch.zeros(2, dtype=torch.int32, device="cuda")
        a.encode_batch(b.d_px.data_ptr(), ps, b.descs[0], 2, streams.data_ptr(), S, lens2.data_ptr(), 0)
        a.encode_status(0)
        base = a.workspace_bytes()["encode"]
        assert len(plan(b.bounds, 2 * S)) == 8
        run(c, b, 64, 2 * S, shift=11)
        held = c.workspace_bytes()["encode"]
        assert held < base + 16 * S // 2, (held, base, S)
        assert held >= base + 2 * S, (held, base, S)       # the staging arena is counted
    finally:
        a.close(); c.close()


# ------------------------------------------------------------------ 8: existing calls unaffected
def test_existing_calls_unaffected(api, ctx, equal):
    import torch
    from qoi_amd.packplan import slot
    n, ps = equal.n, equal.px[0].size
    stride = equal.bounds[0] + 1
    model = offsets(equal.lens, 1)
    cap = int(model[-1])
    st = torch.cuda.current_stream().cuda_stream

    def two_calls():
        streams, lens = filled(n * stride, 0x3C), torch.zeros(n, dtype=torch.int32, device="cuda")
        packed, off = filled(cap + 64), torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        ctx.encode_batch(equal.d_px.data_ptr(), ps, equal.descs[0], n, streams.data_ptr(), stride, lens.data_ptr(), st)
        ctx.pack_streams(streams.data_ptr(), stride, lens.data_ptr(), n, 1, packed.data_ptr(), cap, off.data_ptr(), st)
        ctx.encode_status(st)
        return packed.cpu().numpy(), off.cpu().numpy(), lens.cpu().numpy()

    before = two_calls()
    run(ctx, equal, 1, 2 * slot(equal.bounds[0]))
    after = two_calls()
    for x, y in zip(before, after):
        assert np.array_equal(x, y)
    assert before[0][:cap].tobytes() == b"".join(equal.want) and np.all(before[0][cap:] == GUARD)
    assert before[2].tolist() == equal.lens and np.array_equal(before[1].astype(np.uint64), model)


# ------------------------------------------------------------------ 9: sub-batches of more streams than one tile of the scan
def test_many_tiny_streams(api, ctx, oracle):
    """16400 images of 1 x 1 in sub-batches of 8195: the seeded scan runs over more than one tile of 8192 lengths, a copy tile holds
    hundreds of streams, and hardly a granule lies inside one stream."""
    import torch
    from qoi_amd.packplan import plan
    n = 16400
    px = np.zeros((n, 4), dtype=np.uint8)
    i = np.arange(n)
    px[:, 0], px[:, 1], px[:, 2], px[:, 3] = i & 255, (i >> 8) & 255, 200, np.where(i % 3 == 0, 255, 77)
    px[i % 7 == 0] = (0, 0, 0, 255)                        # the start value: a run, 23 bytes
    want = [oracle.encode(px[k], 1, 1, 4) for k in range(n)]
    lens_want = [len(s) for s in want]
    assert len(set(lens_want)) >= 3
    staging = 8195 * 256
    assert plan([api.encode_bound(1, 1, 4)] * n, staging) == [(0, 8195), (8195, 8195), (16390, 10)]
    d_px = dev(px.reshape(-1))
    for align, shift in ((1, 5), (8, 0)):
        model = offsets(lens_want, align)
        cap = int(model[-1])
        buf = filled(FRONT + shift + cap + 256)
        off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        lens = torch.zeros(n, dtype=torch.int32, device="cuda")
        got_off, got_len = ctx.encode_packed(d_px.data_ptr(), 4, api.QoiDesc(1, 1, 4, 0), n, align, buf[FRONT + shift:].data_ptr(), cap,
                                             off.data_ptr(), lens.data_ptr(), staging)
        assert got_len.tolist() == lens_want and np.array_equal(got_off, model)
        assert np.array_equal(off.cpu().numpy().astype(np.uint64), model)
        expect = np.full(buf.numel(), GUARD, dtype=np.uint8)
        for k, s in enumerate(want):
            a = FRONT + shift + int(model[k])
            expect[a:a + len(s)] = np.frombuffer(s, dtype=np.uint8)
        got = buf.cpu().numpy()
        assert np.array_equal(got, expect), (align, int(np.argmax(got != expect)) - FRONT - shift)
