"""qoimi_pack_streams on the GPU (-m gpu) where tests/test_gpu_packed.py leaves the high halves zero: offsets whose 64-bit sums pass 2**32
inside a thread of pack_offsets, between two lanes, between two wavefronts and between two tiles, lengths outside [0, stride] (clamped,
include/qoi_mi355x.h), and a pack longer than 4 GiB with real streams beyond offset 2**32 that are then read by qoimi_read_descs,
qoimi_inspect_streams and qoimi_decode_images.  The model is tests/test_packed_api.py: offsets on the clamped lengths; every test asserts
from the model that its lengths put the sums where it says.  Every comparison is exact."""
import numpy as np
import pytest

from qoi_amd import streaminfo as si
from gpu_calls import assert_info
from gpu_pack import GUARD, Item, dev, filled
from gpu_pack import api, ctx, oracle  # noqa: F401  (fixtures)
from model_cases import pack_offsets as offsets

pytestmark = pytest.mark.gpu
B32 = 1 << 32
INT_MAX, INT_MIN = (1 << 31) - 1, -(1 << 31)
STRIDE_MAX = 0x7FFFFFFF + 256          # the largest stride qoimi_pack_streams takes
N = 2 * 8192 + 5                       # two tiles of pack_offsets and five lengths of a third


def clamp(lens, stride):
    """a length as the pack takes it (qoi_pack.hip: pack_len)"""
    return np.clip(np.asarray(lens, dtype=np.int64), 0, stride)


# ------------------------------------------------------------------ 1: offsets only
BIG = INT_MAX - 256                    # two of them stay below 2**32 at every align, a third passes it
QUIET = [0, -1, INT_MIN, -5, 0]        # lengths that add nothing: empty streams and negative ones (clamped to 0)


def lengths(where, seed):
    """N seeded lengths in [INT_MIN, INT_MAX].  The running sum of the rounded, clamped lengths first reaches 2**32 ...
      thread: behind three lengths of thread 0 (offset 3)
      lane:   where lane 1 adds its sum to lane 0's (offset 9: both sums are below 2**32)
      wave:   where wavefront 1 adds the sum of wavefront 0 (offset 513)
      tile:   where the second tile adds the sum of the first (offset 8193)
    Behind that point the lengths are random over the whole range of an int, with planted extremes and negative ones."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, INT_MAX, size=N, endpoint=True).astype(np.int64)
    lens[rng.integers(0, N, size=400)] = rng.choice(np.array([0, 1, INT_MAX, -1, INT_MIN, -77, INT_MAX - 1, 255, 256, 257], dtype=np.int64), size=400)
    quiet = {"thread": 0, "lane": 8, "wave": 512, "tile": 8192}[where]
    lens[:quiet + 1] = rng.choice(np.array(QUIET, dtype=np.int64), size=quiet + 1)
    if where == "thread":
        lens[0:3] = BIG
    else:
        lens[0:2] = BIG
        lens[quiet] = 600
    return lens, (3 if where == "thread" else quiet + 1)


def run_offsets(ctx, lens, stride, align):
    """Offsets only: packed_capacity 0, d_packed NULL.  The source is never read in such a call - launch_pack_streams launches pack_copy only
    for a capacity other than 0, and pack_offsets takes the lengths, not the streams - so d_streams is any non-NULL device address and the
    stride may be one no allocation could back."""
    import torch
    n = len(lens)
    d_lens = dev(np.asarray(lens, dtype=np.int32))
    off = torch.full((n + 2,), -1, dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    ctx.pack_streams(d_lens.data_ptr(), stride, d_lens.data_ptr(), n, align, 0, 0, off.data_ptr(), st)
    ctx.encode_status(st)
    got = off.cpu().numpy()
    assert got[n + 1] == -1, "written behind the n + 1 offsets"
    return got[:n + 1].view(np.uint64)


@pytest.mark.parametrize("where", ["thread", "lane", "wave", "tile"])
def test_offsets_pass_2_to_the_32(ctx, where):
    lens, first = lengths(where, 5100 + ["thread", "lane", "wave", "tile"].index(where))
    assert lens.min() == INT_MIN and lens.max() == INT_MAX and np.count_nonzero(lens < 0) > 100
    for align in (1, 4, 64, 256):
        model = offsets(clamp(lens, STRIDE_MAX), align)
        # reach: the first offset from 2**32 is where the docstring of lengths() puts it, and no partial sum in front of it is
        assert int(np.argmax(model >= B32)) == first and model[first - 1] < B32 <= model[first], (where, align)
        if where != "thread":
            assert int(model[8]) == int(model[first - 1]) and 0 < int(model[first]) - int(model[first - 1]) < 1024
        assert int(model[-1]) > 1 << 42
        got = run_offsets(ctx, lens, STRIDE_MAX, align)
        assert np.array_equal(got, model), (where, align, int(np.argmax(got != model)))


def test_offsets_clamped_to_a_small_stride(ctx):
    """the same lengths against a stride of 1 000 003: most are above it and count as the stride, the negative ones as 0"""
    stride = 1_000_003
    lens, _ = lengths("wave", 5200)
    c = clamp(lens, stride)
    assert np.count_nonzero(lens > stride) > N // 2 and np.count_nonzero(lens < 0) > 100 and np.count_nonzero((lens > 0) & (lens < stride)) > 0
    assert set(np.unique(c[(lens > stride) | (lens < 0)])) == {0, stride}
    for align in (1, 256):
        model = offsets(c, align)
        assert int(model[-1]) >= B32
        got = run_offsets(ctx, lens, stride, align)
        assert np.array_equal(got, model), (align, int(np.argmax(got != model)))


# ------------------------------------------------------------------ 2: a pack longer than 4 GiB
STRIDE = 940_000_003                   # odd


def test_pack_longer_than_4gib(api, ctx, oracle):
    """Eight source slots at a stride of 940 MB: five filled with seeded random bytes on the device, of lengths that bring the pack to
    4.37 GiB - the fifth stream straddles offset 2**32 - and three with oracle-encoded images (640 x 360 photo, 257 x 9 uiflat, 1 x 1), which
    therefore start beyond 4 GiB.  Destination at an odd address, align 1 and 256; a capacity that cuts the straddling stream and one that cuts
    the photograph's stream: neither is copied in part.  Every byte of the destination is compared on the device: the streams with their
    sources, everything else - the byte in front, the gaps, the tail - with the guard value.  Then, on the pack of align 256, the three real
    streams are read through qoimi_read_descs, qoimi_inspect_streams (the model) and qoimi_decode_images (the oracle's pixels).
    Peak device memory: 6.6 GB of sources + 4.7 GB of destination + 1 GB while slices are compared = about 12 GiB; freed at the end."""
    import torch
    items = [Item(api, oracle, "photo", 640, 360, 4, frame=2), Item(api, oracle, "uiflat", 257, 9, 4, frame=1),
             Item(api, oracle, None, 1, 1, 4, stream=oracle.encode(np.array([9, 3, 200, 255], dtype=np.uint8), 1, 1, 4))]
    fill = [STRIDE, STRIDE - 1, 937_000_001, STRIDE, 939_999_990]
    lens = fill + [len(it.stream) for it in items]
    n, n_fill = len(lens), len(fill)
    src = torch.empty(7 * STRIDE + lens[-1] + 64, dtype=torch.uint8, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(5300)
    for i in range(n_fill):
        src[i * STRIDE:(i + 1) * STRIDE].random_(0, 256, generator=gen)
    for i, it in enumerate(items):
        at = (n_fill + i) * STRIDE
        src[at:at + len(it.stream)].copy_(dev(np.frombuffer(it.stream, dtype=np.uint8).copy()))
    assert not torch.equal(src[:4096], src[STRIDE:STRIDE + 4096]) and not torch.equal(src[:16], src[16:32])
    d_lens = dev(np.array(lens, dtype=np.int32))
    off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    models = {a: offsets(lens, a) for a in (1, 256)}
    for a, m in models.items():
        m = [int(x) for x in m]
        assert m[4] < B32 < m[4] + lens[4] and all(x > B32 for x in m[5:]), "stream 4 straddles 2**32, the real streams lie beyond it"
        assert 4.3 * 2 ** 30 < m[-1] < 4.6 * 2 ** 30
    room = int(models[256][-1]) + 512
    packed = filled(room + 1)
    view = packed[1:]                                                          # an odd destination address
    st = torch.cuda.current_stream().cuda_stream

    def run(align, cap):
        packed.fill_(GUARD)
        off.zero_()
        ctx.pack_streams(src.data_ptr(), STRIDE, d_lens.data_ptr(), n, align, view.data_ptr(), cap, off.data_ptr(), st)
        ctx.encode_status(st)
        m = [int(x) for x in models[align]]
        assert [int(x) for x in off.cpu().numpy().view(np.uint64)] == m, align
        at = 0                                                                 # everything below `at` is checked
        for i in range(n):
            if m[i] + lens[i] > cap:
                continue                                                       # does not fit wholly: not copied, not in part
            assert bool((view[at:m[i]] == GUARD).all()), (align, cap, "gap in front of stream", i)
            assert torch.equal(view[m[i]:m[i] + lens[i]], src[i * STRIDE:i * STRIDE + lens[i]]), (align, cap, "stream", i)
            at = m[i] + lens[i]
        assert bool((view[at:] == GUARD).all()), (align, cap, "a byte behind the last stream that fits was written")
        assert int(packed[0]) == GUARD
        return m

    m1 = [int(x) for x in models[1]]
    run(1, m1[4] + lens[4] // 2)                                               # cuts the straddling stream: 0 .. 3 are copied
    run(1, m1[5] + lens[5] // 2)                                               # cuts the photograph's stream, wholly beyond 4 GiB: 0 .. 4
    run(1, m1[-1])
    m = run(256, int(models[256][-1]))
    assert any((m[i] + lens[i]) % 256 for i in range(n - 1)), "no gap to check"

    # the real streams, read where the pack put them: beyond 4 GiB from an odd base address
    so, sizes = m[n_fill:n], lens[n_fill:]
    descs, bad = ctx.read_descs(view.data_ptr(), so, sizes)
    assert bad is None and [(d.width, d.height, d.channels, d.colorspace) for d in descs] == [(it.w, it.h, it.ch, 0) for it in items]
    infos, first = ctx.inspect_streams(view.data_ptr(), so, sizes)
    assert first is None
    for k, it in enumerate(items):
        assert_info(infos[k], si.inspect_stream(it.stream), (k, so[k]))
    assert len(items[0].stream) > 22 + 3 * 16384                              # ... several blocks of inspect_maps beyond 4 GiB
    nbytes = [it.w * it.h * 4 for it in items]
    po = [64 + int(x) for x in np.cumsum([0] + [b + 3 for b in nbytes[:-1]])]
    out = filled(po[-1] + nbytes[-1] + 64)
    ctx.decode_images(view.data_ptr(), so, sizes, descs, 4, out.data_ptr(), po)
    got = out.cpu().numpy()
    mask = np.ones(got.size, dtype=bool)
    for k, it in enumerate(items):
        assert np.array_equal(got[po[k]:po[k] + nbytes[k]], oracle.decode(it.stream, 4)[0]), k
        mask[po[k]:po[k] + nbytes[k]] = False
    assert np.all(got[mask] == GUARD)
    del src, packed, view, out
    torch.cuda.empty_cache()
