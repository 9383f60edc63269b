"""Every device call with caller offsets whose high halves are not zero, and tensor outputs that are themselves longer than 4 GiB (-m gpu).

Part 1, the arenas.  B32 = 2^32.  Two device allocations of B32 + 96 MiB: `src` holds what calls read, `dst` (0xA5 everywhere) what they write.
The pointer a call gets is always the allocation's own start and every offset lies below the allocation's size, so an offset o >= B32 has
its alias o - B32 inside the same allocation: a kernel or marshaller that dropped a high half would read or write the alias - a failed
assertion, not a fault (`layout` asserts this for every offset the file uses).  Each offset array gets three placements in ONE call: control
(wholly below B32), straddling (from B32 - k, k an odd number of elements for tensor outputs of every element size, i64 included - an output
is element-aligned and B32 a multiple of 8, so it is the item that lies across byte B32, an element ends at it - and 0 < k < the item's size)
and beyond (wholly beyond, at B32 + an odd number of elements).  After each call the expected output ranges are read back and filled with 0xA5
again, then the WHOLE of `dst` is compared with the guard pattern on the device (one comparison through an int64 view).  What is read from a
high offset has a decoy of the same shape - real streams of the oracle, or pixels, of other content - at its alias; every decoy's result is
asserted to differ from the true one, and the touched windows of `src` are compared with their host-side construction after the calls.  Where
two arrays of one call lie in `src`, only one range can hold byte B32: such calls run twice, the straddling item in either array in turn.
Every expectation is the existing definition (the oracle, then the models of qoi_amd/); every comparison is exact and covers whole outputs.
That the decoy of every item of the newer filters and samplings resamples to other bytes than the true image is asserted without a GPU
(test_the_decoys_of_the_newer_items_differ).

    call                                            moved past 2^32
    qoimi_encode_images                             pixel_offsets, stream_offsets
    qoimi_encode_images_packed                      pixel_offsets
    qoimi_encode_batch                              pixel stride, stream stride (two images, the second wholly beyond)
    qoimi_encode_packed                             pixel stride
    qoimi_decode_batch                              pixel stride
    qoimi_encode_tiles                              pixel_offsets (f = 1, 3, 64; PLAIN and ALPHA_WEIGHTED: tile_gather; NEAREST, and MODE with
                                                    f = 1, 3, 16: tile_select; each at channels 0, 4, 3; one launch per sub-batch)
    qoimi_encode_tiles, tensor sources                  pixel_offsets (tensor_ingest: f16 CHW, bf16 HWC, f32 CHW and u8 CHW tensors of 3 and 4 elements
                                                    a pixel in ONE call at channels 0 and 3; every offset a multiple of 4, so an f32
                                                    element ends at byte B32 inside the f32 CHW tensor that lies across it; every
                                                    dtype has a tensor across or beyond; decoys: tensors of other elements)
    qoimi_decode_thumbnails                         stream_offsets, thumb_offsets
    qoimi_decode_crops / _resized / _bilinear / _warped                 stream_offsets, out_offsets
    qoimi_decode_tensors, all six filters (tensor_area, tensor_tent, tensor_cubic, tensor_lanczos, tensor_nearest, tensor_mode)
                                                    stream_offsets, out_offsets (FORMATS: every dtype - u8, f16, bf16, f32, i32, i64 - and
                                                    every layout - HWC, CHW, HW - lies across byte B32 and beyond it at least once)
    qoimi_decode_warped_tensors                     stream_offsets, out_offsets, five lists of items (below)
    qoimi_decode_crops_indexed / _resized_indexed / _bilinear_indexed / _warped_indexed
                                                    stream_offsets, out_offsets, the index built over the high pack
    the warp calls (u8, tensors, indexed) take five lists: WARPS (bilinear items alone: warp_gather / tensor_warp), WARPS_NEAREST (nearest
    and bilinear items, none bicubic: the nearest branch of the same kernels), WARPS_CUBIC (bicubic, bilinear and nearest items in one
    call: warp_bicubic_bytes / warp_bicubic_tensor serve all of them), WARPS_BORDER (REFLECT, REFLECT_101 and WRAP with each sampling, and
    fill, REPLICATE and bicubic items, in one call: warp_border_bytes / warp_border_tensor; two maps several periods away) and WARPS_SUPER
    (SUPER2 and SUPER4 with the fill and every border, and bilinear, nearest, bicubic and bordered items, in one call: warp_super_bytes /
    warp_super_tensor); the tensor formats of the last two cover every dtype between them and every layout each
    qoimi_build_seek_index                          stream_offsets
    qoimi_seek_index_from_pixels                    pixel_offsets, stream_offsets
    qoimi_make_band_streams                         stream_offsets, out_offsets
    qoimi_pixel_stats                               stream_offsets
    qoimi_verify_images                             pixel_offsets, stream_offsets (a difference planted in a high copy only)
    qoimi_compare_images                            a_offsets, b_offsets (the difference planted in the high copies only)

Part 2, single outputs of 16400 x 16400 x 4 f32 = 4 303 360 000 bytes > 2^32, each in a fresh allocation between two guard pages, checked
wholly on the device:
    1. area filter, f32, CHW: a 41 x 41 noise image enlarged by exactly 400 per axis, either flip in turn - every element of the model's
       41 x 41 result 400 x 400 times (position-sensitive at a 400-pixel grain, the fourth plane lies past 2^32)
    2. warp, f32, HWC, flags 0: a 64 x 48 rectangle under the identity into the corner, the converted fill everywhere else
    3. tent filter, f32, CHW: a constant image stays four constant planes
and single SOURCES of the same size, the image of a tensor call of qoimi_encode_tiles (tensor_ingest), once HWC and once CHW:
    4. the allocation is filled with one byte on the device - as f32 an element that converts to a known byte -, and windows of whole
       rows hold random elements (tests/ingest_cases.py: BIG_WINDOWS): low in the image (control), around byte 2^32 of the image (HWC:
       pixel 2^28 stands at column 256 of row 16368; CHW: in the fourth plane, at column 1024 of row 16272), and the last rows; the
       elements 2^32 bytes below the last two - what a 32-bit byte offset would read - hold decoys.  Tiles of 400 to 403 x 8 pixels of each
       window in every flip, and one of the constant, against tiles.tile over the window alone (a tile depends on its rectangle's elements
       only: tests/test_ingest_paths.py); the tile a wrapped offset would read is built from the decoys and asserted to differ.
The model conditions these rest on - integer enlargement by the area filter replicates, the identity warp pads with the fill and does not
depend on the output's size, the tent filter keeps a constant - are asserted without a GPU by the first three tests of this file."""
import numpy as np
import pytest

import ingest_cases
from gpu_util import GuardedRegion
from mode_cases import IMAGES as LABEL_MAPS
from mode_cases import label_map
from qoi_amd import bilinear, crops, resize, tensors, thumbs, tiles, warp
from qoi_amd import mode as mode_filter
from qoi_amd import pixelstats as ps
from qoi_amd.imagediff import DIFF_DTYPE, DIFF_PIXELS, NONE, diff
from qoi_amd.tensors import (BF16, CHW, F16, F32, FILTER_AREA, FILTER_BICUBIC, FILTER_BILINEAR, FILTER_LANCZOS, FILTER_MODE, FILTER_NEAREST, HW, HWC, I32, I64,
                             U8)
from seek_cases import cases as seek_cases
from gpu_calls import assert_outputs as assert_bytes
from gpu_pack import IMAGENET, Pack, batch_of, filled, image
from gpu_pack import api, ctx, oracle  # noqa: F401  (fixtures)
from model_cases import pack_offsets
from wide_cases import ARENA, B32, layout, tensor_offsets

gpu = pytest.mark.gpu
GUARD, SRC_FILL = 0xA5, 0x5C
GUARD64 = int.from_bytes(bytes([GUARD]) * 8, "little", signed=True)
PAGE = 4096
SIDE = 16400                    # the smallest practical side at which side * side * 4 channels of f32 pass 2^32
BIG_BYTES = SIDE * SIDE * 4 * 4
F32_CHW, F32_HWC = (F32, CHW, *IMAGENET), (F32, HWC, *IMAGENET)
FILL = 0xFF804020               # opaque, four distinct bytes
CONSTANT = (200, 17, 90, 255)   # the constant image of part 2: four distinct values, opaque
assert B32 < BIG_BYTES < ARENA - PAGE and SIDE * SIDE < 400_000_000 and SIDE < 32767 and SIDE == 400 * 41


# ------------------------------------------------------------------ the model conditions of part 2 (no GPU)
def noise41():
    return np.random.default_rng(41).integers(0, 256, size=(41, 41, 4), dtype=np.uint8)


def test_area_enlargement_by_an_integer_replicates():
    D = noise41()
    for mode in (resize.PLAIN, resize.ALPHA_WEIGHTED):
        for flags in (0, 1, 2, 3):
            one = resize.resize(D, (0, 0, 41, 41), (41, 41), flags, mode)
            assert np.array_equal(one, crops.crop(D, (0, 0, 41, 41), flags))
            for m in (2, 3):
                assert np.array_equal(resize.resize(D, (0, 0, 41, 41), (41 * m, 41 * m), flags, mode), one.repeat(m, axis=0).repeat(m, axis=1)), (mode, flags, m)


def test_identity_warp_pads_with_the_fill_whatever_the_output_size():
    D = np.random.default_rng(6448).integers(0, 256, size=(48, 64, 4), dtype=np.uint8)
    small = warp.warp(D, (0, 0, 64, 48), (80, 64), warp.IDENTITY, 0, FILL, warp.PLAIN)
    padded = np.empty((64, 80, 4), dtype=np.uint8)
    padded[:] = np.array([FILL >> (8 * k) & 255 for k in range(4)], dtype=np.uint8)
    padded[:48, :64] = D
    assert np.array_equal(small, padded)                                        # no blending at the edge
    large = warp.warp(D, (0, 0, 64, 48), (200, 100), warp.IDENTITY, 0, FILL, warp.PLAIN)
    assert np.array_equal(large[:64, :80], small) and np.all(large[64:] == padded[63, 79]) and np.all(large[:, 80:] == padded[63, 79])
    assert len(set(int(v) for v in padded[63, 79])) == 4


def test_the_tent_filter_keeps_a_constant():
    D = np.empty((64, 64, 4), dtype=np.uint8)
    D[:] = CONSTANT
    for mode in (bilinear.PLAIN, bilinear.ALPHA_WEIGHTED):
        assert np.all(bilinear.bilinear(D, (0, 0, 64, 64), (150, 131), 0, mode) == np.array(CONSTANT, dtype=np.uint8))


# ------------------------------------------------------------------ the arenas


def flat(a):
    if isinstance(a, (bytes, bytearray)):
        return np.frombuffer(bytes(a), dtype=np.uint8)
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def first_true(mask):
    """the index of the first True of a (large) device bool tensor"""
    step = 1 << 26
    for at in range(0, mask.numel(), step):
        part = mask[at:at + step]
        if bool(part.any()):
            return at + int(part.nonzero()[0])
    return -1


class Source:
    """What the calls read: the arena and its host-side construction, window by window."""

    def __init__(self):
        self.t = filled(ARENA, SRC_FILL)
        self.windows = []

    def put(self, off, data):
        import torch
        data = flat(data).copy()
        assert 0 <= off and off + data.size <= ARENA and all(off + data.size <= o or o + d.size <= off for o, d in self.windows), off
        self.t[off:off + data.size].copy_(torch.from_numpy(data))
        self.windows.append((off, data))

    def seen(self, off, n):
        """the n bytes at off, by the construction"""
        out = np.full(n, SRC_FILL, dtype=np.uint8)
        for o, d in self.windows:
            a, e = max(o, off), min(o + d.size, off + n)
            if a < e:
                out[a - off:e - off] = d[a - o:e - o]
        return out

    def misread(self, off, n):
        """what a reader of [off, off + n) sees that drops the high half of the offset, or of the address of each byte"""
        if off >= B32:
            return self.seen(off - B32, n)
        k = B32 - off
        return np.concatenate([self.seen(off, k), self.seen(0, n - k)])

    def place(self, offsets, true, decoys):
        """true[j] at offsets[j]; where that lies beyond B32, decoys[j] (cut to the same size) at the alias"""
        for o, t, d in zip(offsets, true, decoys):
            t, d = flat(t), flat(d)[:flat(t).size]
            self.put(o, t)
            if o + t.size > B32:
                lo = max(o, B32)
                if d.size > lo - o:
                    self.put(lo - B32, d[lo - o:])
                assert not np.array_equal(self.misread(o, t.size), t), o

    def check(self):
        for o, d in self.windows:
            assert np.array_equal(self.t[o:o + d.size].cpu().numpy(), d), ("a source was written", o)

    def clear(self):
        for o, d in self.windows:
            self.t[o:o + d.size].fill_(SRC_FILL)
        self.windows = []


class Dest:
    """What the calls write: 0xA5 everywhere before and after every call."""

    def __init__(self):
        import torch
        self.t = filled(ARENA, GUARD)
        self.words = self.t.view(torch.int64)

    def clean(self):
        return bool((self.words == GUARD64).all())

    def take(self, offsets, sizes, what):
        """The outputs as host arrays; their ranges are filled with the guard again and then the whole arena is the guard pattern."""
        got = [self.t[o:o + n].cpu().numpy() for o, n in zip(offsets, sizes)]
        for o, n in zip(offsets, sizes):
            self.t[o:o + n].fill_(GUARD)
        if not self.clean():
            w = first_true(self.words != GUARD64)
            k = w * 8 + int(np.argmax(self.t[w * 8:w * 8 + 8].cpu().numpy() != GUARD))
            where = GuardedRegion(ARENA, offsets, GUARD).where(k, sizes)
            self.t.fill_(GUARD)
            raise AssertionError(f"{what}: a byte outside the outputs was written, the first at byte {k} = 2^32 {k - B32:+d} of the arena ({where})")
        return got


def into_dst(dst, want, call, what, elem=1, lane=0, spans=None, sizes=None):
    """call(base of dst, offsets) writes want[j] to a control, a straddling or a beyond placement; every other byte of dst stays the guard"""
    want = [flat(w) for w in want]
    offsets = layout([w.size for w in want] if sizes is None else sizes, elem, lane, spans=spans)
    result = call(dst.t.data_ptr(), offsets)
    assert_bytes(dst.take(offsets, [w.size for w in want], what), want, what)
    return result


# ------------------------------------------------------------------ fixtures


@pytest.fixture(scope="module")
def arenas(api):
    import torch
    pair = [Source(), Dest()]
    yield pair
    pair.clear()
    torch.cuda.empty_cache()


@pytest.fixture
def src(arenas):
    yield arenas[0]
    arenas[0].clear()


@pytest.fixture
def dst(arenas):
    yield arenas[1]
    if not arenas[1].clean():
        arenas[1].t.fill_(GUARD)


SHAPES = [(1, 1, 4), (1, 97, 4), (37, 29, 3), (130, 70, 4), (64, 48, 4), (37, 29, 3), (70, 45, 4)]
TINY, COLUMN, RGB, SPRITE, NOISE, LABEL3, LABEL = range(7)
INTERVALS = [128, 128, 4, 8, 6, 128, 128]             # seek rows: none, none, every 4th, 8th, 6th, none, none
KINDS_OF = ["noise", "photo", "photo", "sprite_alpha", "noise"]


def other(px):
    """pixels of the same shape and other content: the decoys"""
    return flat(px) ^ 0x5A


def pack_pixels():
    """the images of the pack: the content classes of tests/test_gpu_encode_packed.py, then the two label maps of tests/mode_cases.py - three
    classes in 3 channels, five in 4 - for the vote of FILTER_MODE: the other images have no majority anywhere.  Two, so that `layout` places
    the stream of one of them below B32 and that of the other beyond it"""
    return [image(k, w, h, ch, frame=i) for i, ((w, h, ch), k) in enumerate(zip(SHAPES, KINDS_OF))] + [label_map(*im).reshape(-1) for im in LABEL_MAPS]


@pytest.fixture(scope="module")
def pack(api, ctx, oracle):
    """the shapes of the mixed packs with 3 and 4 channels and a label map; the decoy of every image and its stream by the oracle"""
    b = batch_of(api, oracle, SHAPES, pack_pixels())
    b.want = [oracle.encode(px, w, h, ch) for px, (w, h, ch) in zip(b.px, SHAPES)]
    b.lens = [len(s) for s in b.want]
    p = Pack(ctx, oracle, b)
    p.streams = [p.host[o:o + n].copy() for o, n in zip(p.so, p.sizes)]
    assert [s.tobytes() for s in p.streams] == p.b.want
    p.decoy_px = [other(px) for px in p.b.px]
    p.decoy_streams = [oracle.encode(d, w, h, ch) for d, (w, h, ch) in zip(p.decoy_px, SHAPES)]
    p.decoy_decoded = [oracle.decode(s, 4)[0].reshape(h, w, 4) for s, (w, h, _) in zip(p.decoy_streams, SHAPES)]
    return p


def place_streams(src, oracle, streams, decoys, shapes, decodes, lane=0, straddle=True):
    """The streams at control, straddling and beyond offsets of src, decoys at the aliases; whoever dropped a high half would decode other pixels."""
    so = layout([len(s) for s in streams], lane=lane, straddle=straddle)
    src.place(so, streams, decoys)
    for o, s, (w, h, ch), D in zip(so, streams, shapes, decodes):
        if o + len(s) > B32:
            px, _ = oracle.decode(src.misread(o, len(s)).tobytes(), ch)
            assert px is None or not np.array_equal(flat(px), flat(D)), o
    return so


def place_pack(src, oracle, p, **how):
    return place_streams(src, oracle, p.streams, p.decoy_streams, SHAPES, [p.decoded(i, ch) for i, (_, _, ch) in enumerate(SHAPES)], **how)


# ------------------------------------------------------------------ 1: the encoders
@gpu
def test_encode_images_and_images_packed(ctx, pack, src, dst):
    import torch
    b = pack.b
    po = layout([px.size for px in b.px], lane=1)
    src.place(po, b.px, pack.decoy_px)
    lens = torch.full((b.n,), -1, dtype=torch.int32, device="cuda")

    def encode(out, so):
        ctx.encode_images(src.t.data_ptr(), po, b.descs, out, so, lens.data_ptr(), 0)
        ctx.encode_status(0)

    # a slot is the bound; the stream in it is what straddles
    into_dst(dst, b.want, encode, "encode_images", sizes=b.bounds, spans=b.lens)
    assert lens.cpu().numpy().tolist() == b.lens
    want_off = pack_offsets(b.lens, 1)
    off = torch.full((b.n + 1,), -1, dtype=torch.int64, device="cuda")
    lens.fill_(-1)
    got_off, got_len = ctx.encode_images_packed(src.t.data_ptr(), po, b.descs, 1, dst.t.data_ptr(), int(want_off[-1]), off.data_ptr(), lens.data_ptr())
    assert np.array_equal(got_off, want_off) and got_len.tolist() == b.lens and lens.cpu().numpy().tolist() == b.lens
    assert np.array_equal(off.cpu().numpy().astype(np.uint64), want_off)
    assert_bytes(dst.take([int(o) for o in want_off[:b.n]], b.lens, "encode_images_packed"), b.want, "encode_images_packed")
    src.check()


@gpu
def test_strides_past_4gib(api, ctx, oracle, pack, src, dst):
    """two images: the second lies wholly beyond, and its alias is the first one, 3 bytes on"""
    import torch
    w, h, ch = SHAPES[NOISE]
    n = w * h * ch
    px = [pack.b.px[NOISE], other(pack.b.px[NOISE])[::-1].copy()]
    want = [oracle.encode(p, w, h, ch) for p in px]
    desc, bound = api.QoiDesc(w, h, ch, 0), api.encode_bound(w, h, ch)
    pixel_stride, stream_stride = B32 + 3, B32 + 5
    assert pixel_stride + n <= ARENA and stream_stride + bound <= ARENA and 3 + n <= B32 and 5 + bound <= B32
    src.put(0, px[0])
    src.put(pixel_stride, px[1])
    assert not np.array_equal(src.misread(pixel_stride, n), px[1])
    lens = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    ctx.encode_batch(src.t.data_ptr(), pixel_stride, desc, 2, dst.t.data_ptr(), stream_stride, lens.data_ptr(), 0)
    ctx.encode_status(0)
    sizes = [len(s) for s in want]
    assert lens.cpu().numpy().tolist() == sizes
    assert_bytes(dst.take([0, stream_stride], sizes, "encode_batch"), want, "encode_batch")
    off = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    got_off, got_len = ctx.encode_packed(src.t.data_ptr(), pixel_stride, desc, 2, 1, dst.t.data_ptr(), sum(sizes), off.data_ptr(), lens.data_ptr())
    assert got_off.tolist() == [0, sizes[0], sum(sizes)] and got_len.tolist() == sizes and off.cpu().numpy().tolist() == [0, sizes[0], sum(sizes)]
    assert_bytes(dst.take([0, sizes[0]], sizes, "encode_packed"), want, "encode_packed")
    src.check()
    src.clear()
    # the decoder: the streams lie low, a stride of bound + 1 apart (a high stream stride has its own test), the images B32 + 5 apart
    src.put(0, want[0])
    src.put(bound + 1, want[1])
    for och in (4, 3):
        expect = [oracle.decode(s, och)[0] for s in want]
        assert B32 + 5 + expect[1].size <= ARENA
        ctx.decode_batch(src.t.data_ptr(), bound + 1, sizes, [desc, desc], och, dst.t.data_ptr(), B32 + 5, 0)
        assert_bytes(dst.take([0, B32 + 5], [e.size for e in expect], ("decode_batch", och)), expect, ("decode_batch", och))
    src.check()


TILES = [(SPRITE, 0, 0, 130, 70, 1, 0), (SPRITE, 3, 5, 120, 64, 3, 1), (SPRITE, 0, 0, 130, 70, 64, 2), (RGB, 0, 0, 37, 29, 1, 3), (RGB, 1, 2, 30, 21, 3, 0),
         (NOISE, 0, 0, 64, 48, 64, 0), (NOISE, 8, 1, 48, 40, 3, 2), (COLUMN, 0, 0, 1, 97, 1, 1), (COLUMN, 0, 1, 1, 96, 64, 0), (TINY, 0, 0, 1, 1, 1, 0),
         (LABEL3, 0, 2, 37, 27, 3, 1), (LABEL, 1, 0, 69, 45, 1, 2)]


# the label modes (tile_select): MODE votes over blocks of at most 16 x 16 pixels, so its list has the 64-fold tiles of TILES 16-fold
TILES_MODE = [t[:5] + (16 if t[5] == 64 else t[5],) + t[6:] for t in TILES]
BOX_MODES = ((0, tiles.PLAIN), (4, tiles.ALPHA_WEIGHTED), (3, tiles.PLAIN))
LABEL_MODES = tuple((channels, mode) for mode in (tiles.NEAREST, tiles.MODE) for channels in (0, 4, 3))
assert {t[5] for t in TILES} == {1, 3, 64} and {t[5] for t in TILES_MODE} == {1, 3, 16} and tiles.MODE_MAX_FACTOR == 16
assert [t[:5] + t[6:] for t in TILES_MODE] == [t[:5] + t[6:] for t in TILES] and TILES[2][5] == 64 and TILES_MODE[2][5] == 16


@gpu
def test_encode_tiles(ctx, oracle, pack, src, dst):
    """tile_gather in both box modes, then tile_select in NEAREST and MODE - a kernel of its own that reads `pixels + e.src_off` itself -, each
    at channels 0, 4 and 3 over the same pixel_offsets: control, straddling and beyond"""
    import torch
    b = pack.b
    assert {t[0] for t in TILES} == set(range(b.n))
    po = layout([px.size for px in b.px], lane=1)
    src.place(po, b.px, pack.decoy_px)
    assert any(o >= B32 for o in po) and any(o < B32 < o + px.size for o, px in zip(po, b.px))
    images = [px.reshape(h, w, ch) for px, (w, h, ch) in zip(b.px, SHAPES)]
    for channels, mode in BOX_MODES + LABEL_MODES:
        ts = TILES_MODE if mode == tiles.MODE else TILES
        assert {t[5] for t in ts} == ({1, 3, 16} if mode == tiles.MODE else {1, 3, 64})
        px = [tiles.tile(images[t[0]], t, channels, mode) for t in ts]
        want = [oracle.encode(p.reshape(-1), p.shape[1], p.shape[0], p.shape[2], 0) for p in px]
        decoy = tiles.tile(pack.decoy_px[SPRITE].reshape(70, 130, 4), ts[2], channels, mode)
        assert not np.array_equal(decoy, px[2])                    # even the 64-fold (MODE: 16-fold) reduction tells the decoy
        lens = [len(s) for s in want]
        want_off = pack_offsets(lens, 1)
        off = torch.full((len(ts) + 1,), -1, dtype=torch.int64, device="cuda")
        d_len = torch.full((len(ts),), -1, dtype=torch.int32, device="cuda")
        got_off, got_len, got_descs = ctx.encode_tiles(src.t.data_ptr(), po, b.descs, channels, ts, mode, 1, dst.t.data_ptr(), int(want_off[-1]),
                                                       off.data_ptr(), d_len.data_ptr())
        what = ("encode_tiles", channels, mode)
        assert np.array_equal(got_off, want_off) and got_len.tolist() == lens and d_len.cpu().numpy().tolist() == lens, what
        assert [(d.width, d.height, d.channels) for d in got_descs] == [(p.shape[1], p.shape[0], p.shape[2]) for p in px], what
        assert_bytes(dst.take([int(o) for o in want_off[:-1]], lens, what), want, what)
        subs = tiles.plan(SHAPES, ts, channels, 0)[1]
        assert ctx.tile_stats()[:2] == (len(subs), len(subs)), what       # one launch (tile_gather, or tile_select) per sub-batch
    src.check()


def wide_tensors(seed):
    """the tensors of ingest_cases.WIDE_SPECS: random elements over both clamps of each range"""
    from gpu_calls import elements
    rng = np.random.default_rng(seed)
    return [np.ascontiguousarray(elements(rng, w * h * sch, fmt[0], fmt[2])).reshape((sch, h, w) if fmt[1] == tiles.CHW else (h, w, sch))
            for w, h, sch, fmt in ingest_cases.WIDE_SPECS]


@gpu
def test_encode_tiles_tensor_sources(api, ctx, oracle, src, dst):
    """tensor_ingest reads `pixels + e.src_off` itself: tensors of every dtype at control, straddling and beyond offsets in one call"""
    import torch
    specs, ts = ingest_cases.WIDE_SPECS, ingest_cases.wide_tiles()
    po = tensor_offsets()
    true, decoys = wide_tensors(32), wide_tensors(33)
    sizes = [a.nbytes for a in true]
    assert src.t.data_ptr() % 256 == 0                             # (tests/test_ingest_paths.py replays the offsets modulo 256)
    assert all(o % tiles.ELEM[s[3][0]] == 0 for o, s in zip(po, specs))
    assert {s[3][0] for o, n, s in zip(po, sizes, specs) if o + n > B32} == {tiles.U8, tiles.F16, tiles.BF16, tiles.F32}
    across = [i for i, (o, n) in enumerate(zip(po, sizes)) if o < B32 < o + n]
    assert len(across) == 1 and specs[across[0]][3][:2] == (tiles.F32, tiles.CHW) and (B32 - po[across[0]]) % 4 == 0      # an element ends at byte B32
    assert {(s[3][0], s[3][1]) for s in specs} == {(tiles.F16, tiles.CHW), (tiles.BF16, tiles.HWC), (tiles.F32, tiles.CHW), (tiles.U8, tiles.CHW)}
    assert all({s[2] for s in specs if s[3][0] == d} == {3, 4} for d in (tiles.U8, tiles.F16, tiles.BF16, tiles.F32))
    src.place(po, true, decoys)
    descs = [api.QoiDesc(w, h, sch, i & 1) for i, (w, h, sch, _) in enumerate(specs)]
    B = [tiles.convert(a, tiles.source_flags(*s[3])) for a, s in zip(true, specs)]
    for channels in ingest_cases.WIDE_CHANNELS:
        px = [tiles.tile(B[t[0]], t[:6] + (t[6] & 3,), channels) for t in ts]
        want = [oracle.encode(p.reshape(-1), p.shape[1], p.shape[0], p.shape[2], descs[t[0]].colorspace) for p, t in zip(px, ts)]
        for t, p in zip(ts, px):                                   # whoever dropped a high half would convert the decoy: another tile
            i = t[0]
            if po[i] + sizes[i] > B32:
                seen = np.frombuffer(src.misread(po[i], sizes[i]).tobytes(), dtype=true[i].dtype).reshape(true[i].shape)
                assert not np.array_equal(tiles.tile(seen, t, channels), p), (t, channels)
        lens = [len(s) for s in want]
        want_off = pack_offsets(lens, 1)
        off = torch.full((len(ts) + 1,), -1, dtype=torch.int64, device="cuda")
        d_len = torch.full((len(ts),), -1, dtype=torch.int32, device="cuda")
        got_off, got_len, got_descs = ctx.encode_tiles(src.t.data_ptr(), po, descs, channels, ts, tiles.PLAIN, 1, dst.t.data_ptr(), int(want_off[-1]),
                                                       off.data_ptr(), d_len.data_ptr())
        what = ("encode_tiles, tensor sources", channels)
        assert np.array_equal(got_off, want_off) and got_len.tolist() == lens and d_len.cpu().numpy().tolist() == lens, what
        assert [(d.width, d.height, d.channels) for d in got_descs] == [(p.shape[1], p.shape[0], p.shape[2]) for p in px], what
        assert_bytes(dst.take([int(o) for o in want_off[:-1]], lens, what), want, what)
        assert ctx.tile_stats()[:2] == (1, 1) and ctx.tile_stats()[3] == len(specs), what
    src.check()


# ------------------------------------------------------------------ 2: the gather family
FACTORS = [1, 5, 3, 2, 64, 3, 4]
CROPS = [(SPRITE, 5, 17, 101, 50, 1), (RGB, 0, 9, 37, 20, 2), (NOISE, 8, 13, 33, 30, 3), (COLUMN, 0, 3, 1, 90, 0), (TINY, 0, 0, 1, 1, 0), (SPRITE, 0, 40, 130, 30, 0)]
ITEMS = [(SPRITE, 0, 17, 130, 53, 43, 23, 1), (RGB, 0, 9, 37, 20, 50, 40, 2), (NOISE, 3, 13, 40, 30, 40, 30, 3), (COLUMN, 0, 0, 1, 97, 1, 13, 0),
         (TINY, 0, 0, 1, 1, 3, 2, 0), (SPRITE, 20, 20, 64, 32, 9, 5, 0)]
WARPS = [warp.item(SPRITE, (20, 17, 100, 50), (33, 18), warp.rotation((100, 50), (33, 18), 30.0, 0.3), 0, FILL),
         warp.item(RGB, (3, 9, 30, 20), (17, 16), warp.rotation((30, 20), (17, 16), 30.0, 0.9), warp.REPLICATE, 0),
         warp.item(NOISE, (0, 13, 64, 35), (70, 40), warp.IDENTITY, 0, FILL), warp.item(TINY, (0, 0, 1, 1), (2, 2), warp.IDENTITY, warp.REPLICATE, 0)]
# The second and third warp lists.  WARPS_CUBIC: bicubic, bilinear and nearest items in ONE call - one bicubic item sends the whole call to
# warp_bicubic_bytes / warp_bicubic_tensor, which then serve the items that are not bicubic as well.  WARPS_NEAREST: no bicubic item - the call
# stays with warp_gather / tensor_warp and takes their nearest branch.  In both every image with seek rows has an item that begins below one.
WARPS_CUBIC = [warp.item(SPRITE, (20, 17, 100, 50), (33, 18), warp.rotation((100, 50), (33, 18), 30.0, 0.3), warp.BICUBIC, FILL),
               warp.item(RGB, (3, 9, 30, 20), (17, 16), warp.rotation((30, 20), (17, 16), 30.0, 0.9), warp.BICUBIC | warp.REPLICATE, 0),
               warp.item(NOISE, (0, 13, 64, 35), (70, 40), warp.IDENTITY, warp.NEAREST, FILL),
               warp.item(LABEL, (5, 3, 63, 41), (33, 18), warp.rotation((63, 41), (33, 18), 30.0, 0.9), warp.NEAREST | warp.REPLICATE, 0),
               warp.item(SPRITE, (0, 40, 130, 30), (41, 29), warp.rotation((130, 30), (41, 29), -20.0, 0.4), 0, FILL),
               warp.item(NOISE, (8, 13, 33, 30), (23, 40), warp.rotation((33, 30), (23, 40), 90.0, 0.8), warp.REPLICATE, 0),
               warp.item(TINY, (0, 0, 1, 1), (2, 2), warp.IDENTITY, warp.BICUBIC | warp.REPLICATE, 0),
               warp.item(COLUMN, (0, 3, 1, 90), (5, 31), warp.rotation((1, 90), (5, 31), 10.0, 0.4), warp.BICUBIC, FILL),
               warp.item(LABEL3, (2, 1, 33, 25), (40, 30), warp.rotation((33, 25), (40, 30), -15.0, 1.3), warp.NEAREST, FILL)]
WARPS_NEAREST = [warp.item(SPRITE, (20, 17, 100, 50), (33, 18), warp.rotation((100, 50), (33, 18), 30.0, 0.3), warp.NEAREST, FILL),
                 warp.item(RGB, (3, 9, 30, 20), (17, 16), warp.rotation((30, 20), (17, 16), 30.0, 0.9), warp.NEAREST | warp.REPLICATE, 0),
                 warp.item(NOISE, (0, 13, 64, 35), (70, 40), warp.IDENTITY, 0, FILL),
                 warp.item(LABEL, (5, 3, 63, 41), (66, 36), warp.rotation((63, 41), (66, 36), -30.0, 1.8), warp.NEAREST, FILL),
                 warp.item(TINY, (0, 0, 1, 1), (2, 2), warp.IDENTITY, warp.NEAREST | warp.REPLICATE, 0),
                 warp.item(COLUMN, (0, 3, 1, 90), (5, 31), warp.rotation((1, 90), (5, 31), 10.0, 0.4), warp.NEAREST, FILL),
                 warp.item(LABEL3, (2, 1, 33, 25), (40, 30), warp.rotation((33, 25), (40, 30), -15.0, 1.3), warp.NEAREST | warp.REPLICATE, 0)]
assert {it[7] for it in WARPS} == {0, warp.REPLICATE} and not any(it[7] & warp.BICUBIC for it in WARPS_NEAREST)
assert {it[7] & ~warp.REPLICATE for it in WARPS_CUBIC} == {0, warp.NEAREST, warp.BICUBIC} and {it[7] & ~warp.REPLICATE for it in WARPS_NEAREST} == {0, warp.NEAREST}
assert {warp.BICUBIC, warp.BICUBIC | warp.REPLICATE, warp.NEAREST, warp.NEAREST | warp.REPLICATE} <= {it[7] for it in WARPS_CUBIC}
# The fourth and fifth warp lists.  WARPS_BORDER: every folding border with every sampling, and items without such a border - fill, REPLICATE,
# bicubic - in ONE call, none with a SUPER flag: one bordered item sends the whole call to warp_border_bytes / warp_border_tensor.  Two of its
# maps lie several periods away from their rectangles (the quotient estimate of warp_fold_position), the others within one (its conditional
# branch).  WARPS_SUPER: both SUPER flags with the fill and each of the four borders, and one item of each older kind - bilinear, nearest,
# bicubic, bordered -: one SUPER item sends the whole call to warp_super_bytes / warp_super_tensor.  In both every image of the pack has an
# item, every image with seek rows one that begins below a seek row, and no output is larger than 41 x 29.
FOLDING = (warp.REFLECT, warp.REFLECT_101, warp.WRAP)
SAMPLINGS = (0, warp.NEAREST, warp.BICUBIC)
ONE = warp.ONE
WARPS_BORDER = [warp.item(SPRITE, (20, 17, 100, 50), (33, 18), warp.rotation((100, 50), (33, 18), 30.0, 0.2), warp.REFLECT, FILL),
                warp.item(RGB, (3, 9, 30, 20), (17, 16), warp.rotation((30, 20), (17, 16), 30.0, 0.5), warp.REFLECT | warp.NEAREST, FILL),
                warp.item(NOISE, (0, 13, 64, 35), (41, 29), warp.rotation((64, 35), (41, 29), -20.0, 0.4), warp.REFLECT | warp.BICUBIC, FILL),
                warp.item(LABEL, (5, 3, 63, 41), (33, 18), warp.rotation((63, 41), (33, 18), 30.0, 0.3), warp.REFLECT_101 | warp.NEAREST, FILL),
                warp.item(COLUMN, (0, 3, 1, 90), (5, 29), warp.rotation((1, 90), (5, 29), 10.0, 0.2), warp.REFLECT_101, FILL),
                warp.item(SPRITE, (0, 40, 130, 30), (41, 29), warp.rotation((130, 30), (41, 29), -20.0, 0.25), warp.REFLECT_101 | warp.BICUBIC, FILL),
                warp.item(LABEL3, (2, 1, 33, 25), (40, 29), warp.rotation((33, 25), (40, 29), -15.0, 0.6), warp.WRAP | warp.NEAREST, FILL),
                warp.item(NOISE, (8, 13, 33, 30), (23, 29), (ONE + 300, 4000, 2 * ONE * 33 * 5 + 777, -2500, ONE - 200, -2 * ONE * 30 * 7 - 999), warp.WRAP, FILL),
                warp.item(RGB, (1, 4, 35, 24), (19, 18), (ONE, 23000, -2 * ONE * 35 * 40 - 40000, -9000, ONE + 700, 2 * ONE * 24 * 9 + 12345), warp.WRAP | warp.BICUBIC, FILL),
                warp.item(TINY, (0, 0, 1, 1), (2, 2), warp.IDENTITY, warp.REFLECT_101, 0),
                warp.item(SPRITE, (20, 17, 100, 50), (33, 18), warp.rotation((100, 50), (33, 18), 30.0, 0.3), 0, FILL),
                warp.item(NOISE, (8, 13, 33, 30), (23, 29), warp.rotation((33, 30), (23, 29), 90.0, 0.8), warp.REPLICATE, 0),
                warp.item(RGB, (3, 9, 30, 20), (17, 16), warp.rotation((30, 20), (17, 16), 30.0, 0.9), warp.BICUBIC, FILL)]
WARPS_SUPER = [warp.item(SPRITE, (20, 17, 100, 50), (33, 18), warp.rotation((100, 50), (33, 18), 30.0, 0.3), warp.SUPER2, FILL),
               warp.item(SPRITE, (0, 40, 130, 30), (41, 29), warp.rotation((130, 30), (41, 29), -20.0, 0.25), warp.SUPER4, FILL),
               warp.item(RGB, (3, 9, 30, 20), (17, 16), warp.rotation((30, 20), (17, 16), 30.0, 0.5), warp.SUPER2 | warp.REPLICATE, 0),
               warp.item(NOISE, (0, 13, 64, 35), (41, 29), warp.rotation((64, 35), (41, 29), -20.0, 0.4), warp.SUPER4 | warp.REPLICATE, 0),
               warp.item(NOISE, (8, 13, 33, 30), (23, 29), warp.rotation((33, 30), (23, 29), 90.0, 0.4), warp.SUPER2 | warp.REFLECT, FILL),
               warp.item(LABEL, (5, 3, 63, 41), (33, 18), warp.rotation((63, 41), (33, 18), 30.0, 0.3), warp.SUPER4 | warp.REFLECT, FILL),
               warp.item(COLUMN, (0, 3, 1, 90), (5, 29), warp.rotation((1, 90), (5, 29), 10.0, 0.2), warp.SUPER2 | warp.REFLECT_101, FILL),
               warp.item(LABEL3, (2, 1, 33, 25), (20, 15), warp.rotation((33, 25), (20, 15), -15.0, 0.3), warp.SUPER4 | warp.REFLECT_101, FILL),
               warp.item(RGB, (1, 4, 35, 24), (19, 18), (3 * ONE, 23000, -2 * ONE * 35 * 40 - 40000, -9000, 3 * ONE + 700, 2 * ONE * 24 * 9 + 12345), warp.SUPER2 | warp.WRAP, FILL),
               warp.item(TINY, (0, 0, 1, 1), (2, 2), warp.IDENTITY, warp.SUPER4 | warp.WRAP, 0),
               warp.item(SPRITE, (20, 17, 100, 50), (33, 18), warp.rotation((100, 50), (33, 18), -30.0, 0.3), 0, FILL),
               warp.item(LABEL, (1, 0, 64, 45), (33, 18), warp.rotation((64, 45), (33, 18), 30.0, 0.9), warp.NEAREST | warp.REPLICATE, 0),
               warp.item(NOISE, (3, 6, 40, 30), (17, 16), warp.rotation((40, 30), (17, 16), 45.0, 0.7), warp.BICUBIC, FILL),
               warp.item(RGB, (3, 9, 30, 20), (17, 16), warp.rotation((30, 20), (17, 16), 30.0, 0.4), warp.REFLECT | warp.BICUBIC, FILL)]


def leaves_by_periods(it):
    """how many periods of its border the farthest tap of an item lies from the rectangle, the larger of the two axes: above 2 the fold takes its
    quotient estimate (qoi_warp_border_core.h: warp_fold_position), up to 1 its conditional add or subtract alone"""
    _, _, _, cw, rh, ow, oh, flags, a, b, d, e, _, _, c, f = it
    U, V = (2 * np.arange(ow, dtype=np.int64) + 1)[None, :], (2 * np.arange(oh, dtype=np.int64) + 1)[:, None]
    worst = 0
    for P, n in ((a * U + b * V + c, cw), (d * U + e * V + f, rh)):
        period = {warp.REFLECT: 2 * n, warp.REFLECT_101: max(2 * n - 2, 1), warp.WRAP: n}[flags & warp.BORDERS]
        k = (P - (0 if flags & warp.NEAREST else ONE)) >> 17
        worst = max(worst, int(-k.min()) // period, int(k.max()) // period)
    return worst


assert {(it[7] & warp.BORDERS, it[7] & ~warp.BORDERS) for it in WARPS_BORDER} >= {(b, s) for b in FOLDING for s in SAMPLINGS}
assert {0, warp.REPLICATE, warp.BICUBIC} <= {it[7] for it in WARPS_BORDER} and not any(it[7] & warp.SUPERS for it in WARPS_BORDER)
_far = [leaves_by_periods(it) for it in WARPS_BORDER if it[7] & warp.BORDERS & ~warp.REPLICATE]
assert sum(n > 2 for n in _far) >= 2 and sum(n <= 1 for n in _far) >= 2, _far         # (the column of width 1 has a period of 1 or 2: far as well)
assert {(it[7] & warp.SUPERS, it[7] & warp.BORDERS) for it in WARPS_SUPER if it[7] & warp.SUPERS} == {(s, b) for s in (warp.SUPER2, warp.SUPER4) for b in (0, warp.REPLICATE) + FOLDING}
assert {it[7] for it in WARPS_SUPER if not it[7] & warp.SUPERS} == {0, warp.NEAREST | warp.REPLICATE, warp.BICUBIC, warp.REFLECT | warp.BICUBIC}
assert all(it[5] <= 41 and it[6] <= 29 for it in WARPS_BORDER + WARPS_SUPER)
# The items of the newer filters of qoimi_decode_tensors: ITEMS whole - no filter's `size` rejects one of them: the largest reduction is
# 97 to 13 (the filters stop at 16), the largest side 130 (they stop at 16384) - and rectangles of the label maps, where FILTER_MODE has
# majorities and ties in cells of 1 to 16 x 15 pixels (the items of tests/mode_cases.py among them)
LABEL_ITEMS = [(LABEL, 0, 0, 70, 45, 16, 11, 1), (LABEL, 3, 5, 31, 23, 7, 20, 2), (LABEL, 1, 0, 64, 45, 4, 3, 0), (LABEL3, 0, 0, 37, 29, 9, 7, 3), (LABEL3, 0, 0, 37, 29, 50, 7, 0)]
FILTERS = {"resized": FILTER_AREA, "bilinear": FILTER_BILINEAR, "bicubic": FILTER_BICUBIC, "lanczos": FILTER_LANCZOS, "nearest": FILTER_NEAREST, "mode": FILTER_MODE}
NEWER = {"bicubic": ITEMS + LABEL_ITEMS, "lanczos": ITEMS + LABEL_ITEMS, "nearest": ITEMS + LABEL_ITEMS, "mode": ITEMS + LABEL_ITEMS,
         "warped_cubic": WARPS_CUBIC, "warped_nearest": WARPS_NEAREST, "warped_border": WARPS_BORDER, "warped_super": WARPS_SUPER}
_MODELS = {}


def resample(decoded, kind, it, och, mode):
    """the u8 result of one item by the definition; decoded(i, och) is the oracle's decode of image i as uint8[h, w, och]"""
    if kind == "mode":                                                # the vote is over the 4-channel decode; och 3 drops alpha afterwards
        return mode_filter.mode(decoded(it[0], 4), it[1:5], it[5:7], it[7], och=och)
    D = decoded(it[0], och)
    if kind == "thumbnails":
        return thumbs.thumbnail(D, it[1], mode)
    if kind == "crops":
        return crops.crop(D, it[1:5], it[5])
    if kind.startswith("warped"):
        _, x, y, cw, rh, ow, oh, flags, a, b, d, e, fill, _, c, f = it
        return warp.warp(D, (x, y, cw, rh), (ow, oh), (a, b, c, d, e, f), flags, fill, mode)
    return tensors.tensors(D, it[1:5], it[5:7], it[7], FILTERS[kind], mode)      # (U8, HWC: the filter's own bytes)


def model(p, kind, it, och, mode):
    """the u8 result of one item by the definition: computed once, shared, never changed"""
    key = (kind, tuple(it), och, mode)
    if key not in _MODELS:
        P = np.ascontiguousarray(resample(p.decoded, kind, it, och, mode))
        P.setflags(write=False)
        _MODELS[key] = P
    return _MODELS[key]


GATHERS = {"crops": CROPS, "resized": ITEMS, "bilinear": ITEMS, "warped": WARPS, "warped_cubic": WARPS_CUBIC, "warped_nearest": WARPS_NEAREST,
           "warped_border": WARPS_BORDER, "warped_super": WARPS_SUPER}


def gather_call(ctx, kind, streams, so, p, och, mode, index=None):
    """call(out, offsets) of one u8 gather call over the pack at streams + so, plain or - index (intervals, points, firsts) - indexed"""
    items = GATHERS[kind]
    if kind == "crops":
        if index is None:
            return lambda out, oo: ctx.decode_crops(streams, so, p.sizes, p.descs, och, items, out, oo)
        return lambda out, oo: ctx.decode_crops_indexed(streams, so, p.sizes, p.descs, och, items, out, oo, *index)
    f = getattr(ctx, "decode_" + kind.split("_")[0] + ("_indexed" if index is not None else ""))
    return lambda out, oo: f(streams, so, p.sizes, p.descs, och, items, mode, out, oo, *(index or ()))


def test_the_decoys_of_the_newer_items_differ(oracle):
    """(no GPU) At the alias of a stream beyond B32 stands the oracle's stream of the decoy pixels.  For every item of the newer filters and
    warp samplings, at every channel count and alpha mode its calls use: the decoy's decode resamples to other bytes than the true decode,
    so a reader that dropped the high half of a stream offset fails a comparison whichever image lies beyond B32."""
    px = pack_pixels()
    decodes = {}

    def decoder(pixels):
        def decoded(i, och):
            if (id(pixels), i, och) not in decodes:
                w, h, ch = SHAPES[i]
                decodes[(id(pixels), i, och)] = oracle.decode(oracle.encode(pixels[i], w, h, ch), och)[0].reshape(h, w, och)
            return decodes[(id(pixels), i, och)]
        return decoded

    true, decoy = decoder(px), decoder([other(a) for a in px])
    assert all(np.array_equal(true(i, ch).reshape(-1), px[i]) for i, (_, _, ch) in enumerate(SHAPES))
    checked = 0
    for kind, items in NEWER.items():
        combos = {(och, mode) for _, _, och, mode in FORMATS[kind]} | ({(4, 1), (3, 0)} if kind in GATHERS else set())
        assert {it[0] for it in items} == set(range(len(SHAPES)))                      # whichever image straddles or lies beyond: it has an item
        for och, mode in sorted(combos):
            for j, it in enumerate(items):
                assert not np.array_equal(resample(true, kind, it, och, mode), resample(decoy, kind, it, och, mode)), (kind, och, mode, j)
                checked += 1
    assert checked >= 4 * 2 * len(ITEMS + LABEL_ITEMS) + 2 * (len(WARPS_CUBIC) + len(WARPS_NEAREST) + len(WARPS_BORDER) + len(WARPS_SUPER))


def assert_streams_high(so, sizes):
    """stream_offsets of the call: one stream lies across byte B32, others begin beyond it"""
    assert any(o >= B32 for o in so) and any(o < B32 < o + n for o, n in zip(so, sizes))


@gpu
def test_u8_gathers(ctx, oracle, pack, src, dst):
    p = pack
    so = place_pack(src, oracle, p)
    assert_streams_high(so, p.sizes)
    base = src.t.data_ptr()
    for och, mode in ((4, 1), (3, 0)):
        want = [model(p, "thumbnails", (i, f), och, mode) for i, f in enumerate(FACTORS)]
        into_dst(dst, want, lambda out, oo: ctx.decode_thumbnails(base, so, p.sizes, p.descs, och, FACTORS, mode, out, oo), ("thumbnails", och))
        for kind, items in GATHERS.items():
            into_dst(dst, [model(p, kind, it, och, mode) for it in items], gather_call(ctx, kind, base, so, p, och, mode), (kind, och, mode))
    src.check()


OLDER_FORMATS = ((F16, HWC, 4, 1), (F32, CHW, 3, 0), (F16, CHW, 3, 0), (F32, HWC, 4, 1))
# (dtype, layout, output channels, alpha mode) of the calls of each kind; every call has a straddling output and outputs beyond B32.  All
# filters and both warp kernels take every dtype with every layout and either channel count (qoi_host_tensor.hip: tensor_format_wrong looks
# at the format alone; the integer dtypes want scale 1 and bias +0), so the formats are spread: four a kind, and over the newer kinds every
# dtype and every layout
FORMATS = {"resized": OLDER_FORMATS, "bilinear": OLDER_FORMATS, "warped": OLDER_FORMATS,
           "bicubic": ((F16, HWC, 4, 1), (F32, CHW, 3, 0), (BF16, HW, 4, 0), (I64, CHW, 3, 0)),
           "lanczos": ((BF16, HWC, 4, 1), (F32, CHW, 3, 0), (I32, HW, 3, 0), (U8, HWC, 4, 0)),
           "nearest": ((I64, HW, 4, 0), (I32, CHW, 3, 0), (U8, HWC, 3, 0), (F16, CHW, 4, 1)),
           "mode": ((I64, HW, 3, 0), (I32, HWC, 4, 0), (U8, CHW, 4, 1), (BF16, HWC, 3, 0)),
           "warped_cubic": ((F16, HWC, 4, 1), (F32, CHW, 3, 0), (I64, HW, 4, 1), (U8, CHW, 3, 0)),
           "warped_nearest": ((I64, HW, 4, 0), (I32, CHW, 3, 0), (BF16, HWC, 4, 1), (U8, HW, 3, 0)),
           "warped_border": ((BF16, HWC, 4, 1), (U8, CHW, 3, 0), (I32, HW, 4, 0), (F32, CHW, 3, 0)),
           "warped_super": ((I64, HW, 3, 0), (F16, CHW, 4, 1), (BF16, HWC, 3, 0), (I32, CHW, 4, 1))}
assert {f[0] for k in ("bicubic", "lanczos", "nearest", "mode") for f in FORMATS[k]} == {U8, F16, BF16, F32, I32, I64}
assert {f[0] for k in ("warped_cubic", "warped_nearest") for f in FORMATS[k]} == {U8, F16, BF16, F32, I32, I64}
assert {f[0] for k in ("warped_border", "warped_super") for f in FORMATS[k]} == {U8, F16, BF16, F32, I32, I64}
assert all(len(FORMATS[k]) == 4 for k in ("warped_border", "warped_super"))
assert all({f[1] for f in FORMATS[k]} == {HWC, CHW, HW} for k in NEWER) and all({f[2] for f in FORMATS[k]} == {3, 4} for k in FORMATS)


def format_of(dtype, order):
    return tensors.fmt(dtype, order) if dtype in (U8, I32, I64) else (dtype, order, *IMAGENET)


@gpu
@pytest.mark.parametrize("kind", list(FORMATS))
def test_tensors(ctx, oracle, pack, src, dst, kind):
    p, items = pack, NEWER[kind] if kind in NEWER else GATHERS[kind]
    so = place_pack(src, oracle, p)
    base = src.t.data_ptr()
    assert_streams_high(so, p.sizes)
    for dtype, order, och, mode in FORMATS[kind]:
        f = format_of(dtype, order)
        want = [tensors.convert(model(p, kind, it, och, mode), f) for it in items]
        if kind.startswith("warped"):
            call = lambda out, oo: ctx.decode_warped_tensors(base, so, p.sizes, p.descs, och, items, mode, f, out, oo)      # noqa: E731
        else:
            call = lambda out, oo: ctx.decode_tensors(base, so, p.sizes, p.descs, och, items, FILTERS[kind], mode, f, out, oo)      # noqa: E731
        elem = tensors.elem(dtype)
        oo = layout([flat(w).size for w in want], elem)                # what into_dst lays out: asserted here where a reviewer looks for it
        assert any(o >= B32 for o in oo) and any(o < B32 < o + flat(w).size and (B32 - o) % elem == 0 and (B32 - o) // elem % 2 == 1 for o, w in zip(oo, want))
        into_dst(dst, want, call, (kind, "tensors", dtype, order, och), elem=elem)
        assert ctx.tensor_stats()[:2] == (1, 1)
    src.check()


@gpu
def test_indexed_gathers(ctx, oracle, pack, src, dst):
    """the index is built over the high pack; every indexed call gives what the plain call gives (test_u8_gathers: the same items, the same
    expectations), and each image with seek rows has items that begin below one"""
    from qoi_amd import seekindex as si
    p = pack
    so = place_pack(src, oracle, p)
    assert_streams_high(so, p.sizes)
    base = src.t.data_ptr()
    points, firsts = ctx.build_seek_index(base, so, p.sizes, p.descs, INTERVALS)
    want = [si.points(p.streams[i].tobytes(), w, h, K, p.decoded(i, 4)) for i, ((w, h, _), K) in enumerate(zip(SHAPES, INTERVALS))]
    assert [len(x) for x in want] == [0, 0, 7, 8, 7, 0, 0] and firsts == [0, 0, 0, 7, 15, 22, 22] and points.tobytes() == np.concatenate(want).tobytes()
    assert all(any(it[0] == i and it[2] >= INTERVALS[i] for it in items) for items in GATHERS.values() for i in (RGB, SPRITE, NOISE))
    index = (INTERVALS, points, firsts)
    for och, mode in ((4, 1), (3, 0)):
        for kind, items in GATHERS.items():
            into_dst(dst, [model(p, kind, it, och, mode) for it in items], gather_call(ctx, kind, base, so, p, och, mode, index), (kind, "indexed", och, mode))
            assert ctx.seek_stats()[1] == len({it[0] for it in items})
    src.check()


@gpu
def test_pixel_stats(ctx, oracle, pack, src, dst):
    p = pack
    so = place_pack(src, oracle, p)
    regions = CROPS + [(i, 0, 0, w, h, i & 3) for i, (w, h, _) in enumerate(SHAPES)]
    got = ctx.pixel_stats(src.t.data_ptr(), so, p.sizes, p.descs, regions)
    for j, r in enumerate(regions):
        want = ps.stats(p.decoded(r[0], 4), r)
        assert ps.of_struct(got[j]) == want, (j, r)
        if so[r[0]] + p.sizes[r[0]] > B32:
            assert ps.stats(p.decoy_decoded[r[0]], r) != want, (j, r)
    assert dst.clean()
    src.check()


# ------------------------------------------------------------------ 3: the seek index and the band streams
@pytest.fixture(scope="module")
def seek(api, oracle):
    """the cases of tests/seek_cases.py that the band-stream tests keep, but the cut stream (no encoder wrote it from its pixels); decoys: the
    oracle's streams of other pixels"""
    keep = ("noise96", "skip1", "skip61", "all_ff", "old_colour", "w1", "w63", "w65", "no_point")
    cs = [c for c in seek_cases(oracle) if c.name in keep]
    cs.sort(key=lambda c: c.name != "no_point")                     # in front: a control placement - without a point no decoy can differ
    for c in cs:
        c.px = flat(c.full[c.ch])
        c.decoy_px = other(c.px)
        c.decoy = oracle.encode(c.decoy_px, c.w, c.h, c.ch)
        c.desc = api.QoiDesc(c.w, c.h, c.ch, 0)
    return cs


def place_cases(src, oracle, cs, **how):
    return place_streams(src, oracle, [c.stream for c in cs], [c.decoy for c in cs], [(c.w, c.h, c.ch) for c in cs], [c.full[c.ch] for c in cs], **how)


@gpu
def test_seek_index_builds(ctx, oracle, seek, src, dst):
    cs = seek
    sizes, descs, Ks = [len(c.stream) for c in cs], [c.desc for c in cs], [c.K for c in cs]
    want = np.concatenate([c.points for c in cs])
    want_firsts = [int(x) for x in np.cumsum([0] + [len(c.points) for c in cs[:-1]])]
    for turn in (0, 1):                                             # the straddling item: a stream, then an image
        so = place_cases(src, oracle, cs, straddle=turn == 0)
        assert so[0] + sizes[0] <= B32 and len(cs[0].points) == 0
        po = layout([c.px.size for c in cs], lane=1, straddle=turn == 1)
        src.place(po, [c.px for c in cs], [c.decoy_px for c in cs])
        if turn == 0:
            points, firsts = ctx.build_seek_index(src.t.data_ptr(), so, sizes, descs, Ks)
            assert firsts == want_firsts and points.tobytes() == want.tobytes(), "build_seek_index"
        points, firsts = ctx.seek_index_from_pixels(src.t.data_ptr(), po, src.t.data_ptr(), so, sizes, descs, Ks)
        assert firsts == want_firsts and points.tobytes() == want.tobytes(), ("seek_index_from_pixels", turn)
        src.check()
        src.clear()
    assert dst.clean()


@gpu
def test_band_streams(ctx, oracle, seek, src, dst):
    cs = seek
    so = place_cases(src, oracle, cs)
    bands = []
    for i, c in enumerate(cs):
        n = len(c.points)
        bands.append((i, 0, min(c.K, c.h)))
        for k in sorted({n // 2, n - 1} & set(range(n))):
            first = (k + 1) * c.K
            bands += [(i, first, c.h - first), (i, first, 1)]
    want = [cs[i].band(first, rows) for i, first, rows in bands]
    pts = np.concatenate([c.points for c in cs])
    firsts = [int(x) for x in np.cumsum([0] + [len(c.points) for c in cs[:-1]])]
    infos = into_dst(dst, [s for s, _ in want],
                     lambda out, oo: ctx.make_band_streams(src.t.data_ptr(), so, [len(c.stream) for c in cs], [c.desc for c in cs], [c.K for c in cs], pts, firsts,
                                                           bands, out, oo), "make_band_streams")
    for (i, first, rows), (s, pad), info in zip(bands, want, infos):
        assert (info.size, info.pad_rows, info.desc.width, info.desc.height, info.desc.channels) == (len(s), pad, cs[i].w, pad + rows, cs[i].ch)
    src.check()


# ------------------------------------------------------------------ 4: verify and compare
def diffs_of(a, b, shapes, ca, cb):
    """imagediff.diff image by image as the records the calls return, and the first flagged index"""
    out = np.zeros(len(a), dtype=DIFF_DTYPE)
    first = -1
    for i, (x, y, (w, h)) in enumerate(zip(a, b, shapes)):
        m, f, want, got = diff(x, y, w * h, ca[i], cb[i])
        out[i] = (m, f, want, got, DIFF_PIXELS if m else 0, 0)
        if m and first < 0:
            first = i
    return out, first


@gpu
def test_verify_images(ctx, oracle, pack, src, dst):
    p, b = pack, pack.b
    shapes, chs = [(w, h) for w, h, _ in SHAPES], [ch for _, _, ch in SHAPES]
    for turn in (0, 1):                                             # the straddling item: a stream, then an image
        so = place_pack(src, oracle, p, straddle=turn == 0)
        po = layout([px.size for px in b.px], lane=1, straddle=turn == 1)
        src.place(po, b.px, p.decoy_px)
        got, first = ctx.verify_images(src.t.data_ptr(), po, b.descs, src.t.data_ptr(), so, p.sizes)
        assert first == -1 and not got["flags"].any() and not got["mismatched"].any() and (got["first"] == NONE).all(), ("clean", turn)
        src.check()
        src.clear()
        # one byte of an image differs from its stream in the high copy only: at the alias stand the very pixels of the stream
        so = place_pack(src, oracle, p, straddle=turn == 0)
        planted, clean_at_alias = [px.copy() for px in b.px], list(p.decoy_px)
        j = max(i for i in range(b.n) if po[i] + b.px[i].size > B32 and b.px[i].size > 16)
        at = b.px[j].size - 6 if po[j] >= B32 else B32 - po[j] + 4   # beyond B32 in either placement
        planted[j][at] ^= 0x10
        clean_at_alias[j] = b.px[j]
        src.place(po, planted, clean_at_alias)
        assert np.array_equal(src.misread(po[j], b.px[j].size), b.px[j])
        got, first = ctx.verify_images(src.t.data_ptr(), po, b.descs, src.t.data_ptr(), so, p.sizes)
        want, want_first = diffs_of(planted, [p.decoded(i, ch).reshape(-1) for i, ch in enumerate(chs)], shapes, chs, chs)
        assert want_first == j and int(want[j]["mismatched"]) == 1 and int(want[j]["first"]) == at // chs[j]
        assert first == want_first and all(got[i] == want[i] for i in range(b.n)), ("planted", turn, j, got[j], want[j])
        src.check()
        src.clear()
    assert dst.clean()


@gpu
def test_compare_images(api, ctx, pack, src, dst):
    """side A with 4 bytes per pixel, side B with 3; B's copies beyond B32 differ from A in one byte each, and their aliases do not"""
    shapes = [(w, h) for w, h, _ in SHAPES]
    rng = np.random.default_rng(11)
    A = [rng.integers(0, 256, size=(w * h, 4), dtype=np.uint8) for w, h in shapes]
    descs = [api.QoiDesc(w, h, 4, 0) for w, h in shapes]
    for turn in (0, 1):
        ao = layout([a.size for a in A], lane=0, straddle=turn == 0)
        bo = layout([a.shape[0] * 3 for a in A], lane=1, straddle=turn == 1)
        B = [a[:, :3].copy() for a in A]
        for i, o in enumerate(bo):
            if o + B[i].size > B32:
                B[i].reshape(-1)[B[i].size - 2] ^= 0x04            # the last pixel: beyond B32 in either placement
        src.place(ao, A, [other(a) for a in A])
        src.place(bo, B, [a[:, :3] for a in A])
        got, first = ctx.compare_images(src.t.data_ptr(), ao, 4, src.t.data_ptr(), bo, 3, descs)
        want, want_first = diffs_of(A, B, shapes, [4] * len(A), [3] * len(A))
        high = [i for i, o in enumerate(bo) if o + B[i].size > B32]
        assert len(high) >= 2 and want_first == high[0] and all(int(want[i]["mismatched"]) == (i in high) for i in range(len(A)))
        assert first == want_first and all(got[i] == want[i] for i in range(len(A))), (turn, got, want)
        src.check()
        src.clear()
    assert dst.clean()


# ------------------------------------------------------------------ 5: single outputs longer than 4 GiB
@pytest.fixture(scope="module")
def sources(api, ctx, oracle):
    """the three sources of part 2: 41 x 41 noise, 64 x 48 noise, a 64 x 64 constant"""
    constant = np.empty((64, 64, 4), dtype=np.uint8)
    constant[:] = CONSTANT
    rect = np.random.default_rng(6448).integers(0, 256, size=(48, 64, 4), dtype=np.uint8)
    return Pack(ctx, oracle, batch_of(api, oracle, [(41, 41, 4), (64, 48, 4), (64, 64, 4)], [noise41(), rect, constant]))


def words_of(t, at, nbytes):
    import torch
    return t[at:at + nbytes].view(torch.int32)


def guards_stand(t, at, nbytes):
    return bool((t[:at] == GUARD).all()) and bool((t[at + nbytes:] == GUARD).all())


def assert_words(got, want, what):
    """two int32 device tensors of equal shape are equal; else where they first differ"""
    import torch
    if not torch.equal(got, want):
        k = first_true(got.reshape(-1) != want.reshape(-1))
        raise AssertionError(f"{what}: element {k} = 2^30 {k - (1 << 30):+d} of {got.numel()} is {int(got.reshape(-1)[k]):#x}, not {int(want.reshape(-1)[k]):#x}")


def big_area(ctx, p, t, at, flags):
    """item 1 into t at byte `at`: the 41 x 41 image 400-fold, flipped by flags"""
    import torch
    ctx.decode_tensors(p.packed.data_ptr(), p.so, p.sizes, p.descs, 4, [(0, 0, 0, 41, 41, SIDE, SIDE, flags)], FILTER_AREA, flags & 1, F32_CHW, t.data_ptr(), [at])
    small = tensors.convert(resize.resize(p.decoded(0, 4), (0, 0, 41, 41), (41, 41), flags, flags & 1), F32_CHW)
    want = torch.from_numpy(small.view(np.int32)).cuda().repeat_interleave(400, dim=1).repeat_interleave(400, dim=2)
    assert_words(words_of(t, at, BIG_BYTES).view(4, SIDE, SIDE), want, ("area", flags))
    assert guards_stand(t, at, BIG_BYTES), ("area", flags)


def big_tent(ctx, p, t, at):
    """item 3 into t at byte `at`: four constant planes"""
    import torch
    ctx.decode_tensors(p.packed.data_ptr(), p.so, p.sizes, p.descs, 4, [(2, 0, 0, 64, 64, SIDE, SIDE, 0)], FILTER_BILINEAR, 0, F32_CHW, t.data_ptr(), [at])
    values = tensors.convert(np.array(CONSTANT, dtype=np.uint8).reshape(1, 1, 4), F32_CHW).view(np.int32).reshape(4)
    assert len(set(values.tolist())) == 4
    got = words_of(t, at, BIG_BYTES).view(4, SIDE * SIDE)
    for c in range(4):
        if not bool((got[c] == int(values[c])).all()):
            k = first_true(got[c] != int(values[c]))
            raise AssertionError(f"tent: element {k} of plane {c} (byte {(c * SIDE * SIDE + k) * 4 - B32:+d} from 2^32) is {int(got[c][k]):#x}, not {int(values[c]):#x}")
    assert guards_stand(t, at, BIG_BYTES), "tent"


def release():
    import torch
    torch.cuda.empty_cache()


@gpu
def test_area_f32_chw_longer_than_4gib(ctx, sources):
    for flags in (1, 2):
        t = filled(BIG_BYTES + 2 * PAGE, GUARD)
        big_area(ctx, sources, t, PAGE, flags)
        del t
        release()


@gpu
def test_warp_f32_hwc_longer_than_4gib(ctx, sources):
    import torch
    p = sources
    t = filled(BIG_BYTES + 2 * PAGE, GUARD)
    ctx.decode_warped_tensors(p.packed.data_ptr(), p.so, p.sizes, p.descs, 4, [warp.item(1, (0, 0, 64, 48), (SIDE, SIDE), warp.IDENTITY, 0, FILL)], warp.PLAIN,
                              F32_HWC, t.data_ptr(), [PAGE])
    corner = tensors.convert(warp.warp(p.decoded(1, 4), (0, 0, 64, 48), (80, 64), warp.IDENTITY, 0, FILL, warp.PLAIN), F32_HWC)
    fill = tensors.convert(np.array([FILL >> (8 * k) & 255 for k in range(4)], dtype=np.uint8).reshape(1, 1, 4), F32_HWC)
    assert np.array_equal(corner[63, 79], fill[0, 0]) and len(set(fill.view(np.int32).reshape(4).tolist())) == 4
    want = torch.from_numpy(fill.view(np.int32).reshape(4)).cuda().expand(SIDE, SIDE, 4).contiguous()
    want[:64, :80] = torch.from_numpy(corner.view(np.int32)).cuda()
    assert_words(words_of(t, PAGE, BIG_BYTES).view(SIDE, SIDE, 4), want, "warp")
    assert guards_stand(t, PAGE, BIG_BYTES), "warp"
    del t, want
    release()


@gpu
def test_tent_f32_chw_longer_than_4gib(ctx, sources):
    t = filled(BIG_BYTES + 2 * PAGE, GUARD)
    big_tent(ctx, sources, t, PAGE)
    del t
    release()


# ------------------------------------------------------------------ 6: a single source longer than 4 GiB
BIG_FILL = 0x3E                 # as f32 0x3E3E3E3E = 0.18578...: UNIT gives 47.37...
BIG_FILL_BYTE = 47
assert ingest_cases.BIG_SIDE == SIDE


def big_windows(order):
    """(true, decoys): lists of (first element, float32 elements) - whole rows of the image, of every plane for CHW (the decoys: of the
    first plane, where the aliases of the fourth lie)"""
    rng = np.random.default_rng(64 + order)
    win = ingest_cases.BIG_WINDOWS[order]

    def rows(r0, r1, planes):
        if order == tiles.HWC:
            return [(r0 * SIDE * 4, rng.uniform(-0.25, 1.25, size=(r1 - r0) * SIDE * 4).astype(np.float32))]
        return [((c * SIDE + r0) * SIDE, rng.uniform(-0.25, 1.25, size=(r1 - r0) * SIDE).astype(np.float32)) for c in planes]

    true = [w for name in ("control", "straddle", "last") for w in rows(*win[name], range(4))]
    return true, [w for r0, r1 in win["decoys"] for w in rows(r0, r1, (0,))]


def big_gather(windows, idx, fill):
    """the elements at the indices idx by the construction"""
    out = np.full(idx.shape, fill, dtype=np.float32)
    for start, a in windows:
        m = (idx >= start) & (idx < start + a.size)
        out[m] = a[idx[m] - start]
    return out


@gpu
@pytest.mark.parametrize("order", [tiles.HWC, tiles.CHW], ids=["hwc", "chw"])
def test_encode_tiles_f32_source_longer_than_4gib(api, ctx, oracle, order):
    import torch
    fill = np.frombuffer(bytes([BIG_FILL]) * 4, dtype=np.float32)[0]
    assert int(tiles.to_bytes(fill, tiles.UNIT)) == BIG_FILL_BYTE and 0.18 < float(fill) < 0.19
    true, decoys = big_windows(order)
    t = filled(BIG_BYTES + 2 * PAGE, BIG_FILL)
    assert t.data_ptr() % 256 == 0 and PAGE % 256 == 0
    for start, a in true + decoys:
        assert 0 <= start and (start + a.size) * 4 <= BIG_BYTES
        t[PAGE + 4 * start:PAGE + 4 * (start + a.size)].copy_(torch.from_numpy(a.view(np.uint8)))
    named = ingest_cases.big_tiles(order)
    ts = [tile for _, tile in named]
    desc = api.QoiDesc(SIDE, SIDE, 4, 0)
    hwc = tiles.source_flags(tiles.F32, tiles.HWC, tiles.UNIT)
    wrapped_tiles = 0
    for channels in ingest_cases.BIG_CHANNELS:
        px = []
        for name, (_, x, y, cw, ch, _, flags) in named:
            idx = ingest_cases.big_index(order, y + np.arange(ch, dtype=np.int64)[:, None, None], x + np.arange(cw, dtype=np.int64)[None, :, None],
                                         np.arange(4, dtype=np.int64)[None, None, :])
            window = (0, 0, 0, cw, ch, 1, hwc | (flags & 3))
            p = tiles.tile(big_gather(true, idx, fill), window, channels)
            if name == "fill":
                assert np.all(p[:, :, :3] == BIG_FILL_BYTE)
            else:
                assert all(any(start <= int(i) < start + a.size for start, a in true) for i in (idx.min(), idx.max()))
            if idx.max() * 4 >= B32:                               # what a byte offset cut to 32 bits reads: the decoys, another tile
                low = np.where(idx * 4 >= B32, idx - (B32 >> 2), idx)
                assert all(any(start <= int(i) < start + a.size for start, a in decoys) for i in (low[idx * 4 >= B32].min(), low[idx * 4 >= B32].max()))
                if order == tiles.HWC or channels != 3:             # (of a CHW image the fourth plane alone lies there: och 3 drops it)
                    assert not np.array_equal(tiles.tile(big_gather(true + decoys, low, fill), window, channels), p), (name, flags)
                    wrapped_tiles += 1
            else:
                assert name in ("control", "fill")
            px.append(p)
        want = [oracle.encode(p.reshape(-1), p.shape[1], p.shape[0], p.shape[2], 0) for p in px]
        lens = [len(s) for s in want]
        want_off = pack_offsets(lens, 1)
        pack = filled(int(want_off[-1]) + 2 * PAGE, GUARD)
        off = torch.full((len(ts) + 1,), -1, dtype=torch.int64, device="cuda")
        d_len = torch.full((len(ts),), -1, dtype=torch.int32, device="cuda")
        got_off, got_len, _ = ctx.encode_tiles(t.data_ptr(), [PAGE], [desc], channels, ts, tiles.PLAIN, 1, pack.data_ptr() + PAGE, int(want_off[-1]),
                                               off.data_ptr(), d_len.data_ptr())
        what = ("a source longer than 4 GiB", order, channels)
        assert np.array_equal(got_off, want_off) and got_len.tolist() == lens and d_len.cpu().numpy().tolist() == lens, what
        host = pack.cpu().numpy()
        assert_bytes([host[PAGE + int(o):PAGE + int(o) + n] for o, n in zip(want_off[:-1], lens)], want, what)
        assert np.all(host[:PAGE] == GUARD) and np.all(host[PAGE + int(want_off[-1]):] == GUARD), what
        assert ctx.tile_stats()[:2] == (1, 1), what
    assert wrapped_tiles == 2 * 4 * (2 if order == tiles.HWC else 1) and ingest_cases.BIG_CHANNELS == (0, 3)
    for start, a in true + decoys:                                     # the source is only read
        assert np.array_equal(t[PAGE + 4 * start:PAGE + 4 * (start + a.size)].cpu().numpy(), a.view(np.uint8)), start
    assert bool((t[:PAGE] == BIG_FILL).all()) and bool((t[PAGE + BIG_BYTES:] == BIG_FILL).all())
    del t
    release()
