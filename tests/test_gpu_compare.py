"""qoimi_compare_images on the GPU (-m gpu) against qoi_amd/imagediff.py: diff - every channel pairing, both sides at odd byte offsets
independently of each other, guard bytes around the images that DIFFER between the two sides (they must never be counted), differences
planted at the edges of an image and at every boundary a tile size could have."""
import ctypes

import numpy as np
import pytest

from qoi_amd.imagediff import DIFF_PIXELS, NONE, diff
from gpu_pack import dev
from gpu_pack import api, ctx  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1), (1, 97), (131, 1), (37, 23), (257, 9), (64, 48), (333, 7), (300, 300)]
PAIRINGS = [(4, 4), (3, 3), (4, 3), (3, 4)]
SHIFTS = [0, 1, 2, 3, 5]
GAP = 7                                         # guard bytes between two images (odd: every image begins at another residue)
FRONT = 256


class Side:
    """Images tightly packed in one host buffer: FRONT + shift guard bytes, then every image followed by GAP guard bytes; the images may be
    laid out in any order.  guard: the byte the space around the images holds."""

    def __init__(self, images, channels, shift, guard, order=None):
        self.ch = channels
        order = list(range(len(images))) if order is None else order
        self.offsets = [0] * len(images)
        at = FRONT + shift
        for i in order:
            self.offsets[i] = at
            at += images[i].size + GAP
        self.host = np.full(at + 64, guard, dtype=np.uint8)
        for i, im in enumerate(images):
            self.host[self.offsets[i]:self.offsets[i] + im.size] = im.reshape(-1)
        self.dev = dev(self.host)
        assert self.dev.data_ptr() % 256 == 0

    def unchanged(self):
        return np.array_equal(self.dev.cpu().numpy(), self.host)


def base_images(shapes, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, size=(w * h, 4), dtype=np.uint8) for (w, h) in shapes]


def expect(api, imgs_a, imgs_b, ca, cb):
    """the model's answer as an array of records, and first_diff"""
    from qoi_amd.imagediff import DIFF_DTYPE
    out = np.zeros(len(imgs_a), dtype=DIFF_DTYPE)
    first = -1
    for i, (x, y) in enumerate(zip(imgs_a, imgs_b)):
        m, f, want, got = diff(x, y, x.shape[0], ca[i], cb[i])
        out[i] = (m, f, want, got, DIFF_PIXELS if m else 0, 0)
        if m and first < 0:
            first = i
    return out, first


def run(api, ctx, shapes, imgs_a, imgs_b, ca, cb, shift_a=0, shift_b=0, order_a=None, order_b=None, explicit=True):
    """imgs_*: (npx, 4) arrays; side A keeps ca bytes of every pixel, side B cb.  One call, compared with the model; both buffers unchanged."""
    cut_a = [x[:, :ca] for x in imgs_a]
    cut_b = [x[:, :cb] for x in imgs_b]
    A = Side(cut_a, ca, shift_a, 0x11, order_a)
    B = Side(cut_b, cb, shift_b, 0xEE, order_b)                 # the guards differ between the sides
    descs = [api.QoiDesc(w, h, 4, 0) for (w, h) in shapes]
    got, first = ctx.compare_images(A.dev.data_ptr(), A.offsets, ca, B.dev.data_ptr(), B.offsets, cb, descs)
    want, want_first = expect(api, cut_a, cut_b, [ca] * len(shapes), [cb] * len(shapes))
    what = (ca, cb, shift_a, shift_b)
    for i in range(len(shapes)):
        assert got[i] == want[i], (what, shapes[i], got[i], want[i])
    assert first == want_first, what
    assert A.unchanged() and B.unchanged(), what
    return got


def planted(shapes, imgs, kind, rng):
    """a copy of imgs with differences planted; returns the copy"""
    out = [x.copy() for x in imgs]
    for (w, h), x in zip(shapes, out):
        n = w * h
        if kind == "pixel 0":
            x[0, 1] ^= 0x80
        elif kind == "last pixel":
            x[n - 1, 2] ^= 0x01
        elif kind == "alpha only":
            x[n // 2, 3] ^= 0x55
        elif kind == "every pixel":
            x[:, 0] ^= 0x04
        elif kind == "tile boundaries" and n == 300 * 300:
            idx = set()
            for k in range(0, n, 1024):
                idx.update(j for j in (k - 1, k, k + 1) if 0 <= j < n)
            idx.update(int(j) for j in rng.integers(0, n, size=200))
            for j in idx:
                x[j, j % 3] ^= 1 << (j % 8)
    return out


@pytest.fixture(scope="module")
def images():
    return base_images(SHAPES, 20240)


@pytest.mark.parametrize("ca,cb", PAIRINGS)
@pytest.mark.parametrize("kind", ["none", "pixel 0", "last pixel", "alpha only", "tile boundaries", "every pixel"])
def test_planted_differences(api, ctx, images, ca, cb, kind):
    rng = np.random.default_rng(7)
    other = planted(SHAPES, images, kind, rng)
    got = run(api, ctx, SHAPES, images, other, ca, cb, shift_a=1, shift_b=2)
    if kind == "none" or (kind == "alpha only" and (ca, cb) != (4, 4)):
        assert not got["flags"].any() and not got["mismatched"].any() and (got["first"] == NONE).all()
    elif kind == "tile boundaries":
        assert got["mismatched"][-1] > 200 and not got["mismatched"][:-1].any()
    else:
        assert got["flags"].all()
        if kind == "every pixel":
            assert got["mismatched"].tolist() == [w * h for (w, h) in SHAPES]


@pytest.mark.parametrize("ca,cb", PAIRINGS)
def test_every_pair_of_shifts(api, ctx, images, ca, cb):
    """both sides 0, 1, 2, 3 and 5 bytes behind a 256-aligned base, independently; a difference in the first and last pixel of every image
    and at the tile boundaries of the large one"""
    rng = np.random.default_rng(11)
    other = planted(SHAPES, planted(SHAPES, planted(SHAPES, images, "pixel 0", rng), "last pixel", rng), "tile boundaries", rng)
    for sa in SHIFTS:
        for sb in SHIFTS:
            run(api, ctx, SHAPES, images, other, ca, cb, shift_a=sa, shift_b=sb)


def test_channels_from_the_descriptors(api, ctx):
    """a_channels = b_channels = 0: every image at its descriptor's channel count, 3 and 4 in one call; and 0 against 4"""
    shapes = [(37, 23), (64, 48), (1, 1), (131, 1), (300, 300)]
    chans = [3, 4, 4, 3, 3]
    imgs = base_images(shapes, 5)
    rng = np.random.default_rng(3)
    other = planted(shapes, planted(shapes, imgs, "last pixel", rng), "alpha only", rng)
    cut_a = [x[:, :c] for x, c in zip(imgs, chans)]
    cut_b = [x[:, :c] for x, c in zip(other, chans)]
    full_b = [x for x in other]
    A, B, B4 = Side(cut_a, 0, 3, 0x11), Side(cut_b, 0, 1, 0xEE), Side(full_b, 4, 2, 0x77)
    descs = [api.QoiDesc(w, h, c, 0) for (w, h), c in zip(shapes, chans)]
    got, first = ctx.compare_images(A.dev.data_ptr(), A.offsets, 0, B.dev.data_ptr(), B.offsets, 0, descs)
    want, want_first = expect(api, cut_a, cut_b, chans, chans)
    assert all(got[i] == want[i] for i in range(len(shapes))) and first == want_first == 0
    assert got["mismatched"].tolist() == [1, 2, 1, 1, 1]                      # alpha counts in the 4-channel images only (1 x 1: one pixel)
    got, first = ctx.compare_images(A.dev.data_ptr(), A.offsets, 0, B4.dev.data_ptr(), B4.offsets, 4, descs)
    want, want_first = expect(api, cut_a, full_b, chans, [4] * len(shapes))
    assert all(got[i] == want[i] for i in range(len(shapes))) and first == want_first
    assert A.unchanged() and B.unchanged() and B4.unchanged()


def test_many_small_images(api, ctx):
    """300 images of 5 x 3 in one call - the image table spans more than a workgroup of cmp_first and every tile another image; a third of
    them differ"""
    shapes = [(5, 3)] * 300
    imgs = base_images(shapes, 99)
    other = [x.copy() for x in imgs]
    for i in range(0, 300, 3):
        other[i][(i * 7) % 15, i % 4] ^= 0x20
    for ca, cb in PAIRINGS:
        got = run(api, ctx, shapes, imgs, other, ca, cb, shift_a=3, shift_b=5)
        if (ca, cb) == (4, 4):
            assert int(got["flags"].astype(bool).sum()) == 100
    rev = list(range(299, -1, -1))
    run(api, ctx, shapes, imgs, other, 4, 4, shift_a=1, order_a=rev)          # ... and side A laid out back to front


def test_same_buffer_and_descending_offsets(api, ctx, images):
    cut = [x[:, :4] for x in images]
    A = Side(cut, 4, 1, 0x11, order=list(range(len(SHAPES) - 1, -1, -1)))     # image 0 lies last
    assert A.offsets == sorted(A.offsets, reverse=True)
    descs = [api.QoiDesc(w, h, 4, 0) for (w, h) in SHAPES]
    p = A.dev.data_ptr()
    got, first = ctx.compare_images(p, A.offsets, 4, p, A.offsets, 4, descs)  # an image against itself
    assert first == -1 and not got["flags"].any() and not got["mismatched"].any() and (got["first"] == NONE).all()
    assert not got["want"].any() and not got["got"].any() and not got["reserved"].any()
    # ... and against its neighbour in the same buffer (overlapping ranges where the neighbour is shorter are fine: nothing is written)
    same = [(64, 48)] * 3
    imgs = base_images(same, 1)
    imgs[2] = imgs[0].copy()
    S = Side(imgs, 4, 2, 0x33)
    d3 = [api.QoiDesc(64, 48, 4, 0)] * 3
    got, first = ctx.compare_images(S.dev.data_ptr(), S.offsets, 4, S.dev.data_ptr(), [S.offsets[2], S.offsets[0], S.offsets[0]], 4, d3)
    want, want_first = expect(api, imgs, [imgs[2], imgs[0], imgs[0]], [4] * 3, [4] * 3)
    assert all(got[i] == want[i] for i in range(3)) and first == want_first == 1
    assert got["flags"].tolist() == [0, DIFF_PIXELS, 0]
    assert A.unchanged() and S.unchanged()


def test_rejections_leave_the_output_untouched(api, ctx, images):
    lib = api.load_library()
    cut = [x[:, :4] for x in images[:2]]
    A = Side(cut, 4, 0, 0x11)
    n = 2
    offs = (ctypes.c_size_t * n)(*A.offsets)
    descs = (api.QoiDesc * n)(*[api.QoiDesc(w, h, 4, 0) for (w, h) in SHAPES[:2]])
    bad = (api.QoiDesc * n)(descs[0], api.QoiDesc(1, 97, 5, 0))
    out = (api.ImageDiff * n)()
    ctypes.memset(out, 0x5A, ctypes.sizeof(out))
    first = ctypes.c_int(7)
    p = A.dev.data_ptr()
    for name, call in {
        "descriptor": lambda: lib.qoimi_compare_images(ctx._h, p, offs, 4, p, offs, 4, bad, n, out, ctypes.byref(first), None),
        "a_channels": lambda: lib.qoimi_compare_images(ctx._h, p, offs, 1, p, offs, 4, descs, n, out, ctypes.byref(first), None),
        "n": lambda: lib.qoimi_compare_images(ctx._h, p, offs, 4, p, offs, 4, descs, 0, out, ctypes.byref(first), None),
    }.items():
        assert call() == -1, name
        assert bytes(out) == b"\x5A" * ctypes.sizeof(out) and first.value == 7, name
    assert lib.qoimi_compare_images(ctx._h, p, offs, 4, p, offs, 4, descs, n, out, None, None) == 0     # first_diff may be NULL
    assert [d.flags for d in out] == [0, 0]
