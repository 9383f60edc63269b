"""QOIMI_TILE_LABELS_ID24 and QOIMI_TENSOR_HW_ID24 through the C interface, what can be checked without a GPU: the constants in every layer
and the header's statement of them; qoimi_tile_size with the bit; qoimi_tensor_size and qoimi_warp_tensor_size with the layout; every new
QOIMI_E_ARG case, reported before the context or the device is looked at - a block of zeroed host memory stands in for a context and host
arrays for device buffers (the idiom of test_label_ingest_api.py and test_labels_api.py) -, with the buffers untouched and
qoimi_last_error naming the cause."""
import ctypes
import os
import re

import pytest

from qoi_amd import api, nearest, tensors, tiles, warp
from model_cases import E_ARG, tl, untouched
from model_cases import args  # noqa: F401  (fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U8, I32, I64 = (tiles.label_flags(d, ids=True) for d in (tiles.L_U8, tiles.L_I32, tiles.L_I64))
ONE4, ZERO4 = (1.0,) * 4, (0.0,) * 4
ID32, ID64 = (tensors.I32, tensors.HW_ID24, ONE4, ZERO4), (tensors.I64, tensors.HW_ID24, ONE4, ZERO4)


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def flat(text):
    return " ".join(re.sub(r"(?m)^\s*(/?\*|//)", " ", text).split())


def test_constants_in_every_layer():
    header = read("include", "qoi_mi355x.h")
    for name, value in (("QOIMI_TILE_LABELS_ID24", 32768), ("QOIMI_TENSOR_HW_ID24", 5), ("QOIMI_TILE_LABELS", 2048), ("QOIMI_TENSOR_HW", 3)):
        m = re.search(r"\b%s\s*=\s*(\d+)" % name, header)
        assert m and int(m.group(1)) == value, name
    assert tiles.LABELS_ID24 == 32768 and tensors.HW_ID24 == 5 and tiles.LABELS_MASK == 0x3800
    core = read("qoi_amd", "csrc", "qoi_label_core.h")
    assert re.search(r"kTileLabelsId24\s*=\s*32768\b", core) and re.search(r"kLabelId24\s*=\s*4\b", core) and re.search(r"kTileLabelsMask\s*=", core)
    assert re.search(r"kTensorHWId24\s*=\s*5\b", read("qoi_amd", "csrc", "qoi_tensor_core.h"))
    kernel = read("qoi_amd", "csrc", "qoi_label.hip")
    for case in ("kLabelId24 | kLabelU8", "kLabelId24 | kLabelI32", "kLabelId24 | kLabelI64", "case kLabelU8", "case kLabelI32", "case kLabelI64"):
        assert case in kernel, case                                     # the switch names all six
    # the header, the model and the kernel's core state the same conversion
    for text in (header, core, tiles.__doc__):
        f = flat(text)
        assert "0 for v < 0, 2^24 - 1 for v > 2^24 - 1, else v" in f and "2^32 + 5 is 2^24 - 1" in f and "(id & 255, (id >> 8) & 255, id >> 16, 255)" in f, text[:60]
        assert "id = R + 256 * G + 256^2 * B" in f and "not the lowest id" in f and "(v, 0, 0, 255)" in f
    h = flat(header)
    for phrase in ("QOIMI_TILE_LABELS_ID24 bit 15, only together with QOIMI_TILE_LABELS", "id | 0xFF000000", "so that a mask can join an id pack",
                   "r << 24 | g << 16 | b << 8 | a wins - the order of the id's bytes from the LOW byte up", "compares bit 15 too",
                   "images with and without the bit mix in one label call", "tests/test_label_id_model.py", "bit 14 stays an unknown flag bit",
                   "QOIMI_TENSOR_HW_ID24 is one plane, as QOIMI_TENSOR_HW is", "r | g << 8 | b << 16", "Alpha is ignored",
                   "It goes with QOIMI_TENSOR_I32 and QOIMI_TENSOR_I64 only", "QOIMI_FILTER_NEAREST / _MODE and QOIMI_WARP_NEAREST / _VOTE2 / _VOTE4",
                   "count one element per pixel", "the last of the format checks; its message names ID24", "4 is not a layout",
                   "Not here (of label sources): a count of saturated elements, a remap table, i16 / u16, ids above 2^24 - 1"):
        assert phrase in h, phrase
    assert "ids above 255 spread over r, g and b" not in h             # the one thing the list lost
    assert "16-bit or signed label sources (a label is a byte of the image" in h and "2 is not a layout" in h


def test_tile_size_with_the_bit():
    lib = api.load_library()
    for lab in (U8, I32, I64):
        for flips in range(4):
            for f in (1, 2, 16, 64):
                for ch_in in (3, 4):
                    for ch in (0, 3, 4):
                        t = (7, 3, 2, 30, 17, f, lab | flips)
                        tw, th = -(-30 // f), -(-17 // f)
                        assert api.tile_size(37, 23, ch_in, t, ch) == tiles.size(37, 23, ch_in, t, ch) == (tw * th * (ch or ch_in), tw, th)
                        assert api.tile_size(37, 23, ch_in, t, ch) == api.tile_size(37, 23, ch_in, t[:6] + (lab & ~tiles.LABELS_ID24 | flips,), ch)   # no size changes
    bad = [tiles.LABELS_ID24, tiles.LABELS_ID24 | 1, tiles.LABELS_ID24 | tiles.LABELS_I32, tiles.LABELS_ID24 | 12288,          # no LABELS
           tiles.LABELS | tiles.LABELS_ID24 | 12288,                                                                           # no dtype
           U8 | tiles.SRC, I64 | tiles.SRC_CHW, I32 | tiles.source_flags(tiles.F16), tiles.LABELS_ID24 | tiles.SRC,            # with a SRC bit
           I32 | 4, I32 | 8, I64 | 1 << 10, I64 | 1 << 14, U8 | 1 << 31, I32 | 1 << 16, 1 << 14, 1 << 16]                      # bits that stay unknown
    for flags in bad:
        tw, th = ctypes.c_uint(77), ctypes.c_uint(78)
        t = api.QoimiTile(0, 0, 0, 4, 4, 1, flags, 0)
        assert lib.qoimi_tile_size(ctypes.byref(api.QoiDesc(4, 4, 4, 0)), ctypes.byref(t), 0, ctypes.byref(tw), ctypes.byref(th)) == 0, flags
        assert (tw.value, th.value) == (77, 78) and tiles.size(4, 4, 4, t, 0) == (0, 0, 0)


def test_tile_rejections_in_order(args):  # noqa: F811
    a = args
    # images: 0 is 4 x 4 (descriptor channels 4), 2 is 5 x 3 (channels 3); 1 is named by no tile; a.p is 8-aligned at least (ctypes)

    def call(po=(0, 1024, 2048), tiles_=None, mode=tiles.NEAREST, pack=a.pack, cap=1024, px=a.p):
        return a.lib.qoimi_encode_tiles(a.ctx, px, (ctypes.c_size_t * 3)(*po), a.descs, 3, 0, tiles_, len(tiles_), mode, 1, pack, cap, a.off, a.len, 0,
                                        a.h_off, a.h_len, a.h_desc, None)

    assert a.p % 8 == 0
    t0 = (0, 1, 1, 2, 2, 1, I32, 0)
    t2 = (2, 0, 0, 5, 3, 1, I64 | 3, 0)
    plain0 = (0, 0, 0, 1, 1, 1, tiles.label_flags(tiles.L_I32), 0)
    cases = [
        # bit 15 without QOIMI_TILE_LABELS joins the check of the dtype bits - behind every check that was there
        ("ID24 without LABELS", lambda: call(tiles_=tl(t0, (2, 0, 0, 5, 3, 1, tiles.LABELS_ID24, 0))), "without QOIMI_TILE_LABELS"),
        ("ID24 and I64 without LABELS", lambda: call(tiles_=tl(t0, (2, 0, 0, 5, 3, 1, tiles.LABELS_ID24 | tiles.LABELS_I64 | 2, 0))), "without QOIMI_TILE_LABELS"),
        ("ID24 without LABELS, averaged at factor 2", lambda: call(tiles_=tl(t0, (2, 0, 0, 5, 3, 2, tiles.LABELS_ID24, 0)), mode=tiles.PLAIN), "without QOIMI_TILE_LABELS"),
        ("an unknown bit comes first", lambda: call(tiles_=tl(t0, (2, 0, 0, 5, 3, 1, tiles.LABELS_ID24 | 4, 0))), "unknown flag bit"),
        ("bit 14 stays unknown", lambda: call(tiles_=tl(t0, (2, 0, 0, 5, 3, 1, I64 | 1 << 14, 0))), "unknown flag bit"),
        ("bit 16 stays unknown", lambda: call(tiles_=tl(t0, (2, 0, 0, 5, 3, 1, I64 | 1 << 16, 0))), "unknown flag bit"),
        ("bit 10 stays unknown", lambda: call(tiles_=tl(t0, (2, 0, 0, 5, 3, 1, I64 | 1 << 10, 0))), "unknown flag bit"),
        ("bit 31 stays unknown", lambda: call(tiles_=tl(t0, (2, 0, 0, 5, 3, 1, U8 | 1 << 31, 0))), "unknown flag bit"),
        ("bits 2 and 3 stay unknown", lambda: call(tiles_=tl(t0, (2, 0, 0, 5, 3, 1, U8 | 12, 0))), "unknown flag bit"),
        ("reserved comes first", lambda: call(tiles_=tl(t0, (2, 0, 0, 5, 3, 1, tiles.LABELS_ID24, 1))), "reserved"),
        ("factor above 16 with QOIMI_TILE_MODE comes first", lambda: call(tiles_=tl(t0, (2, 0, 0, 5, 3, 17, tiles.LABELS_ID24, 0)), mode=tiles.MODE), "factor above 16"),
        ("an id tile votes over at most 16 x 16 too", lambda: call(tiles_=tl(t0, (2, 0, 0, 5, 3, 17, I64, 0)), mode=tiles.MODE), "factor above 16"),
        ("the checks of QOIMI_TILE_SRC come first", lambda: call(tiles_=tl(t0, (2, 0, 0, 5, 3, 1, tiles.LABELS_ID24 | tiles.SRC_CHW, 0))), "without QOIMI_TILE_SRC"),
        # then the label checks as they were
        ("dtype 12288 with the bit", lambda: call(tiles_=tl(t0, (2, 0, 0, 5, 3, 1, tiles.LABELS | tiles.LABELS_ID24 | 12288, 0))), "12288 is not a dtype"),
        ("an id tile with SRC", lambda: call(tiles_=tl(t0, (2, 0, 0, 5, 3, 1, U8 | tiles.SRC, 0))), "together with a QOIMI_TILE_SRC"),
        ("ids are never averaged: PLAIN at factor 2", lambda: call(tiles_=tl(t0, (2, 0, 0, 5, 3, 2, I64, 0)), mode=tiles.PLAIN), "never averaged"),
        ("ALPHA_WEIGHTED at factor 64", lambda: call(tiles_=tl(t0, (2, 0, 0, 5, 3, 64, U8, 0)), mode=tiles.ALPHA_WEIGHTED), "never averaged"),
        # over the call: an id tile is a label tile
        ("a byte tile in an id call", lambda: call(po=(1, 1024, 2048), tiles_=tl(t0, (0, 0, 0, 4, 4, 1, 0, 0), t2)), "a byte call, a tensor call or a label call"),
        # the same image with and without the bit (before the alignment: image 0 at an odd address)
        ("image 0 as ids and as class indices of the same dtype", lambda: call(po=(1, 1024, 2048), tiles_=tl(t0, plain0)), "two different label"),
        ("image 2 without the bit, then with it", lambda: call(tiles_=tl((2, 0, 0, 1, 1, 1, tiles.label_flags(tiles.L_I64), 0), t0, t2)), "two different label"),
        ("image 0 as i32 ids and as u8 ids", lambda: call(tiles_=tl(t0, (0, 0, 0, 1, 1, 1, U8, 0))), "two different label"),
        # the alignment and the extents are a label tile's
        ("i32 ids at an odd offset", lambda: call(po=(1, 1024, 2048), tiles_=tl(t0, t2)), "multiple of the element size"),
        ("i64 ids at offset 4", lambda: call(po=(0, 1024, 2052), tiles_=tl(t0, t2)), "multiple of the element size"),
        ("image end wraps the address space, counted in bytes", lambda: call(po=(0, 1024, 2 ** 64 - a.p - 112), tiles_=tl(t0, t2)), "address space"),
        ("image 2's last element lies in the pack", lambda: call(po=(0, 1024, 4096 - 112), tiles_=tl(t0, t2)), "overlap"),
        ("the pack inside image 2's last element", lambda: call(pack=a.p + 2048 + 119, cap=1, tiles_=tl(t0, t2)), "overlap"),
    ]
    for name, c, cause in cases:
        assert c() == E_ARG, name
        assert cause in api.last_error(), (name, api.last_error())
        assert untouched(a), name


def test_id_and_plain_images_mix_in_one_label_call(args):  # noqa: F811
    """image 0 as ids, image 2 as class indices, every dtype, mode and factor: the label checks pass, and such a call gets as far as the
    context, which this test must not do - so the tile limit stops it, the last check before anything is launched"""
    a = args
    w, h = 19999, 20000
    descs = (api.QoiDesc * 2)(api.QoiDesc(w, h, 3, 0), api.QoiDesc(w, h, 4, 0))
    for lab in (U8, I32, I64):
        for mode, f in ((0, 1), (4, 1), (5, 1), (4, 2), (5, 2), (5, 16)):
            per = tiles.label_tiles(w, h, f, 3, mode)
            n = -(-(2 ** 31 - 1) // per)
            other = lab & ~tiles.LABELS_ID24
            many = (api.QoimiTile * n)(*[api.QoimiTile(j & 1, 0, 0, w, h, f, (other if j & 1 else lab) | (j & 3), 0) for j in range(n)])
            rc = a.lib.qoimi_encode_tiles(a.ctx, a.p, (ctypes.c_size_t * 2)(0, 0), descs, 2, 3, many, n, mode, 1, None, 0, a.off, a.len, 1 << 60, a.h_off, a.h_len, a.h_desc, None)
            assert rc == E_ARG and "tiles of work items" in api.last_error(), (lab, mode, f, api.last_error())
            assert untouched(a)


def model_size(u8_bytes, och, f):
    return tensors.size_hw(u8_bytes, och, f[0]) if f[1] in (tensors.HW, tensors.HW_ID24) else tensors.size(u8_bytes, f[0])


def test_tensor_sizes_with_the_layout():
    good = (0, 1, 1, 2, 2, 5, 3, 0)
    gw = warp.item(0, (1, 1, 2, 2), (5, 3), flags=warp.NEAREST)
    for filt in (tensors.FILTER_NEAREST, tensors.FILTER_MODE, tensors.FILTER_AREA, tensors.FILTER_BILINEAR, tensors.FILTER_BICUBIC, tensors.FILTER_LANCZOS):
        for ch in (3, 4):                                               # one element per pixel, whatever channels says
            assert api.tensor_size(4, 4, 4, good, filt, ch, ID64) == 120 and api.tensor_size(4, 4, 4, good, filt, ch, ID32) == 60, (filt, ch)
    for ch in (3, 4):
        assert api.warp_tensor_size(4, 4, 4, gw, ch, ID64) == 120 and api.warp_tensor_size(4, 4, 3, gw, ch, ID32) == 60
    w, h = 20000, 17000
    for rect in [(0, 0, 1, 1), (3, 2, 16, 32), (0, 0, 16384, 16384), (0, 0, 16385, 1), (0, 0, 0, 1)]:
        for out in [(1, 1), (224, 224), (16384, 16384), (16385, 1), (0, 1)]:
            for ch in (3, 4):
                it = (5,) + rect + out + (3,)
                u8 = nearest.size(w, h, rect, out, 3, ch)
                for f in (ID32, ID64):
                    assert api.tensor_size(w, h, 4, it, tensors.FILTER_NEAREST, ch, f) == model_size(u8, ch, f) == u8 // ch * tensors.INT_ELEM[f[0]], (it, ch, f[:2])
    # the dtypes it does not go with, the formats the integer dtypes reject, and the layouts that stay none
    for td in (tensors.U8, tensors.F16, tensors.BF16, tensors.F32):
        f = (td, tensors.HW_ID24, ONE4, ZERO4)
        assert api.tensor_size(4, 4, 4, good, tensors.FILTER_NEAREST, 4, f) == 0 and api.warp_tensor_size(4, 4, 4, gw, 4, f) == 0 and "ID24" in tensors.wrong(tensors.fmt(*f)), td
    for f in [(tensors.I64, tensors.HW_ID24, (1.0, 1.0, 1.0, 0.5), ZERO4), (tensors.I32, tensors.HW_ID24, ONE4, (-0.0, 0.0, 0.0, 0.0)), (4, tensors.HW_ID24, ONE4, ZERO4),
              (7, tensors.HW_ID24, ONE4, ZERO4)]:
        assert api.tensor_size(4, 4, 4, good, tensors.FILTER_NEAREST, 4, f) == 0 and api.warp_tensor_size(4, 4, 4, gw, 4, f) == 0 and tensors.wrong(tensors.fmt(*f)), f
    for layout in (2, 4, 6, 7, 9):
        f = (tensors.I64, layout, ONE4, ZERO4)
        assert api.tensor_size(4, 4, 4, good, tensors.FILTER_NEAREST, 4, f) == 0 and api.warp_tensor_size(4, 4, 4, gw, 4, f) == 0 and "layout" in tensors.wrong(f), layout


@pytest.fixture()
def targs():
    class A:
        pass
    a = A()
    a.lib = api.load_library()
    a.fake_ctx = (ctypes.c_ubyte * (1 << 16))()                  # never looked at: every rejection comes first
    a.ctx = ctypes.addressof(a.fake_ctx)
    a.buf = (ctypes.c_ubyte * 4096)()
    a.p = ctypes.addressof(a.buf)
    a.out = (ctypes.c_ubyte * 8192)()
    ctypes.memset(a.out, 0x5A, 8192)
    a.o = (ctypes.addressof(a.out) + 15) & ~15                   # a multiple of 16: the offsets are the alignment
    a.so = (ctypes.c_size_t * 2)(0, 1024)
    a.sizes = (ctypes.c_int * 2)(40, 40)
    a.descs = (api.QoiDesc * 2)(api.QoiDesc(4, 4, 4, 0), api.QoiDesc(20000, 17000, 4, 1))
    a.items = [(0, 1, 1, 2, 2, 2, 2, 0), (1, 0, 0, 16384, 1, 5, 1, 1)]                  # 4 and 5 pixels
    a.warps = [warp.item(0, (1, 1, 2, 2), (2, 2), flags=warp.NEAREST), warp.item(1, (0, 0, 130, 1), (5, 1), flags=1)]
    return a


def tensor_untouched(a):
    return bytes(a.out) == b"\x5A" * 8192 and bytes(a.buf) == b"\0" * 4096 and bytes(a.fake_ctx) == b"\0" * (1 << 16)


def fm(f, reserved=(0, 0)):
    t = api.tensor_format(f)
    return api.QoimiTensorFormat(t.dtype, t.layout, t.scale, t.bias, (ctypes.c_uint * 2)(*reserved))


@pytest.mark.parametrize("warped", [False, True])
def test_tensor_rejections_and_their_order(targs, warped):
    a = targs

    def call(ctx=a.ctx, ch=0, items=None, filter=tensors.FILTER_NEAREST, mode=0, f=fm(ID64), oo=(0, 1024)):
        fp = None if f is None else ctypes.byref(f)
        o2 = (ctypes.c_size_t * 2)(*oo)
        if warped:
            arr = (api.QoimiWarp * 2)(*[api.QoimiWarp(*it) for it in (a.warps if items is None else items)])
            return a.lib.qoimi_decode_warped_tensors(ctx, a.p, a.so, a.sizes, a.descs, 2, ch, arr, 2, mode, fp, a.o, o2, 0, None)
        arr = (api.QoimiResize * 2)(*[api.QoimiResize(*it) for it in (a.items if items is None else items)])
        return a.lib.qoimi_decode_tensors(ctx, a.p, a.so, a.sizes, a.descs, 2, ch, arr, 2, filter, mode, fp, a.o, o2, 0, None)

    nan = float("nan")
    ID = tensors.HW_ID24
    # item 0 is 4 pixels: 32 bytes as I64 ids, 16 as I32 ids
    calls = {
        "ID24 with U8": (lambda: call(f=fm((tensors.U8, ID, ONE4, ZERO4))), "ID24"), "ID24 with F16": (lambda: call(f=fm((tensors.F16, ID, ONE4, ZERO4))), "ID24"),
        "ID24 with BF16": (lambda: call(f=fm((tensors.BF16, ID, (0.5,) * 4, (1.0,) * 4))), "ID24"), "ID24 with F32": (lambda: call(f=fm((tensors.F32, ID, ONE4, ZERO4))), "ID24"),
        # the last of the format checks ...
        "order: dtype first": (lambda: call(f=fm((7, ID, (nan,) * 4, ZERO4), (1, 1))), "unknown dtype"), "order: dtype 4": (lambda: call(f=fm((4, ID, ONE4, ZERO4))), "unknown dtype"),
        "order: reserved before ID24": (lambda: call(f=fm((tensors.F32, ID, ONE4, ZERO4), (0, 1))), "reserved"),
        "order: finite before ID24": (lambda: call(f=fm((tensors.F16, ID, (1.0, nan, 1.0, 1.0), ZERO4))), "finite"),
        "order: the U8 rule before ID24": (lambda: call(f=fm((tensors.U8, ID, (2.0, 1.0, 1.0, 1.0), ZERO4))), "QOIMI_TENSOR_U8 takes scale 1 and bias +0 only"),
        "order: the I64 rule holds": (lambda: call(f=fm((tensors.I64, ID, ONE4, (0.0, 0.0, -0.0, 0.0)))), "QOIMI_TENSOR_I64 takes scale 1 and bias +0 only"),
        "order: the I32 rule holds": (lambda: call(f=fm((tensors.I32, ID, (1.0, 1.0, 1.0, 0.5), ZERO4))), "QOIMI_TENSOR_I32 takes scale 1 and bias +0 only"),
        "order: mode before the format": (lambda: call(mode=3, f=fm((tensors.F32, ID, ONE4, ZERO4))), "mode"),
        # ... and in front of everything behind the format
        "order: ID24 before the outputs": (lambda: call(f=fm((tensors.F32, ID, ONE4, ZERO4)), oo=(2, 3)), "ID24"),
        "layout 4 stays unknown": (lambda: call(f=fm((tensors.I64, 4, ONE4, ZERO4))), "unknown layout"), "layout 6 stays unknown": (lambda: call(f=fm((tensors.I64, 6, ONE4, ZERO4))), "unknown layout"),
        "layout 2 stays unknown": (lambda: call(f=fm((tensors.I32, 2, ONE4, ZERO4))), "unknown layout"), "layout 7 stays unknown": (lambda: call(f=fm((tensors.I32, 7, ONE4, ZERO4))), "unknown layout"),
        "layout 9 stays unknown": (lambda: call(f=fm((tensors.I32, 9, ONE4, ZERO4))), "unknown layout"),
        # sizes, overlap and alignment count one element per pixel: 32 bytes, not 128
        "I64 ids overlap by one element": (lambda: call(ch=4, oo=(0, 24)), "overlap"), "I32 ids overlap by one element": (lambda: call(oo=(0, 12), f=fm(ID32)), "overlap"),
        "I64 ids side by side get as far as the alignment": (lambda: call(ch=4, oo=(0, 36)), "multiple of the element size"),
        "I32 ids side by side get as far as the alignment": (lambda: call(ch=3, oo=(0, 18), f=fm(ID32)), "multiple of the element size"),
        "I64 ids at 4 mod 8": (lambda: call(oo=(4, 1024)), "multiple of the element size"), "I32 ids at 2 mod 4": (lambda: call(oo=(0, 1026), f=fm(ID32)), "multiple of the element size"),
        "output end wraps": (lambda: call(oo=(0, 2 ** 64 - a.o - 32)), "address space"),
    }
    if not warped:
        calls.update({"order: the filter before the format": (lambda: call(filter=10, f=fm((tensors.F32, ID, ONE4, ZERO4))), "filter"),
                      "order: ID24 before the items": (lambda: call(f=fm((tensors.F32, ID, ONE4, ZERO4)), items=[a.items[0], (1, 0, 0, 16385, 1, 1, 1, 0)]), "ID24")})
    for name, (c, word) in calls.items():
        assert c() == E_ARG, name
        assert word in api.last_error(), (name, api.last_error())
        assert tensor_untouched(a), name
    # the two formats it goes with get as far as the output ranges, under every filter
    small = None if warped else [a.items[0], (1, 0, 0, 10, 1, 5, 1, 1)]    # (item 1 of a.items is reduced by 3276: the nearest filter alone takes it)
    for f in (ID32, ID64):
        for filt in ((tensors.FILTER_NEAREST, tensors.FILTER_MODE, tensors.FILTER_BILINEAR, tensors.FILTER_AREA) if not warped else (0,)):
            assert call(f=fm(f), filter=filt, items=small, oo=(64, 64)) == E_ARG and "overlap" in api.last_error(), (f[:2], filt)
    assert tensor_untouched(a)
