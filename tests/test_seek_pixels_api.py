"""The API surface of qoimi_seek_index_from_pixels, qoimi_decode_resized_indexed and qoimi_pixel_stats_indexed without a GPU: the header's
prototypes, the ctypes bindings, and every rejection that happens before a context is looked at (the output arrays stay as they were)."""
import ctypes
import os
import re

import pytest

from qoi_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1
NAMES = ("qoimi_seek_index_from_pixels", "qoimi_decode_resized_indexed", "qoimi_pixel_stats_indexed")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(api.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return api.load_library()


def test_header_and_bindings(lib):
    hdr = open(os.path.join(ROOT, "include", "qoi_mi355x.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        assert re.fullmatch(r"qoimi_[a-z_]+", name) and re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert name in api.EXPORTS and hasattr(lib, name) and getattr(lib, name).argtypes is not None
    assert len(lib.qoimi_seek_index_from_pixels.argtypes) == 11
    # the arguments of the plain call followed by interval_rows, points, point_firsts, as qoimi_decode_crops_indexed has them
    tail = lib.qoimi_decode_crops_indexed.argtypes[-3:]
    assert lib.qoimi_decode_resized_indexed.argtypes == lib.qoimi_decode_resized.argtypes + tail
    assert lib.qoimi_pixel_stats_indexed.argtypes == lib.qoimi_pixel_stats.argtypes + tail
    for plain in ("qoimi_decode_resized", "qoimi_pixel_stats"):
        args = lambda name: re.sub(r"\s+", " ", re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\);", code).group(1))
        assert args(plain + "_indexed").startswith(args(plain)) and \
            args(plain + "_indexed")[len(args(plain)):].replace(" ", "") == ",constunsigned*interval_rows,constqoimi_seek_point*points,constsize_t*point_firsts"
    assert "points_from_pixels" in hdr and "TRUSTED" in hdr[hdr.index("qoimi_encode_images_packed: packed_off_out"):hdr.index("int qoimi_seek_index_from_pixels")]
    assert os.path.exists(os.path.join(ROOT, "qoi_amd", "csrc", "qoi_seekpx_core.h"))
    assert '#include "qoi_seekpx_core.h"' in open(os.path.join(ROOT, "qoi_amd", "csrc", "qoi_seek.hip")).read()


def test_from_pixels_rejections_before_a_context_is_looked_at(lib):
    """a context that is not one: every call below must return before it touches it"""
    fake = ctypes.c_void_p(0x10)
    n = 2
    po, so, sz = (ctypes.c_size_t * n)(1, 70001), (ctypes.c_size_t * n)(0, 4096), (ctypes.c_int * n)(100, 100)
    ds, ks = (api.QoiDesc * n)(api.QoiDesc(64, 8, 4, 0), api.QoiDesc(64, 8, 3, 0)), (ctypes.c_uint * n)(2, 2)
    pts = (api.QoimiSeekPoint * 6)()
    ctypes.memset(pts, 0x5A, ctypes.sizeof(pts))
    before = bytes(pts)
    px, dev = ctypes.c_void_p(0x3000000), ctypes.c_void_p(0x1000000)

    def build(ctx=fake, px_=px, po_=po, streams=dev, so_=so, sz_=sz, ds_=ds, n_=n, ks_=ks, out=pts):
        return lib.qoimi_seek_index_from_pixels(ctx, px_, po_, streams, so_, sz_, ds_, n_, ks_, out, None)

    for kw in ("ctx", "px_", "po_", "streams", "so_", "sz_", "ds_", "ks_", "out"):
        assert build(**{kw: None}) == E_ARG, kw
    assert build(n_=0) == E_ARG and build(n_=-1) == E_ARG
    assert build(sz_=(ctypes.c_int * n)(100, 21)) == E_ARG and "22" in api.last_error()
    assert build(ds_=(api.QoiDesc * n)(ds[0], api.QoiDesc(64, 8, 3, 2))) == E_ARG and build(ds_=(api.QoiDesc * n)(api.QoiDesc(64, 8, 5, 0), ds[1])) == E_ARG
    assert build(ks_=(ctypes.c_uint * n)(2, 1)) == E_ARG and "128" in api.last_error() and build(ks_=(ctypes.c_uint * n)(0, 2)) == E_ARG
    # an image whose last byte's address does not fit in a pointer: the 64 * 8 * 3 bytes of image 1 end one byte behind address 2^64 - 1 ...
    top = 2 ** 64 - 0x3000000
    assert build(po_=(ctypes.c_size_t * n)(1, top - 64 * 8 * 3 + 1)) == E_ARG and "pointer" in api.last_error()
    assert build(po_=(ctypes.c_size_t * n)(top, 0)) == E_ARG and "pointer" in api.last_error()
    # ... and image 0 with its last byte AT address 2^64 - 1 is fine: the call goes on to what is wrong with image 1
    assert build(po_=(ctypes.c_size_t * n)(top - 64 * 8 * 4, 0), ks_=(ctypes.c_uint * n)(2, 1)) == E_ARG and "image 1" in api.last_error() and "128" in api.last_error()
    # 2^31 - 1 or more tiles of 1024 pixels in the call: 11 000 images of 19999 x 20000 with one point each, 195 303 tiles per point
    m = 11000
    assert api.seek_points(19999, 20000, 3, 10000) == 1 and m * -(-19999 * 10000 // 1024) >= 2 ** 31 - 1
    zeros = (ctypes.c_size_t * m)()
    assert lib.qoimi_seek_index_from_pixels(fake, px, zeros, dev, zeros, (ctypes.c_int * m)(*[100] * m), (api.QoiDesc * m)(*[api.QoiDesc(19999, 20000, 3, 0)] * m), m,
                                            (ctypes.c_uint * m)(*[10000] * m), pts, None) == E_ARG and "tiles" in api.last_error()
    assert bytes(pts) == before


def test_indexed_rejections_before_a_context_is_looked_at(lib):
    fake = ctypes.c_void_p(0x10)
    n = 2
    so, sz = (ctypes.c_size_t * n)(0, 4096), (ctypes.c_int * n)(100, 100)
    ds, ks, pf = (api.QoiDesc * n)(api.QoiDesc(64, 8, 4, 0), api.QoiDesc(64, 8, 3, 0)), (ctypes.c_uint * n)(2, 2), (ctypes.c_size_t * n)(0, 3)
    pts = (api.QoimiSeekPoint * 6)()
    for p in pts:
        p.byte_off = 14
    bad = (api.QoimiSeekPoint * 6)()
    ctypes.memmove(bad, pts, ctypes.sizeof(pts))
    bad[0].skip = 62
    hostile = (api.QoimiSeekPoint * 6)()
    ctypes.memmove(hostile, pts, ctypes.sizeof(pts))
    hostile[0].prev = 0x7F7F7F7F
    for k in range(64):
        hostile[0].table[k] = 0x01000000 + k
    dev, out, o1 = ctypes.c_void_p(0x1000000), ctypes.c_void_p(0x2000000), (ctypes.c_size_t * 1)(0)

    items = (api.QoimiResize * 1)(api.QoimiResize(0, 0, 3, 8, 2, 4, 4, 0))     # its band starts at row 2: point 0

    def resized(ctx=fake, streams=dev, so_=so, sz_=sz, ds_=ds, n_=n, ch=4, it=items, ni=1, mode=0, out_=out, oo_=o1, ks_=ks, pts_=pts, pf_=pf):
        return lib.qoimi_decode_resized_indexed(ctx, streams, so_, sz_, ds_, n_, ch, it, ni, mode, out_, oo_, 0, None, ks_, pts_, pf_)

    for kw in ("ctx", "streams", "so_", "sz_", "ds_", "it", "out_", "oo_", "ks_", "pts_", "pf_"):
        assert resized(**{kw: None}) == E_ARG, kw
    assert resized(n_=0) == E_ARG and resized(ni=0) == E_ARG and resized(ch=5) == E_ARG and resized(mode=2) == E_ARG
    assert resized(it=(api.QoimiResize * 1)(api.QoimiResize(0, 0, 7, 8, 2, 4, 4, 0))) == E_ARG and "leaves" in api.last_error()
    assert resized(it=(api.QoimiResize * 1)(api.QoimiResize(0, 0, 0, 8, 8, 4, 0, 0))) == E_ARG and "zero" in api.last_error()
    assert resized(it=(api.QoimiResize * 1)(api.QoimiResize(0, 0, 0, 64, 2, 0x80000000, 0x80000000, 0)), ch=4) == E_ARG and "address space" in api.last_error()
    assert resized(ks_=(ctypes.c_uint * n)(1, 0)) == E_ARG and "128" in api.last_error()
    assert resized(pts_=bad) == E_ARG and "skip" in api.last_error()
    assert resized(pts_=hostile) == E_ARG and "64 loads" in api.last_error()
    assert resized(sz_=(ctypes.c_int * n)(21, 0)) == E_ARG
    # an item in the first interval uses point 0 as e2 only; image 1 is not referenced: its interval is not looked at
    assert resized(it=(api.QoimiResize * 1)(api.QoimiResize(0, 0, 0, 8, 2, 4, 4, 0)), pts_=bad) == E_ARG and "skip" in api.last_error()

    regions = (api.QoimiCrop * 1)(api.QoimiCrop(0, 0, 3, 8, 2, 0))
    stats = (api.QoimiPixelStat * 1)()
    ctypes.memset(stats, 0x5A, ctypes.sizeof(stats))
    before = bytes(stats)

    def pstats(ctx=fake, streams=dev, so_=so, sz_=sz, ds_=ds, n_=n, rs=regions, nr=1, out_=stats, ks_=ks, pts_=pts, pf_=pf):
        return lib.qoimi_pixel_stats_indexed(ctx, streams, so_, sz_, ds_, n_, rs, nr, out_, None, 0, None, ks_, pts_, pf_)

    for kw in ("ctx", "streams", "so_", "sz_", "ds_", "rs", "out_", "ks_", "pts_", "pf_"):
        assert pstats(**{kw: None}) == E_ARG, kw
    assert pstats(n_=0) == E_ARG and pstats(nr=0) == E_ARG
    assert pstats(rs=(api.QoimiCrop * 1)(api.QoimiCrop(0, 0, 7, 8, 2, 0))) == E_ARG and "leaves" in api.last_error()
    assert pstats(rs=(api.QoimiCrop * 1)(api.QoimiCrop(2, 0, 3, 8, 2, 0))) == E_ARG and "no image" in api.last_error()
    assert pstats(rs=(api.QoimiCrop * 1)(api.QoimiCrop(0, 0, 3, 8, 2, 4))) == E_ARG and "flag" in api.last_error()
    assert pstats(ks_=(ctypes.c_uint * n)(1, 0)) == E_ARG and "128" in api.last_error()
    assert pstats(pts_=bad) == E_ARG and "skip" in api.last_error()
    assert pstats(pts_=hostile) == E_ARG and "64 loads" in api.last_error()
    assert pstats(sz_=(ctypes.c_int * n)(21, 0)) == E_ARG
    assert bytes(stats) == before


def test_python_wrappers_check_their_lists():
    class Dummy(api.Context):
        def __init__(self):                                                 # no device: the checks below come before the library is called
            pass

        def __del__(self):
            pass

    c = Dummy()
    d = [api.QoiDesc(64, 8, 4, 0)]
    with pytest.raises(api.QoiError):
        c.seek_index_from_pixels(0, [0, 1], 0, [0], [100], d, 2)
    with pytest.raises(api.QoiError):
        c.seek_index_from_pixels(0, [0], 0, [0], [100], d, 1)               # 1 * 64 < 128
    with pytest.raises(api.QoiError):
        c.decode_resized_indexed(0, [0], [100], d, 4, [(0, 0, 0, 8, 2, 4, 4, 0)], 0, 0, [0, 1], 2, None, [0])
    with pytest.raises(api.QoiError):
        c.pixel_stats_indexed(0, [0], [100], d, [(0, 0, 0, 8, 2, 0)], [2, 3], None, [0])
