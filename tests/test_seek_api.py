"""The API surface of the row seek index, without a GPU: the header's prototypes, the layouts of its three structures and the ctypes bindings;
qoimi_seek_points and qoimi_band_plan - host arithmetic - against qoi_amd/seekindex.py; every rejection that happens before a context is
looked at."""
import ctypes
import os
import re

import numpy as np
import pytest

from qoi_amd import api
from qoi_amd import seekindex as si
from model_cases import END, header, index_image, runs_image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1
NAMES = ("qoimi_seek_points", "qoimi_build_seek_index", "qoimi_band_plan", "qoimi_make_band_streams", "qoimi_decode_crops_indexed", "qoimi_seek_stats")


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
        assert re.search(r"\b(int|void)\s+" + name + r"\s*\(", code), name
        assert name in api.EXPORTS and hasattr(lib, name) and getattr(lib, name).argtypes is not None
    assert re.search(r"typedef struct \{ unsigned byte_off, skip, prev, reserved; unsigned table\[64\]; \} qoimi_seek_point;", code)
    assert re.search(r"typedef struct \{ unsigned image, first_row, rows, reserved; \} qoimi_band;", code)
    assert re.search(r"typedef struct \{ unsigned long long size; qoi_desc desc; unsigned pad_rows; \} qoimi_band_info;", code)
    assert len(lib.qoimi_build_seek_index.argtypes) == 10 and len(lib.qoimi_make_band_streams.argtypes) == 15
    assert len(lib.qoimi_decode_crops_indexed.argtypes) == len(lib.qoimi_decode_crops.argtypes) + 3 and len(lib.qoimi_band_plan.argtypes) == 6
    assert "seekindex.py" in hdr and "qoimi_decode_crops_indexed" in open(os.path.join(ROOT, "qoi_amd", "csrc", "qoi_host_seek.hip")).read()
    for f in ("qoi_seek.hip", "qoi_seek_core.h"):
        assert os.path.exists(os.path.join(ROOT, "qoi_amd", "csrc", f))


def test_struct_layouts():
    P, B, I = api.QoimiSeekPoint, api.QoimiBand, api.QoimiBandInfo
    assert ctypes.sizeof(P) == 272 == si.POINT_DTYPE.itemsize and [getattr(P, f).offset for f, _ in P._fields_] == [0, 4, 8, 12, 16]
    assert [si.POINT_DTYPE.fields[f][1] for f in ("byte_off", "skip", "prev", "reserved", "table")] == [0, 4, 8, 12, 16]
    assert ctypes.sizeof(B) == 16 and [getattr(B, f).offset for f, _ in B._fields_] == [0, 4, 8, 12]
    assert ctypes.sizeof(I) == 24 and [getattr(I, f).offset for f, _ in I._fields_] == [0, 8, 20]


def test_seek_points(lib):
    for w, h, K in [(1, 128, 128), (1, 129, 128), (1, 389, 128), (64, 13, 2), (64, 13, 1), (129, 8, 1), (16384, 16384, 256), (5, 100, 25), (5, 100, 26),
                    (7, 3, 0), (128, 1, 1), (128, 2, 1), (127, 9, 1), (19999, 20000, 1), (1, 1, 2 ** 32 - 1)]:
        assert api.seek_points(w, h, 4, K) == si.n_points(w, h, K), (w, h, K)
    assert api.seek_points(16384, 16384, 4, 256) == 63
    assert api.seek_points(0, 9, 4, 200) == -1 and api.seek_points(20000, 20000, 4, 1) == -1 and api.seek_points(64, 64, 5, 2) == -1
    assert lib.qoimi_seek_points(None, 4) == -1


def test_band_plan_against_the_model(lib, port):
    checked = 0
    for w, h, ch, make, K in [(1, 400, 4, runs_image, 128), (61, 20, 3, index_image, 3), (64, 13, 4, index_image, 2), (129, 9, 3, runs_image, 1), (333, 11, 4, runs_image, 2)]:
        s = port.encode(make(w, h, ch, w + 1), w, h, ch)
        for stream in (s, s[:len(s) // 2], s[:22], header(w, h, ch) + b"\xfd" * (w * h // 30 + 3) + END):
            full4, _ = port.decode(stream, 4)
            pts = si.points(stream, w, h, K, full4)
            desc = api.QoiDesc(w, h, ch, 1)
            for first in [0] + [(k + 1) * K for k in range(len(pts))]:
                for rows in sorted({1, min(K, h - first), h - first, min(K + 1, h - first)}):
                    want = si.band_info(len(stream), w, h, ch, 1, K, pts, first, rows)
                    got = api.band_plan(desc, len(stream), K, pts, first, rows)
                    assert got is not None and (got.size, got.pad_rows, (got.desc.width, got.desc.height, got.desc.channels, got.desc.colorspace)) == \
                        (want["size"], want["pad_rows"], want["desc"]), (w, K, first, rows)
                    assert got.size == len(si.band_stream(stream, w, h, ch, 1, K, pts, first, rows)[0])
                    checked += 1
    assert checked > 300


def test_band_plan_rejections(lib, port):
    w, h, K = 64, 13, 2
    s = port.encode(index_image(w, h, 4, 1), w, h, 4)
    full4, _ = port.decode(s, 4)
    pts = si.points(s, w, h, K, full4)
    d = api.QoiDesc(w, h, 4, 0)
    assert api.band_plan(d, len(s), K, pts, 4, 2) is not None
    for desc, size, k, first, rows in [(api.QoiDesc(w, h, 2, 0), len(s), K, 4, 2), (api.QoiDesc(0, h, 4, 0), len(s), K, 4, 2), (d, 21, K, 4, 2), (d, len(s), 1, 4, 2),
                                       (d, len(s), 0, 4, 2), (d, len(s), K, 3, 2), (d, len(s), K, 4, 0), (d, len(s), K, 4, 10), (d, len(s), K, 14, 1), (d, len(s), K, 2 ** 32 - 2, 4)]:
        assert api.band_plan(desc, size, k, pts, first, rows) is None, (size, k, first, rows)
        assert api.last_error().startswith("band: ")
    for field, value, first, rows in [("byte_off", 13, 4, 2), ("byte_off", len(s) - 7, 4, 2), ("skip", 62, 4, 2), ("byte_off", 2 ** 32 - 1, 4, 2)]:
        bad = pts.copy()
        bad[1][field] = value                                            # the point at row 4
        assert api.band_plan(d, len(s), K, bad, first, rows) is None
        assert api.band_plan(d, len(s), K, bad, 8, 2) is not None            # a band that does not use it
    bad = pts.copy()
    bad[2]["byte_off"] = 14                                              # e2 of the band (4, 2): far in front of e
    assert int(pts[1]["byte_off"]) > 14 + 13 and api.band_plan(d, len(s), K, bad, 4, 2) is None and "ascend" in api.last_error()
    # a hostile index: 64 non-zero table words that all differ from prev would be 65 loads, a head of 339 bytes - no point of a stream
    bad = pts.copy()
    bad[1]["table"] = np.arange(64, dtype=np.uint32) + 0x01000000
    bad[1]["prev"] = 0x7F7F7F7F
    assert api.band_plan(d, len(s), K, bad, 4, 2) is None and "64 loads" in api.last_error()
    with pytest.raises(ValueError):
        si.band_info(len(s), w, h, 4, 0, K, bad, 4, 2)
    assert api.band_plan(d, len(s), K, bad, 2, 2) is not None and api.band_plan(d, len(s), K, bad, 8, 2) is not None   # as e2, and not at all
    bad[1]["table"][9] = 0x7F7F7F7F                                      # prev in a slot: 64 loads, the largest head there is
    got = api.band_plan(d, len(s), K, bad, 4, 2)
    assert got is not None and got.pad_rows == 1 and got.size == si.band_info(len(s), w, h, 4, 0, K, bad, 4, 2)["size"] and \
        got.size == 14 + 5 * 64 + 0 + (min(int(pts[2]["byte_off"]) + 13, len(s)) - int(pts[1]["byte_off"]))
    out, band = api.QoimiBandInfo(), api.QoimiBand(0, 4, 2, 0)
    arr, _ = api._point_array(pts)
    assert lib.qoimi_band_plan(None, len(s), K, arr, ctypes.byref(band), ctypes.byref(out)) == E_ARG
    assert lib.qoimi_band_plan(ctypes.byref(d), len(s), K, arr, None, ctypes.byref(out)) == E_ARG
    assert lib.qoimi_band_plan(ctypes.byref(d), len(s), K, arr, ctypes.byref(band), None) == E_ARG
    assert lib.qoimi_band_plan(ctypes.byref(d), len(s), K, None, ctypes.byref(band), ctypes.byref(out)) == E_ARG
    assert lib.qoimi_band_plan(ctypes.byref(api.QoiDesc(w, 2, 4, 0)), len(s), K, None, ctypes.byref(api.QoimiBand(0, 0, 2, 0)), ctypes.byref(out)) == 0 and out.pad_rows == 0
    # a band stream of 2^31 - 1 bytes or more
    big = api.QoiDesc(128, 4, 4, 0)
    assert lib.qoimi_band_plan(ctypes.byref(big), 2 ** 31 - 1, 4, None, ctypes.byref(api.QoimiBand(0, 0, 4, 0)), ctypes.byref(out)) == E_ARG
    assert lib.qoimi_band_plan(ctypes.byref(big), 2 ** 31 - 2, 4, None, ctypes.byref(api.QoimiBand(0, 0, 4, 0)), ctypes.byref(out)) == 0 and out.size == 2 ** 31 - 2


def test_rejections_before_a_context_is_looked_at(lib):
    """a context that is not one: every call below must return before it touches it"""
    fake = ctypes.c_void_p(0x10)
    n = 2
    so, sz = (ctypes.c_size_t * n)(0, 4096), (ctypes.c_int * n)(100, 100)
    ds, ks, pf = (api.QoiDesc * n)(api.QoiDesc(64, 8, 4, 0), api.QoiDesc(64, 8, 3, 0)), (ctypes.c_uint * n)(2, 2), (ctypes.c_size_t * n)(0, 3)
    pts = (api.QoimiSeekPoint * 6)()
    for p in pts:
        p.byte_off = 14
    before = bytes(pts)
    dev = ctypes.c_void_p(0x1000000)

    def build(ctx=fake, streams=dev, so_=so, sz_=sz, ds_=ds, n_=n, ks_=ks, out=pts):
        return lib.qoimi_build_seek_index(ctx, streams, so_, sz_, ds_, n_, ks_, out, 0, None)

    assert build(ctx=None) == E_ARG and build(streams=None) == E_ARG and build(so_=None) == E_ARG and build(sz_=None) == E_ARG
    assert build(ds_=None) == E_ARG and build(ks_=None) == E_ARG and build(out=None) == E_ARG and build(n_=0) == E_ARG and build(n_=-1) == E_ARG
    assert build(sz_=(ctypes.c_int * n)(100, 21)) == E_ARG and build(ds_=(api.QoiDesc * n)(ds[0], api.QoiDesc(64, 8, 3, 2))) == E_ARG
    assert build(ks_=(ctypes.c_uint * n)(2, 1)) == E_ARG and build(ks_=(ctypes.c_uint * n)(0, 2)) == E_ARG
    assert bytes(pts) == before

    bands = (api.QoimiBand * 2)(api.QoimiBand(0, 2, 2, 0), api.QoimiBand(1, 0, 8, 0))
    oo = (ctypes.c_size_t * 2)(0, 4096)
    out = ctypes.c_void_p(0x2000000)

    def make(ctx=fake, streams=dev, so_=so, sz_=sz, ds_=ds, n_=n, ks_=ks, pts_=pts, pf_=pf, bands_=bands, nb=2, out_=out, oo_=oo):
        return lib.qoimi_make_band_streams(ctx, streams, so_, sz_, ds_, n_, ks_, pts_, pf_, bands_, nb, out_, oo_, None, None)

    for kw in ("ctx", "streams", "so_", "sz_", "ds_", "ks_", "pts_", "pf_", "bands_", "out_", "oo_"):
        assert make(**{kw: None}) == E_ARG, kw
    assert make(n_=0) == E_ARG and make(nb=0) == E_ARG
    info = api.band_plan(ds[0], 100, 2, pts, 2, 2)
    assert info is not None and info.size == 14 + 5 + 2 + 13                 # header, prev, a run of 63, 13 bytes of tail
    assert make(bands_=(api.QoimiBand * 2)(api.QoimiBand(2, 0, 1, 0), bands[1])) == E_ARG and "no image" in api.last_error()
    assert make(bands_=(api.QoimiBand * 2)(api.QoimiBand(0, 3, 1, 0), bands[1])) == E_ARG and make(bands_=(api.QoimiBand * 2)(api.QoimiBand(0, 2, 0, 0), bands[1])) == E_ARG
    assert make(bands_=(api.QoimiBand * 2)(api.QoimiBand(0, 2, 7, 0), bands[1])) == E_ARG and "leaves" in api.last_error()
    assert make(sz_=(ctypes.c_int * n)(21, 100)) == E_ARG and make(ks_=(ctypes.c_uint * n)(1, 2)) == E_ARG
    assert make(oo_=(ctypes.c_size_t * 2)(0, 33)) == E_ARG and "overlap" in api.last_error()
    assert make(out_=dev, oo_=(ctypes.c_size_t * 2)(8192, 4096 + 99)) == E_ARG and "overlap" in api.last_error()       # an output on a source stream
    bad = (api.QoimiSeekPoint * 6)()
    ctypes.memmove(bad, pts, ctypes.sizeof(pts))
    bad[0].skip = 62
    assert make(pts_=bad) == E_ARG and "skip" in api.last_error()
    hostile = (api.QoimiSeekPoint * 6)()
    ctypes.memmove(hostile, pts, ctypes.sizeof(pts))
    hostile[0].prev = 0x7F7F7F7F
    for k in range(64):
        hostile[0].table[k] = 0x01000000 + k
    assert make(pts_=hostile) == E_ARG and "64 loads" in api.last_error()

    crops_ = (api.QoimiCrop * 1)(api.QoimiCrop(0, 0, 3, 8, 2, 0))          # its band starts at row 2: point 0
    o1 = (ctypes.c_size_t * 1)(0)

    def indexed(ctx=fake, streams=dev, so_=so, sz_=sz, ds_=ds, n_=n, ch=4, cs=crops_, nc=1, out_=out, oo_=o1, ks_=ks, pts_=pts, pf_=pf):
        return lib.qoimi_decode_crops_indexed(ctx, streams, so_, sz_, ds_, n_, ch, cs, nc, out_, oo_, 0, None, ks_, pts_, pf_)

    for kw in ("ctx", "streams", "so_", "sz_", "ds_", "cs", "out_", "oo_", "ks_", "pts_", "pf_"):
        assert indexed(**{kw: None}) == E_ARG, kw
    assert indexed(n_=0) == E_ARG and indexed(nc=0) == E_ARG and indexed(ch=5) == E_ARG
    assert indexed(cs=(api.QoimiCrop * 1)(api.QoimiCrop(0, 0, 7, 8, 2, 0))) == E_ARG and "leaves" in api.last_error()
    assert indexed(ks_=(ctypes.c_uint * n)(1, 0)) == E_ARG and "128" in api.last_error()
    assert indexed(pts_=bad) == E_ARG and "skip" in api.last_error()
    assert indexed(pts_=hostile) == E_ARG and "64 loads" in api.last_error()
    assert indexed(sz_=(ctypes.c_int * n)(21, 0)) == E_ARG
    z = (ctypes.c_longlong * 4)(9, 9, 9, 9)
    lib.qoimi_seek_stats(None, z)
    assert list(z) == [0, 0, 0, 0]
