"""QOIMI_TILE_NEAREST / QOIMI_TILE_MODE in every layer, what can be checked without a GPU: the values in the header, the model and the
host; the header's statement of the definition; the kernel in the built library; which values of `mode` qoimi_encode_tiles takes and
which it keeps rejecting, the factor limit of the vote and the order of the rejections - all of them are reported before the context or the
device is looked at, so a block of zeroed host memory stands in for a context here and host arrays for device buffers (an accepted mode is
shown by the LATER rejection the call then reaches); qoimi_decode_thumbnails keeps rejecting both values.  (What the library does behind
the rejections needs a device: tests/test_gpu_tile_labels.py.)"""
import ctypes
import os
import re

from qoi_amd import api, tiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_the_values_in_every_layer_and_the_headers_statement():
    header = read("include", "qoi_mi355x.h")
    assert re.search(r"enum \{ QOIMI_TILE_NEAREST = 4, QOIMI_TILE_MODE = 5 \};\s*/\* 2 and 3 are not modes \*/", header)
    assert (tiles.NEAREST, tiles.MODE, tiles.MODE_MAX_FACTOR) == (4, 5, 16)
    for text in ("qoi_amd/tiles.py: tile", "a 3-channel source has alpha 255, and that alpha takes part", "columns [X*f, min((X+1)*f, cw))", "rows [Y*f, min((Y+1)*f, ch))",
                 "column X*f + nx/2, row Y*f + ny/2", "the output pixel is the centre pixel, byte for byte", "qoi_amd/mode.py: vote", "whole pixels vote, all four bytes",
                 "the centre pixel wins if it is one of them", "r << 24 | g << 16 |", "A tile with factor > 16 is QOIMI_E_ARG", "behind the reserved != 0 check",
                 "drops alpha AFTER the vote", "qoimi_tile_size has no mode argument", "factor == 1 is the rectangle itself", "a constant block gives the constant",
                 "QOIMI_FILTER_MODE (u8, HWC)", "its nearest sample is Z*f + f/2", "levels 5 and 6 (f = 32, 64) need QOIMI_TILE_NEAREST", "counts its launches in [1]",
                 "a vote over blocks above 16 x 16", "QOIMI_TILE_NEAREST / QOIMI_TILE_MODE in qoimi_decode_thumbnails", "a factor above 16 with QOIMI_TILE_MODE"):
        assert text in header, text
    assert "other filters, row-pitched sources" not in header          # the gap the header used to name
    host = read("qoi_amd", "csrc", "qoi_host_pack.hip")
    assert "QOIMI_TILE_NEAREST == 4 && QOIMI_TILE_MODE == 5" in host and "launch_tile_select" in host and "tile_select_tiles" in host and "tile_select_cfg" in host
    assert "launch_tile_select" in read("qoi_amd", "csrc", "qoi_kernels.h")
    kernel = read("qoi_amd", "csrc", "qoi_tile.hip")
    assert "walk_tiles" in kernel and "__shared__" not in kernel and "__syncthreads" not in kernel and "atomic" not in kernel.replace("no atomics", "")
    for name in ("mode_meet", "mode_best", "mode_pick", "tile_vote_hold", "tile_centre_pixel", "tile_copy_item"):
        assert name in kernel, name
    core = read("qoi_amd", "csrc", "qoi_tile_core.h")
    assert "kTileModeMaxFactor = kModeMaxRatio" in core and "sizeof(TileEntry) == 56" in core and "mode_split(f, f, 1u, 1u, lg, c)" in core
    doc = api.Context.encode_tiles.__doc__
    assert "tiles.NEAREST" in doc and "tiles.MODE" in doc


def test_the_kernel_is_built_once_without_scratch_agprs_and_lds():
    from tools import kernel_resources as KR
    ks = KR.kernels(os.path.join(ROOT, "qoi_amd", "lib", "libqoi_mi355x.so"))
    hits = [k for k in ks if "tile_select" in k]
    assert len(hits) == 1, hits
    k = ks[hits[0]]
    assert k["scratch"] == 0 and k["vgpr_spills"] == 0 and k["agpr"] == 0 and k["lds"] == 0, k
    assert "tile_select uses no LDS" in read("DESIGN.md")
    assert len([k for k in ks if "tile_gather" in k]) == 1
    lib = api.load_library()
    assert not any("tile" in lib.qoimi_kernel_name(i).decode() for i in range(64))      # no timer entry, as tile_gather has none


class Args:
    def __init__(self):
        self.lib = api.load_library()
        self.fake_ctx = (ctypes.c_ubyte * (1 << 20))()              # never looked at: every rejection comes first
        self.ctx = ctypes.addressof(self.fake_ctx)
        self.buf = (ctypes.c_ubyte * 8192)()                        # stands in for d_pixels, the device tables and the pack
        ctypes.memset(self.buf, 0x5A, 8192)
        self.p = ctypes.addressof(self.buf)
        self.pack, self.off, self.len = self.p + 4096, self.p + 6144, self.p + 7168
        self.po = (ctypes.c_size_t * 2)(1, 2051)
        self.descs = (api.QoiDesc * 2)(api.QoiDesc(4, 4, 4, 0), api.QoiDesc(5, 3, 3, 1))
        self.h_off = (ctypes.c_ulonglong * 3)(7, 7, 7)
        self.h_len = (ctypes.c_int * 2)(7, 7)
        self.h_desc = (api.QoiDesc * 2)(api.QoiDesc(7, 7, 7, 7), api.QoiDesc(7, 7, 7, 7))

    def untouched(self):
        return (bytes(self.buf) == b"\x5A" * 8192 and bytes(self.fake_ctx[:4096]) == b"\0" * 4096 and list(self.h_off) == [7] * 3 and list(self.h_len) == [7] * 2
                and all((d.width, d.height, d.channels, d.colorspace) == (7, 7, 7, 7) for d in self.h_desc))

    def call(self, mode, t0=(0, 1, 1, 2, 2, 1, 0, 0), t1=(1, 0, 0, 5, 3, 2, 3, 0), ctx=0, po=None, ch=0):
        """a call that is fine but for what the arguments say, and whose first image overlaps the pack unless po is given - so that a call
        nothing else is wrong with ends in "overlap", before the context is looked at"""
        tl = (api.QoimiTile * 2)(api.QoimiTile(*t0), api.QoimiTile(*t1))
        po = (ctypes.c_size_t * 2)(4096 - 63, 2051) if po is None else po
        rc = self.lib.qoimi_encode_tiles(self.ctx if ctx == 0 else ctx, self.p, po, self.descs, 2, ch, tl, 2, mode, 1, self.pack, 1024, self.off, self.len, 0,
                                         self.h_off, self.h_len, self.h_desc, None)
        assert rc == E_ARG and self.untouched(), (mode, t0, t1, api.last_error())
        return api.last_error()


def test_the_modes_accepted_and_rejected():
    a = Args()
    for mode in (tiles.PLAIN, tiles.ALPHA_WEIGHTED, tiles.NEAREST, tiles.MODE):
        err = a.call(mode)
        assert "overlap" in err and "mode" not in err, (mode, err)                  # accepted: the call got as far as the images' addresses
    for mode in (2, 3, 6, -1, 4 + 256, 5 + 65536, 2 ** 31 - 1, -4):
        err = a.call(mode)
        assert "mode" in err and "overlap" not in err, (mode, err)
        assert "QOIMI_TILE_NEAREST" in err and "QOIMI_TILE_MODE" in err and "QOIMI_THUMB_PLAIN" in err


def test_the_factor_limit_of_the_vote():
    a = Args()
    for f in (17, 33, 64):
        err = a.call(tiles.MODE, t1=(0, 0, 0, 4, 4, f, 0, 0))
        assert err.startswith("tile 1: ") and "factor above 16" in err and "QOIMI_TILE_MODE" in err and "QOIMI_TILE_NEAREST" in err, (f, err)
        err = a.call(tiles.MODE, t0=(1, 0, 0, 5, 3, f, 3, 0))
        assert err.startswith("tile 0: ") and "factor above 16" in err, (f, err)
        for mode in (tiles.NEAREST, tiles.PLAIN, tiles.ALPHA_WEIGHTED):
            assert "overlap" in a.call(mode, t1=(0, 0, 0, 4, 4, f, 0, 0)), (f, mode)        # no such limit: accepted
    for f in (1, 2, 16):
        assert "overlap" in a.call(tiles.MODE, t1=(0, 0, 0, 4, 4, f, 0, 0)), f
    assert "factor outside 1..64" in a.call(tiles.MODE, t1=(0, 0, 0, 4, 4, 65, 0, 0)) and "factor outside 1..64" in a.call(tiles.NEAREST, t1=(0, 0, 0, 4, 4, 0, 0, 0))


def test_the_order_of_the_rejections():
    a = Args()
    big = (0, 0, 0, 4, 4, 17, 0, 0)
    # the call's own arguments come first: NULL, align (not varied here), channels, mode - then the tiles, one by one
    assert "NULL" in a.call(tiles.MODE, t1=big, ctx=None)
    assert "channels" in a.call(6, t1=big, ch=5)
    assert "mode" in a.call(6, t1=big)
    # within a tile: image, descriptor, zero, leaves, the factor's range, flag, reserved - and only then the vote's limit
    assert "no image" in a.call(tiles.MODE, t1=(2, 0, 0, 4, 4, 17, 4, 1))
    assert "zero" in a.call(tiles.MODE, t1=(0, 0, 0, 0, 4, 17, 4, 1))
    assert "leaves" in a.call(tiles.MODE, t1=(0, 1, 0, 4, 4, 17, 4, 1))
    assert "flag" in a.call(tiles.MODE, t1=(0, 0, 0, 4, 4, 17, 4, 1))
    assert "reserved" in a.call(tiles.MODE, t1=(0, 0, 0, 4, 4, 17, 0, 1))
    assert "factor above 16" in a.call(tiles.MODE, t1=big)
    # tile by tile: the first wrong tile is the one reported
    assert a.call(tiles.MODE, t0=(0, 0, 0, 4, 4, 64, 0, 0), t1=(0, 0, 0, 0, 4, 1, 0, 0)).startswith("tile 0: factor above 16")
    assert a.call(tiles.MODE, t0=(0, 0, 0, 4, 4, 16, 0, 1), t1=big).startswith("tile 0: reserved")
    # the tiles before the images' addresses and the overlap
    assert "factor above 16" in a.call(tiles.MODE, t1=big, po=(ctypes.c_size_t * 2)(1, 2 ** 64 - 8))
    assert "address space" in a.call(tiles.MODE, po=(ctypes.c_size_t * 2)(1, 2 ** 64 - 8))
    assert "address space" in a.call(tiles.NEAREST, t0=(0, 0, 0, 4, 4, 64, 0, 0), po=(ctypes.c_size_t * 2)(1, 2 ** 64 - 8))


def test_the_pyramid_tools_arguments(tmp_path):
    """everything that ends before the device is looked at"""
    from tools import qoipyramid_mi355x as tool
    lines = []
    f, o = str(tmp_path / "x.qoi"), ["-o", str(tmp_path / "o")]
    for levels in ("6", "7"):
        assert tool.main([f, "--tile", "64", "--levels", levels, "--filter", "mode"] + o, out=lines.append) == 2
        assert "nearest" in lines[-1] and "--levels" in lines[-1]
    assert tool.main([f, "--tile", "64", "--levels", "3", "--filter", "median"] + o, out=lines.append) == 2
    assert tool.main([f, "--tile", "64", "--levels", "3", "--filter", "mode", "--alpha-weighted"] + o, out=lines.append) == 2 and "box" in lines[-1]
    assert tool.main([f, "--tile", "64", "--levels", "8", "--filter", "nearest"] + o, out=lines.append) == 2 and "1..7" in lines[-1]
    assert not os.path.exists(tmp_path / "o")


def test_decode_thumbnails_keeps_rejecting_both():
    lib = api.load_library()
    fake_ctx = (ctypes.c_ubyte * (1 << 20))()
    buf, out = (ctypes.c_ubyte * 4096)(), (ctypes.c_ubyte * 4096)()
    ctypes.memset(out, 0x5A, 4096)
    so, to, sizes = (ctypes.c_size_t * 2)(0, 1024), (ctypes.c_size_t * 2)(0, 1024), (ctypes.c_int * 2)(40, 40)
    descs = (api.QoiDesc * 2)(api.QoiDesc(4, 4, 4, 0), api.QoiDesc(5, 3, 4, 1))
    for mode in (tiles.NEAREST, tiles.MODE, 2, 3):
        rc = lib.qoimi_decode_thumbnails(ctypes.addressof(fake_ctx), ctypes.addressof(buf), so, sizes, descs, 2, 0, (ctypes.c_uint * 2)(2, 3), mode, ctypes.addressof(out), to, 0, None)
        assert rc == E_ARG and "mode" in api.last_error() and "QOIMI_TILE" not in api.last_error(), (mode, api.last_error())
        assert bytes(out) == b"\x5A" * 4096 and bytes(fake_ctx[:4096]) == b"\0" * 4096
