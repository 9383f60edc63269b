"""Label tensors as the source of qoimi_encode_tiles (QOIMI_TILE_LABELS*), what can be checked without a GPU: the constants in every layer,
qoimi_tile_size with the bits, and every QOIMI_E_ARG case of a label source in the order the header gives - all of them are reported
before the context or the device is looked at, so a block of zeroed host memory stands in for a context and host arrays for device buffers
(the idiom of test_ingest_api.py); the outputs keep their bytes and qoimi_last_error names the cause."""
import ctypes
import os
import re

from qoi_amd import api, tiles
from model_cases import E_ARG, tl, untouched
from model_cases import args  # noqa: F401  (fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U8, I32, I64 = (tiles.label_flags(d) for d in (tiles.L_U8, tiles.L_I32, tiles.L_I64))


def test_constants_in_every_layer():
    header = open(os.path.join(ROOT, "include", "qoi_mi355x.h")).read()
    want = {"QOIMI_TILE_LABELS": tiles.LABELS, "QOIMI_TILE_LABELS_I32": tiles.LABELS_I32, "QOIMI_TILE_LABELS_I64": tiles.LABELS_I64}
    assert list(want.values()) == [2048, 4096, 8192]
    for name, value in want.items():
        m = re.search(r"\b%s\s*=\s*(\d+)" % name, header)
        assert m and int(m.group(1)) == value, name
    assert tiles.LABELS_MASK == 0x3800 and tiles.SRC_MASK == 0x3F0
    core = open(os.path.join(ROOT, "qoi_amd", "csrc", "qoi_label_core.h")).read()
    assert re.search(r"kTileLabels\s*=\s*2048\b", core) and re.search(r"kTileLabelsDtypeShift\s*=\s*12\b", core) and re.search(r"kTileKindLabel\s*=\s*4\b", core)
    mk = open(os.path.join(ROOT, "qoi_amd", "csrc", "sources.mk")).read()
    assert "qoi_label.hip" in mk
    # the header, the model and the kernel state the same conversion, and that it is silent
    for text in (header, core, tiles.__doc__):
        flat = " ".join(re.sub(r"(?m)^\s*(/?\*|//)", " ", text).split())
        assert "0 for v < 0, 255 for v > 255, else v" in flat and "2^32 is 255" in flat and "-100 becomes" in flat and "(b, b, b, 255)" in flat, text[:60]
    assert "SILENT" in header and "Not here (of label sources)" in header


def test_the_label_kernel_has_no_timer_entry():
    lib = api.load_library()
    names = [lib.qoimi_kernel_name(i).decode() for i in range(64)]
    assert not any("label_ingest" in n for n in names)


def test_tile_size_with_the_bits():
    lib = api.load_library()
    for lab in (U8, I32, I64):
        for flips in range(4):
            for f in (1, 2, 16, 64):                                   # no mode argument: the averaging rule is not applied
                for ch_in in (3, 4):
                    for ch in (0, 3, 4):
                        t = (7, 3, 2, 30, 17, f, lab | flips)
                        tw, th = -(-30 // f), -(-17 // f)
                        assert api.tile_size(37, 23, ch_in, t, ch) == tiles.size(37, 23, ch_in, t, ch) == (tw * th * (ch or ch_in), tw, th)   # no size changes
    bad = [tiles.LABELS_I32, tiles.LABELS_I64, 12288, tiles.LABELS_I64 | 1,                                                    # no LABELS
           tiles.LABELS | 12288,                                                                                               # no dtype
           tiles.LABELS | tiles.SRC, I64 | tiles.SRC_CHW, I32 | tiles.source_flags(tiles.F16), U8 | tiles.SRC_BYTES,           # with a SRC bit
           tiles.LABELS | 4, tiles.LABELS | 8, I64 | 1 << 10, I32 | 1 << 31, U8 | 1 << 14, 1 << 10, 1 << 14]                   # bits that stay unknown
    for flags in bad:
        tw, th = ctypes.c_uint(77), ctypes.c_uint(78)
        t = api.QoimiTile(0, 0, 0, 4, 4, 1, flags, 0)
        assert lib.qoimi_tile_size(ctypes.byref(api.QoiDesc(4, 4, 4, 0)), ctypes.byref(t), 0, ctypes.byref(tw), ctypes.byref(th)) == 0, flags
        assert (tw.value, th.value) == (77, 78) and tiles.size(4, 4, 4, t, 0) == (0, 0, 0)


def test_rejections_in_order(args):  # noqa: F811
    a = args
    # images: 0 is 4 x 4 (descriptor channels 4), 2 is 5 x 3 (channels 3); 1 is named by no tile; a.p is 8-aligned at least (ctypes)

    def call(po=(0, 1024, 2048), tiles_=None, mode=tiles.NEAREST, pack=a.pack, cap=1024, px=a.p, staging=0):
        return a.lib.qoimi_encode_tiles(a.ctx, px, (ctypes.c_size_t * 3)(*po), a.descs, 3, 0, tiles_, len(tiles_), mode, 1, pack, cap, a.off, a.len, staging,
                                        a.h_off, a.h_len, a.h_desc, None)

    assert a.p % 8 == 0
    t0 = (0, 1, 1, 2, 2, 1, I32, 0)
    t2 = (2, 0, 0, 5, 3, 1, I64 | 3, 0)
    cases = [
        # 1: a dtype bit without QOIMI_TILE_LABELS - behind every check that exists today
        ("I32 without LABELS", lambda: call(tiles_=tl(t0, (2, 0, 0, 5, 3, 1, tiles.LABELS_I32, 0))), "without QOIMI_TILE_LABELS"),
        ("12288 without LABELS, averaged at factor 2", lambda: call(tiles_=tl(t0, (2, 0, 0, 5, 3, 2, 12288 | 1, 0)), mode=tiles.PLAIN), "without QOIMI_TILE_LABELS"),
        ("an unknown bit comes first", lambda: call(tiles_=tl(t0, (2, 0, 0, 5, 3, 1, tiles.LABELS_I32 | 4, 0))), "unknown flag bit"),
        ("bit 10 stays unknown", lambda: call(tiles_=tl(t0, (2, 0, 0, 5, 3, 1, I64 | 1 << 10, 0))), "unknown flag bit"),
        ("bit 14 stays unknown", lambda: call(tiles_=tl(t0, (2, 0, 0, 5, 3, 1, I64 | 1 << 14, 0))), "unknown flag bit"),
        ("bit 31 stays unknown", lambda: call(tiles_=tl(t0, (2, 0, 0, 5, 3, 1, U8 | 1 << 31, 0))), "unknown flag bit"),
        ("reserved comes first", lambda: call(tiles_=tl(t0, (2, 0, 0, 5, 3, 1, tiles.LABELS_I64, 1))), "reserved"),
        ("the rectangle comes first", lambda: call(tiles_=tl(t0, (2, 1, 0, 5, 3, 1, tiles.LABELS_I64, 0))), "leaves"),
        ("factor above 16 with QOIMI_TILE_MODE comes first", lambda: call(tiles_=tl(t0, (2, 0, 0, 5, 3, 17, tiles.LABELS_I64, 0)), mode=tiles.MODE), "factor above 16"),
        ("a label tile votes over at most 16 x 16 too", lambda: call(tiles_=tl(t0, (2, 0, 0, 5, 3, 17, I64, 0)), mode=tiles.MODE), "factor above 16"),
        ("the checks of QOIMI_TILE_SRC come first", lambda: call(tiles_=tl(t0, (2, 0, 0, 5, 3, 1, tiles.LABELS_I64 | tiles.SRC_CHW, 0))), "without QOIMI_TILE_SRC"),
        ("... its factor check too", lambda: call(tiles_=tl(t0, (2, 0, 0, 5, 3, 2, I64 | tiles.SRC, 0))), "factor 1 only"),
        # 2: dtype 12288
        ("dtype 12288", lambda: call(tiles_=tl(t0, (2, 0, 0, 5, 3, 1, tiles.LABELS | 12288, 0))), "12288 is not a dtype"),
        ("dtype 12288 with a SRC bit, averaged at factor 1", lambda: call(tiles_=tl(t0, (2, 0, 0, 5, 3, 1, tiles.LABELS | 12288 | tiles.SRC, 0)), mode=tiles.PLAIN), "12288 is not a dtype"),
        # 3: with a bit of the QOIMI_TILE_SRC mask
        ("LABELS with SRC", lambda: call(tiles_=tl(t0, (2, 0, 0, 5, 3, 1, U8 | tiles.SRC, 0))), "together with a QOIMI_TILE_SRC"),
        ("I64 with a whole tensor format", lambda: call(tiles_=tl(t0, (2, 0, 0, 5, 3, 1, I64 | tiles.source_flags(tiles.F32, tiles.CHW, tiles.BYTES), 0)), mode=tiles.PLAIN), "together with a QOIMI_TILE_SRC"),
        # 4: an averaging mode with factor != 1
        ("PLAIN at factor 2", lambda: call(tiles_=tl(t0, (2, 0, 0, 5, 3, 2, I64, 0)), mode=tiles.PLAIN), "never averaged"),
        ("ALPHA_WEIGHTED at factor 64, in a mixed call", lambda: call(tiles_=tl((0, 0, 0, 4, 4, 1, 0, 0), (2, 0, 0, 5, 3, 64, U8, 0)), mode=tiles.ALPHA_WEIGHTED), "never averaged"),
        # 5: some but not all tiles carry LABELS (before 6 and 7: image 0 would be misaligned and of two dtypes)
        ("a byte tile in a label call", lambda: call(po=(1, 1024, 2048), tiles_=tl(t0, (0, 0, 0, 4, 4, 1, 0, 0), t2)), "a byte call, a tensor call or a label call"),
        ("a label tile in a byte call", lambda: call(tiles_=tl((0, 0, 0, 4, 4, 2, 0, 0), (2, 0, 0, 5, 3, 1, U8, 0))), "a byte call, a tensor call or a label call"),
        ("a label tile in a tensor call: the existing message", lambda: call(tiles_=tl((0, 0, 0, 4, 4, 1, tiles.SRC, 0), (2, 0, 0, 5, 3, 1, I64, 0))), "a byte call or a tensor call"),
        # 6: one image with two label dtypes (before 7: image 0 at an odd address)
        ("image 0 as i32 and as u8", lambda: call(po=(1, 1024, 2048), tiles_=tl(t0, (0, 0, 0, 1, 1, 1, U8, 0))), "two different label dtypes"),
        ("image 2 as i64 and as i32", lambda: call(tiles_=tl(t2, t0, (2, 0, 0, 1, 1, 2, I32, 0))), "two different label dtypes"),
        # 7: the address is not a multiple of E (before 8: the image would wrap the address space)
        ("i32 at an odd offset", lambda: call(po=(1, 1024, 2048), tiles_=tl(t0, t2)), "multiple of the element size"),
        ("i32 at offset 2", lambda: call(po=(2, 1024, 2048), tiles_=tl(t0, t2)), "multiple of the element size"),
        ("i64 at offset 4", lambda: call(po=(0, 1024, 2052), tiles_=tl(t0, t2)), "multiple of the element size"),
        ("i64 at an aligned offset of an odd d_pixels", lambda: call(px=a.p + 4, po=(4, 1024, 2048), tiles_=tl(t0, t2)), "multiple of the element size"),
        ("i64 at an odd offset that also wraps", lambda: call(po=(0, 1024, 2 ** 64 - 9), tiles_=tl(t0, t2)), "multiple of the element size"),
        # 8: extents over w * h * E bytes.  Image 2 is 5 x 3 i64 = 120 bytes (45 as a 3-channel byte image), image 0 is 4 x 4 i32 = 64 bytes
        ("image end wraps the address space, counted in bytes", lambda: call(po=(0, 1024, 2 ** 64 - a.p - 112), tiles_=tl(t0, t2)), "address space"),
        ("image 2's last element lies in the pack", lambda: call(po=(0, 1024, 4096 - 112), tiles_=tl(t0, t2)), "overlap"),
        ("image 0's last element reaches into the pack", lambda: call(po=(4096 - 60, 1024, 2048), tiles_=tl(t0, t2)), "overlap"),
        ("the pack behind image 2's 45th byte", lambda: call(pack=a.p + 2048 + 45, cap=8, tiles_=tl(t0, t2)), "overlap"),
        ("the pack inside image 2's last element", lambda: call(pack=a.p + 2048 + 119, cap=1, tiles_=tl(t0, t2)), "overlap"),
    ]
    for name, c, cause in cases:
        assert c() == E_ARG, name
        assert cause in api.last_error(), (name, api.last_error())
        assert untouched(a), name


def test_what_is_not_rejected_is_not_rejected_for_the_wrong_reason(args):  # noqa: F811
    """planes that end one byte in front of the pack - in bytes of their dtype, one plane whatever the descriptor's channels say - pass the
    overlap check, and every legal dtype, mode and factor passes the label checks: such calls get as far as the context, which this test must
    not do, so it is the tile limit (9) that stops them.  The limit counts the label kernel's items: four output pixels each at factor 1,
    tile_select's above."""
    a = args
    w, h = 19999, 20000
    descs = (api.QoiDesc * 1)(api.QoiDesc(w, h, 3, 0))
    for lab in (U8, I32, I64):
        nbytes = tiles.label_bytes(w, h, lab)
        assert nbytes == w * h * {U8: 1, I32: 4, I64: 8}[lab]
        for mode, f in ((0, 1), (1, 1), (4, 1), (5, 1), (4, 2), (4, 64), (5, 2), (5, 16)):
            per = tiles.label_tiles(w, h, f, 3, mode)
            n = -(-(2 ** 31 - 1) // per)
            assert per * n >= 2 ** 31 - 1 > per * (n - 1)
            if n > 6000:
                continue                                               # (f = 64: too few items a tile to reach the limit with a short list)
            many = (api.QoimiTile * n)(*[api.QoimiTile(0, 0, 0, w, h, f, lab | (j & 3), 0) for j in range(n)])
            for pack, cap in ((a.p - 64, 64), (a.p + nbytes, 64), (None, 0)):
                rc = a.lib.qoimi_encode_tiles(a.ctx, a.p, (ctypes.c_size_t * 1)(0), descs, 1, 0, many, n, mode, 1, pack, cap, a.off, a.len, 1 << 60, a.h_off, a.h_len, a.h_desc, None)
                assert rc == E_ARG and "tiles of work items" in api.last_error(), (lab, mode, f, api.last_error())
                assert untouched(a)
    # the count is the label kernel's: tile_gather's items at factor 1 (16 bytes of och 3 each, fewer than four pixels' 12) stay below the limit
    per = tiles.label_tiles(w, h, 1, 3, 0)
    n = -(-(2 ** 31 - 1) // per)
    assert -(-(-(-w * h * 3 // 16)) // 256) * n < 2 ** 31 - 1 <= per * n
