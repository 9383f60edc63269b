"""The two ends of 24-bit label ids as the GPU runs them - the item arithmetic of label_ingest with QOIMI_TILE_LABELS_ID24
(qoi_amd/csrc/qoi_label_core.h) and the store of QOIMI_TENSOR_HW_ID24 (qoi_amd/csrc/qoi_tensor_core.h: tensor_store) - compiled with g++
(tests/host/label_id_host.cpp) and compared with the Python models qoi_amd/tiles.py and qoi_amd/tensors.py on the CPU: every item of every
tile of small planes - every dtype, both och, all four flips, the copy at factor 1, the centre element and the vote above it, rectangles at
odd x and y, partial edge blocks, every alignment of the plane's address at which the kernel takes another load.  The host's memory functor
checks every address: a load is whole, naturally aligned elements of the plane (u8: an aligned dword that holds one of its bytes), a store
lies in the slot or in the tensor and no byte is stored twice.  Every comparison is exact.  The same file with a main of its own is built
with the address and undefined-behaviour sanitizers and run directly against a plain counting loop."""
import ctypes

import numpy as np
import pytest

import hostbuild
from hostbuild import Banded, i64, i64p, u32, u32p, u64, u8p
from qoi_amd import tensors, tiles

SRC = "label_id_host.cpp"
DTYPES = (tiles.L_U8, tiles.L_I32, tiles.L_I64)
# the residues of the plane's address modulo 16 at which the loads differ
RESIDUES = {tiles.L_U8: (0, 1, 2, 3), tiles.L_I32: (0, 4, 8, 12), tiles.L_I64: (0, 8)}
# ids whose low, middle and high bytes differ one at a time: votes, ties between them and constants all happen
FEW = [0, 1, 256, 65536, 65537, 2 ** 24 - 1, 70000, 513]
WILD = [2 ** 24, -1, -100, 2 ** 31 - 1, -2 ** 31, 2 ** 32, 2 ** 32 + 5, -2 ** 32 + 7, 2 ** 63 - 1, -2 ** 63]
# (w, h) of the plane and the rectangle (x, y, cw, ch) in it
RECTS = [((4, 4), (1, 1, 1, 1)), ((6, 4), (1, 3, 3, 1)), ((7, 4), (3, 1, 4, 1)), ((8, 4), (1, 1, 5, 1)), ((41, 27), (3, 1, 37, 23)), ((1030, 3), (5, 1, 1024, 1)),
         ((37, 23), (0, 0, 37, 23))]
# (mode, factor): the copy (f = 1) in two modes' names, the vote at 2, 3 and 16, the centre at 2 and 64
REDUCTIONS = [(tiles.PLAIN, 1), (tiles.MODE, 1), (tiles.MODE, 2), (tiles.MODE, 3), (tiles.MODE, 16), (tiles.NEAREST, 2), (tiles.NEAREST, 64)]


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    return hostbuild.shared(SRC, tmp_path_factory, {
        "label_id_host_run": (i64, [ctypes.c_void_p, u32, u32, u32, u32, u32, u32, u32, u32, u32, u32, u32, u64, u64, u8p, u8p, u64, i64p]),
        "label_id_host_cfg": (u32, [u32, u32, u32, u32]),
        "label_id_host_ids": (None, [u32p, u32, u32p, u32p]),
        "label_id_host_store": (i64, [u32p, u32, u32, u32, u32, u64, u64, u8p, u8p, u64])})


def plane(w, h, dtype, res, seed):
    """the ids of FEW in short runs (a u8 plane: 0, 85, 170, 255) with every sixteenth element, where the dtype can hold it, far outside
    0..2^24 - 1; inside a buffer of other bytes, its first element `res` bytes behind a 16-aligned address"""
    rng = np.random.default_rng(seed)
    elem = tiles.LABEL_ELEM[dtype]
    raw = np.full(w * h * elem + 96, 0x5A, dtype=np.uint8)
    at = (-raw.ctypes.data) % 16 + 16 + res
    A = raw[at:at + w * h * elem].view(tiles.LABEL_ARRAYS[dtype]).reshape(h, w)
    pick = np.repeat(rng.integers(0, 8, size=w * h), rng.integers(1, 4, size=w * h))[:w * h]
    if dtype == tiles.L_U8:
        v = (pick % 4) * 85
    else:
        lo, hi = (-2 ** 31, 2 ** 31 - 1) if dtype == tiles.L_I32 else (-2 ** 63, 2 ** 63 - 1)
        wild = np.array([x for x in WILD if lo <= x <= hi], dtype=np.int64)
        v = np.where(rng.integers(0, 16, size=w * h) == 0, wild[rng.integers(0, wild.size, size=w * h)], np.array(FEW, dtype=np.int64)[pick])
    A[:] = v.reshape(h, w).astype(tiles.LABEL_ARRAYS[dtype])
    assert A.ctypes.data % 16 == res
    return raw, A


def stored_bytes(P, och, f):
    """bytes of the slot a tile of P output pixels stores: whole 16-byte items at och 4 and the dwords that hold a byte at och 3 (factor 1),
    the pixels themselves above"""
    return P * och if f != 1 else 16 * -(-P // 4) if och == 4 else 4 * -(-3 * P // 4)


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_item_of_every_id_tile_reproduces_the_model(host_lib, dtype):
    checked, wide, coloured = 0, 0, 0
    for (w, h), (x, y, cw, ch) in RECTS:
        for res in RESIDUES[dtype]:
            raw, A = plane(w, h, dtype, res, seed=w * 131 + h * 7 + res)
            before = raw.copy()
            for mode, f in REDUCTIONS:
                if f > 1 and cw * ch > 2000 and f != 2:
                    continue                                           # (the long row: the copy and one reduction of each kind are enough)
                tw, th = -(-cw // f), -(-ch // f)
                for flips in range(4):
                    for och in (3, 4):
                        flags = tiles.label_flags(dtype, ids=True) | flips
                        want = tiles.tile(A, (0, x, y, cw, ch, f, flags), och, mode)
                        nbytes = tw * th * och
                        band = Banded(stored_bytes(tw * th, och, f), 0, band=256)
                        loads = (ctypes.c_longlong * 4)()
                        rc = host_lib.label_id_host_run(A.ctypes.data, w, h, dtype, x, y, cw, ch, f, flips | tiles.LABELS_ID24, och, 1 if mode == tiles.MODE else 0, *band.args, loads)
                        what = ((w, h), (x, y, cw, ch), res, mode, f, flips, och)
                        assert rc >= 0, (what, "bad accesses", -1 - rc)
                        assert rc == tiles.label_tiles(cw, ch, f, och, mode if f > 1 else tiles.PLAIN) >= 1, what
                        got = band.inside(what)                        # every stored byte once, none beside them, none behind the slot
                        got = got[:nbytes].reshape(th, tw, och)
                        assert np.array_equal(got, want), what
                        coloured += int((got[:, :, 0] != got[:, :, 1]).any() and (got[:, :, 1] != got[:, :, 2]).any())
                        if f == 1 and cw >= 4 and dtype != tiles.L_U8:
                            wide += loads[2]
                        checked += 1
                        if och == 4 and flips == 0:
                            # the other end: the tile's pixels through tensor_store come back as the ids tensors.convert gives
                            px = np.ascontiguousarray(got).view(np.uint32).reshape(-1)
                            for td in (tensors.I32, tensors.I64):
                                E = tensors.INT_ELEM[td]
                                for a in (0, E):
                                    out = Banded(tw * th * E, a)
                                    n = host_lib.label_id_host_store(px.ctypes.data_as(u32p), tw, th, och, td, *out.args)
                                    assert n == tw * th * (E // 4), (what, td, n)
                                    ids = out.inside(what).view(tensors.numpy_dtype(td)).reshape(th, tw)
                                    assert np.array_equal(ids, tensors.convert(got, tensors.fmt(td, tensors.HW_ID24))), (what, td)
            assert np.array_equal(raw, before)                          # the source is only read
    assert checked >= 7 * len(RESIDUES[dtype]) * 4 * 8
    if dtype != tiles.L_U8:
        assert wide > 0 and coloured > 0                                # the 16-byte loads were taken; r, g and b differed somewhere


def test_the_store_ignores_alpha_and_keeps_to_its_elements(host_lib):
    """pixels with every alpha, as I32 and I64, at och 3 and 4, the output at an element-aligned address that is no multiple of 16"""
    rng = np.random.default_rng(24)
    ow, oh = 13, 5
    px = rng.integers(0, 2 ** 32, size=ow * oh, dtype=np.uint64).astype(np.uint32)
    P = np.ascontiguousarray(px).view(np.uint8).reshape(oh, ow, 4)
    for td in (tensors.I32, tensors.I64):
        E = tensors.INT_ELEM[td]
        for och in (3, 4):
            out = Banded(ow * oh * E, E)
            n = host_lib.label_id_host_store(px.ctypes.data_as(u32p), ow, oh, och, td, *out.args)
            assert n == ow * oh * (E // 4)
            ids = out.inside((td, och)).view(tensors.numpy_dtype(td)).reshape(oh, ow)
            assert np.array_equal(ids, (px & 0xFFFFFF).reshape(oh, ow).astype(np.int64))
            assert np.array_equal(ids, tensors.convert(P[:, :, :och], tensors.fmt(td, tensors.HW_ID24)))
        # a store at an address that is no multiple of the element is a bad access, not a silent one
        out = Banded(ow * oh * E, 2)
        assert host_lib.label_id_host_store(px.ctypes.data_as(u32p), ow, oh, 4, td, *out.args) < 0


def test_the_entry(host_lib):
    for ids in (False, True):
        for dtype in DTYPES:
            for f, vote in ((1, 0), (1, 1), (2, 0), (2, 1), (3, 1), (16, 1), (64, 0)):
                for och in (3, 4):
                    for flips in range(4):
                        cfg = host_lib.label_id_host_cfg(tiles.label_flags(dtype, ids) | flips, f, vote, och)
                        lg, c = tiles.select_split(f, tiles.MODE if vote else tiles.NEAREST) if f > 1 else (0, 1)
                        field = dtype + (4 if ids else 0)               # 0 / 1 / 2 stay what they were; ids are 4 / 5 / 6
                        assert cfg == lg | c << 8 | field << 16 | och << 20 | (1 if vote and f > 1 else 0) << 24 | 4 << 25 | flips << 28, (ids, dtype, f, vote, och, flips)


def test_the_saturation_alone(host_lib):
    """int64 values as their two dwords: the listed ones, the neighbourhood of every power of two and random patterns"""
    r = np.random.default_rng(8)
    near = [s * 2 ** k + d for k in range(64) for s in (1, -1) for d in (-1, 0, 1)]
    v = np.array([x for x in WILD + FEW + [255, 65535] + near if -2 ** 63 <= x <= 2 ** 63 - 1], dtype=np.int64)
    v = np.concatenate([v, r.integers(-2 ** 63, 2 ** 63 - 1, size=20000, dtype=np.int64), r.integers(-2 ** 25, 2 ** 25, size=20000, dtype=np.int64)])
    words = np.ascontiguousarray(v).view(np.uint32)
    out64, out32 = np.zeros(v.size, np.uint32), np.zeros(v.size, np.uint32)
    host_lib.label_id_host_ids(words.ctypes.data_as(u32p), v.size, out64.ctypes.data_as(u32p), out32.ctypes.data_as(u32p))

    def ids(A, dtype):
        B = tiles.label_ids_to_bytes(A[None, :], tiles.label_flags(dtype, ids=True))[0].astype(np.uint32)
        assert np.all(B[:, 3] == 255)
        return B[:, 0] | B[:, 1] << 8 | B[:, 2] << 16

    assert np.array_equal(out64, ids(v, tiles.L_I64))
    low = words[0::2].view(np.int32)
    assert np.array_equal(out32, ids(low, tiles.L_I32))
    assert np.array_equal(out64, np.clip(v, 0, 2 ** 24 - 1).astype(np.uint32))
    for value, want in ((2 ** 32, 2 ** 24 - 1), (2 ** 32 + 5, 2 ** 24 - 1), (-2 ** 32 + 7, 0), (-2 ** 63, 0), (2 ** 63 - 1, 2 ** 24 - 1), (2 ** 24, 2 ** 24 - 1), (65537, 65537)):
        assert (v == value).any() and np.all(out64[v == value] == want), value


def test_standalone_program_under_sanitizers(tmp_path):
    """label_id_host.cpp with its own main and its own counting-loop model, built with AddressSanitizer and UndefinedBehaviorSanitizer, run directly"""
    out = hostbuild.sanitized(SRC, "LABEL_ID_HOST_MAIN", tmp_path)
    assert out.startswith("label_id_host: ") and out.endswith(" tiles ok\n") and int(out.split()[1]) == 5 * 10 * 2 * (6 + 5) * 4 * 2, out
