"""24-bit label ids in the models: ``tiles.LABELS_ID24`` (qoi_amd/tiles.py: label_ids_to_bytes) and ``tensors.HW_ID24``
(qoi_amd/tensors.py: convert) - the constants, the saturation value by value, the three properties the header states, the order of the
vote's tie rule, the rejections in the order the calls look, and the bits that stay unknown.  No GPU."""
import numpy as np
import pytest

from qoi_amd import mode as mode_model, tensors, tiles

ID_MAX = 2 ** 24 - 1
BOUNDARY = [-2 ** 63, -2 ** 31, -1, 0, 255, 256, 65535, 65536, 2 ** 24 - 1, 2 ** 24, 2 ** 31 - 1, 2 ** 32, 2 ** 32 + 5, 2 ** 63 - 1]
RANGES = {tiles.L_U8: (0, 255), tiles.L_I32: (-2 ** 31, 2 ** 31 - 1), tiles.L_I64: (-2 ** 63, 2 ** 63 - 1)}
U8, I32, I64 = (tiles.label_flags(d, ids=True) for d in (tiles.L_U8, tiles.L_I32, tiles.L_I64))


def ids_of(B):
    """r | g << 8 | b << 16 of uint8[..., 3 or 4]"""
    B = B.astype(np.int64)
    return B[..., 0] | B[..., 1] << 8 | B[..., 2] << 16


def test_constants():
    assert tiles.LABELS_ID24 == 32768 == 1 << 15 and tiles.ID_MAX == ID_MAX
    assert tiles.LABELS_MASK == 0x3800 and tiles.SRC_MASK == 0x3F0
    assert (tiles.LABELS, tiles.LABELS_I32, tiles.LABELS_I64) == (2048, 4096, 8192)
    assert [tiles.label_flags(d, ids=True) for d in (0, 1, 2)] == [2048 | 32768, 2048 | 4096 | 32768, 2048 | 8192 | 32768]
    assert [tiles.label_flags(d) for d in (0, 1, 2)] == [2048, 2048 | 4096, 2048 | 8192]
    assert [tiles.label_dtype(f) for f in (U8, I32, I64)] == [0, 1, 2]
    assert tensors.HW_ID24 == 5 and tensors.HW == 3
    assert tensors.LAYOUT_NAMES == {"hwc": 0, "chw": 1, "hw": 3} and tensors.INT_ELEM == {5: 4, 6: 8}
    assert tensors.ID_LAYOUT_NAMES == {"id24": 5}


@pytest.mark.parametrize("dtype", [tiles.L_U8, tiles.L_I32, tiles.L_I64])
def test_saturation_value_by_value(dtype):
    lo, hi = RANGES[dtype]
    values = [v for v in BOUNDARY if lo <= v <= hi]
    assert len(values) == {tiles.L_U8: 2, tiles.L_I32: 10, tiles.L_I64: 14}[dtype]
    A = np.array([values], dtype=tiles.LABEL_ARRAYS[dtype])
    B = tiles.label_ids_to_bytes(A, tiles.label_flags(dtype, ids=True))
    assert B.shape == (1, len(values), 4) and B.dtype == np.uint8 and np.all(B[:, :, 3] == 255)
    for v, px in zip(values, B[0]):
        want = 0 if v < 0 else ID_MAX if v > ID_MAX else v
        assert tuple(px) == (want & 255, (want >> 8) & 255, want >> 16, 255), v
    # the dword of a pixel is id | 0xFF000000
    assert np.array_equal(B.view(np.uint32)[0, :, 0], np.array([(0 if v < 0 else min(v, ID_MAX)) | 0xFF000000 for v in values], dtype=np.uint32))
    if dtype == tiles.L_I64:
        assert ids_of(B)[0, values.index(2 ** 32 + 5)] == ID_MAX and ids_of(B)[0, values.index(2 ** 32)] == ID_MAX      # not 5, not 0
    # labels_to_bytes goes the same way with the bit, and keeps its bytes without it
    assert np.array_equal(tiles.labels_to_bytes(A, tiles.label_flags(dtype, ids=True)), B)
    plain = tiles.labels_to_bytes(A, tiles.label_flags(dtype))
    assert np.array_equal(plain[0, :, 0], np.clip(np.array(values, dtype=object), 0, 255).astype(np.uint8)) and np.all(plain[:, :, 0] == plain[:, :, 1])


def test_a_u8_plane_joins_an_id_pack():
    A = np.arange(256, dtype=np.uint8).reshape(16, 16)
    B = tiles.label_ids_to_bytes(A, U8)
    assert np.array_equal(B[:, :, 0], A) and not B[:, :, 1:3].any() and np.all(B[:, :, 3] == 255)


def test_label_ids_to_bytes_wants_the_bit_and_the_dtype():
    A = np.zeros((2, 2), np.int32)
    for flags in (tiles.label_flags(tiles.L_I32), tiles.LABELS_ID24, tiles.LABELS_ID24 | tiles.LABELS_I32, 0):
        with pytest.raises(ValueError):
            tiles.label_ids_to_bytes(A, flags)
    with pytest.raises(ValueError):
        tiles.label_ids_to_bytes(A, I64)
    with pytest.raises(ValueError):
        tiles.label_ids_to_bytes(A.astype(np.float32), I32)


def random_ids(w, h, dtype, seed):
    rng = np.random.default_rng(seed)
    top = 255 if dtype == tiles.L_U8 else ID_MAX
    A = rng.integers(0, top + 1, size=(h, w)).astype(tiles.LABEL_ARRAYS[dtype])
    A.flat[:4] = [0, top, min(256, top), min(65536, top)][:min(4, A.size)]
    return A


@pytest.mark.parametrize("dtype", [tiles.L_U8, tiles.L_I32, tiles.L_I64])
def test_property_a_the_round_trip(dtype):
    """whole-image tiles at factor 1, then NEAREST at the image's size as I64 (and I32) with HW_ID24, return the plane widened"""
    for w, h in ((1, 1), (5, 3), (37, 29)):
        A = random_ids(w, h, dtype, w * 100 + h)
        for channels in (0, 3, 4):
            T = tiles.tile(A, (0, 0, 0, w, h, 1, tiles.label_flags(dtype, ids=True)), channels, tiles.NEAREST)
            assert T.shape == (h, w, channels or 4)
            for td in (tensors.I64, tensors.I32):
                out = tensors.tensors(T, (0, 0, w, h), (w, h), 0, tensors.FILTER_NEAREST, tensors.PLAIN, tensors.fmt(td, tensors.HW_ID24))
                assert out.dtype == tensors.numpy_dtype(td) and out.shape == (h, w) and out.flags["C_CONTIGUOUS"]
                assert np.array_equal(out, A.astype(np.int64)), (w, h, channels, td)


def test_property_b_a_call_without_the_bit_gives_the_bytes_it_gave():
    rng = np.random.default_rng(5)
    A = rng.integers(-300, 70000, size=(9, 14)).astype(np.int32)
    for f, m in ((1, tiles.PLAIN), (2, tiles.NEAREST), (3, tiles.MODE)):
        for flips in range(4):
            T = tiles.tile(A, (0, 1, 2, 12, 6, f, tiles.label_flags(tiles.L_I32) | flips), 0, m)
            b = np.clip(A, 0, 255).astype(np.uint8)
            B = np.dstack([b, b, b, np.full_like(b, 255)])
            assert np.array_equal(T, tiles.tile(B, (0, 1, 2, 12, 6, f, flips), 0, m))
            assert np.all(T[:, :, 0] == T[:, :, 1]) and np.all(T[:, :, 1] == T[:, :, 2])
    # ... and the formats that were: HW of an I64 is still channel 0 alone
    P = rng.integers(0, 256, size=(4, 6, 4), dtype=np.uint8)
    assert np.array_equal(tensors.convert(P, tensors.fmt(tensors.I64, tensors.HW)), P[:, :, 0].astype(np.int64))
    assert tiles.size(14, 9, 4, (0, 1, 2, 12, 6, 2, tiles.label_flags(tiles.L_I32))) == tiles.size(14, 9, 4, (0, 1, 2, 12, 6, 2, I32)) == (6 * 3 * 4, 6, 3)


@pytest.mark.parametrize("dtype", [tiles.L_I32, tiles.L_I64])
def test_property_c_a_mode_tile_is_filter_mode_of_the_factor_1_pack(dtype):
    rng = np.random.default_rng(11)
    for w, h, f in ((12, 8, 2), (12, 9, 3), (32, 16, 4), (32, 32, 16)):
        few = np.array([0, 1, 256, 65536, 65537, ID_MAX, 300000])
        A = few[np.repeat(rng.integers(0, few.size, size=w * h), rng.integers(1, 4, size=w * h))[:w * h]].reshape(h, w).astype(tiles.LABEL_ARRAYS[dtype])
        flags = tiles.label_flags(dtype, ids=True)
        T = tiles.tile(A, (0, 0, 0, w, h, f, flags), 4, tiles.MODE)
        one = tiles.tile(A, (0, 0, 0, w, h, 1, flags), 4, tiles.MODE)
        fm = tensors.fmt(tensors.I64, tensors.HW_ID24)
        want = tensors.tensors(one, (0, 0, w, h), (w // f, h // f), 0, tensors.FILTER_MODE, tensors.PLAIN, fm)
        assert np.array_equal(tensors.convert(T, fm), want), (w, h, f)
        assert np.array_equal(T, mode_model.mode(one, (0, 0, w, h), (w // f, h // f)))
        assert set(np.unique(want)) <= set(few.tolist())               # no id is invented


def test_the_tie_is_decided_by_the_bytes_not_by_the_id():
    """blocks in which two ids tie for the largest count and the centre pixel is neither: the winner is the one with the lowest
    r << 24 | g << 16 | b << 8 | a.  Of 1 = (1, 0, 0) and 256 = (0, 1, 0) that is 256, the HIGHER id."""
    A = np.array([[1, 256, 7, 7], [256, 1, 7, 7], [1, 256, 9, 9], [256, 1, 9, 9]], dtype=np.int32)
    # block (0, 0) of f = 4 holds 1 x 4, 256 x 4, 7 x 4, 9 x 4; centre (2, 2) is 9: a winner, so the centre wins
    assert tensors.convert(tiles.tile(A, (0, 0, 0, 4, 4, 4, I32), 4, tiles.MODE), tensors.fmt(tensors.I64, tensors.HW_ID24))[0, 0] == 9
    # 3 x 3 blocks of f = 3 over a 3 x 3 plane: 1 and 256 four times each, the centre 70000 once
    C = np.array([[1, 256, 1], [256, 70000, 256], [1, 256, 1]], dtype=np.int64)
    C[2, 2] = 5                                                        # 1 three times, 256 four times: one winner, the larger count
    assert ids_of(tiles.tile(C, (0, 0, 0, 3, 3, 3, I64), 3, tiles.MODE))[0, 0] == 256
    C[0, 1] = 6                                                        # 1 three times, 256 three times, centre once: the tie
    got = ids_of(tiles.tile(C, (0, 0, 0, 3, 3, 3, I64), 4, tiles.MODE))[0, 0]
    assert got == 256 and got != min(1, 256)
    # the same tie between 2 = (2, 0, 0) and 513 = (1, 2, 0): the low byte decides
    D = np.array([[2, 513, 2], [513, 70000, 513], [6, 5, 2]], dtype=np.int64)
    assert ids_of(tiles.tile(D, (0, 0, 0, 3, 3, 3, I64), 4, tiles.MODE))[0, 0] == 513      # r = 1 < r = 2
    E = np.array([[3, 259, 3], [259, 70000, 259], [6, 5, 3]], dtype=np.int64)               # 3 = (3, 0, 0), 259 = (3, 1, 0): r ties, g decides
    assert ids_of(tiles.tile(E, (0, 0, 0, 3, 3, 3, I64), 4, tiles.MODE))[0, 0] == 3


def test_rejections_in_call_order():
    # tiles: the unknown bits first (size), then the tensor-source checks, then the label checks in their order
    assert tiles.label_wrong(tiles.LABELS_ID24) == "a LABELS_* bit without LABELS"
    assert tiles.label_wrong(tiles.LABELS_ID24 | tiles.LABELS_I32) == "a LABELS_* bit without LABELS"
    assert tiles.label_wrong(tiles.LABELS_ID24 | 12288) == "a LABELS_* bit without LABELS"
    assert tiles.label_wrong(tiles.LABELS | tiles.LABELS_ID24 | 12288) == "12288 is not a dtype"
    assert tiles.label_wrong(I32 | tiles.SRC) == "LABELS together with a SRC bit"
    assert tiles.label_wrong(I64, 2, tiles.PLAIN) == tiles.label_wrong(I64, 2, tiles.ALPHA_WEIGHTED) == "a label source is never averaged"
    assert tiles.label_wrong(I64, 2, tiles.NEAREST) == tiles.label_wrong(I64, 16, tiles.MODE) == tiles.label_wrong(I64, 1, tiles.PLAIN) == tiles.label_wrong(U8) == ""
    assert tiles.source_wrong(tiles.LABELS_ID24 | tiles.SRC_CHW) == "a SRC_* bit without SRC"          # looked at in front of the label checks
    for flags in (tiles.LABELS_ID24, tiles.LABELS_ID24 | 1, tiles.LABELS_ID24 | tiles.LABELS_I64, I32 | tiles.SRC, tiles.LABELS | tiles.LABELS_ID24 | 12288):
        assert tiles.size(8, 8, 4, (0, 0, 0, 8, 8, 1, flags)) == (0, 0, 0), flags
    for flags in (U8, I32, I64, I64 | 3):
        assert tiles.size(8, 8, 3, (0, 0, 0, 8, 8, 2, flags)) == (48, 4, 4) and tiles.size(8, 8, 3, (0, 0, 0, 8, 8, 64, flags), 4) == (4, 1, 1)
    with pytest.raises(ValueError, match="never averaged"):
        tiles.tile(np.zeros((4, 4), np.int32), (0, 0, 0, 4, 4, 2, I32), 0, tiles.PLAIN)
    # an image is bytes or ids; images with and without the bit mix in one label call
    descs = [(8, 8, 4), (8, 8, 3)]
    with pytest.raises(ValueError, match="two label dtypes"):
        tiles.plan(descs, [(0, 0, 0, 8, 8, 1, I32), (0, 0, 0, 4, 4, 1, tiles.label_flags(tiles.L_I32))], 0, 0)
    with pytest.raises(ValueError, match="label call"):
        tiles.plan(descs, [(0, 0, 0, 8, 8, 1, I32), (1, 0, 0, 4, 4, 1, 0)], 0, 0)
    slots, subs, _, named = tiles.plan(descs, [(0, 0, 0, 8, 8, 1, I32), (1, 0, 0, 4, 4, 1, tiles.label_flags(tiles.L_I64)), (0, 0, 0, 8, 8, 2, I32 | 1)], 0, 0)
    assert len(slots) == 3 and named == 2 and slots == tiles.plan(descs, [(0, 0, 0, 8, 8, 1, 0), (1, 0, 0, 4, 4, 1, 0), (0, 0, 0, 8, 8, 2, 1)], 0, 0)[0]
    # tensors: dtype, layout, finiteness, the integer dtypes' scale and bias, and LAST the id layout's dtype
    ok = (1, 1, 1, 1), (0, 0, 0, 0)
    assert tensors.wrong(tensors.fmt(tensors.I32, tensors.HW_ID24)) == tensors.wrong(tensors.fmt(tensors.I64, tensors.HW_ID24)) == ""
    for td in (tensors.U8, tensors.F16, tensors.BF16, tensors.F32):
        assert "ID24" in tensors.wrong(tensors.fmt(td, tensors.HW_ID24, *ok)), td
    assert tensors.wrong(tensors.fmt(4, tensors.HW_ID24)) == tensors.wrong(tensors.fmt(7, tensors.HW_ID24)) == "unknown dtype"
    for layout in (2, 4, 6, 7, 9):
        assert tensors.wrong(tensors.fmt(tensors.I64, layout)) == "unknown layout", layout
    assert tensors.wrong(tensors.fmt(tensors.F32, tensors.HW_ID24, (1, np.inf, 1, 1))) == "scale or bias is not finite"
    assert tensors.wrong(tensors.fmt(tensors.U8, tensors.HW_ID24, (1, 2, 1, 1))) == "QOIMI_TENSOR_U8 takes scale 1 and bias +0 only"
    assert tensors.wrong(tensors.fmt(tensors.I64, tensors.HW_ID24, (1, 1, 1, 1), (0, 0, -0.0, 0))) == "QOIMI_TENSOR_I64 takes scale 1 and bias +0 only"
    with pytest.raises(ValueError, match="ID24"):
        tensors.convert(np.zeros((2, 2, 4), np.uint8), tensors.fmt(tensors.F32, tensors.HW_ID24))
    # sizes count one element per pixel
    assert tensors.size_hw(6 * 5 * 3, 3, tensors.I64) == 240 and tensors.size_hw(6 * 5 * 4, 4, tensors.I32) == 120


def test_the_bits_that_stay_unknown():
    for bit in (2, 3, 10, 14, 31):
        for base in (0, tiles.LABELS, I32, I64 | 3):
            assert tiles.size(8, 8, 4, (0, 0, 0, 8, 8, 1, base | 1 << bit)) == (0, 0, 0), (bit, base)
    for bit in (16, 17, 30):
        assert tiles.size(8, 8, 4, (0, 0, 0, 8, 8, 1, I32 | 1 << bit)) == (0, 0, 0), bit
    assert tiles.size(8, 8, 4, (0, 0, 0, 8, 8, 1, I32)) == (256, 8, 8)


def test_alpha_is_ignored_and_every_filter_is_a_pure_function_of_the_bytes():
    rng = np.random.default_rng(3)
    D = rng.integers(0, 256, size=(9, 11, 4), dtype=np.uint8)
    fm = tensors.fmt(tensors.I32, tensors.HW_ID24)
    assert np.array_equal(tensors.convert(D, fm), tensors.convert(D[:, :, :3], fm))
    assert np.array_equal(tensors.convert(D, fm), ids_of(D).astype(np.int32))
    for flt in (tensors.FILTER_AREA, tensors.FILTER_BILINEAR, tensors.FILTER_NEAREST, tensors.FILTER_MODE):
        P = tensors.tensors(D, (1, 1, 9, 7), (4, 3), 1, flt, tensors.PLAIN, tensors.fmt())
        assert np.array_equal(tensors.tensors(D, (1, 1, 9, 7), (4, 3), 1, flt, tensors.PLAIN, fm), ids_of(P).astype(np.int32))
