"""Which branches of the item arithmetic of tensor_ingest (qoi_amd/csrc/qoi_ingest_core.h) the GPU cases reach, certified on the CPU: the
case lists of tests/ingest_cases.py - the very lists tests/test_gpu_ingest_values.py, tests/test_gpu_ingest.py and
tests/test_gpu_offsets_wide.py run - are replayed through the host build of the core (tests/host/ingest_host.cpp: ingest_host_paths; shape,
format, address modulo 256, rectangle, flips, och) whose memory functor counts the loads of 2, 4, 8 and 16 bytes and the stores of 4, 12 and
16 bytes.  A case list can look complete while an address class goes unvisited - before the 256-aligned placements no GPU case took the
8- or 16-byte load of a four-element HWC pixel -, so the classes are asserted here.  With them: the witness search of the fused
multiply-add, and the conditions the expectations of the GPU modules rest on.  No GPU."""
import numpy as np
import pytest

import hostbuild
import ingest_cases as ic
from hostbuild import i64, u32, u64p
from qoi_amd import tiles

LOAD2, LOAD4, LOAD8, LOAD16, STORE4, STORE12, STORE16 = range(7)
ELEMENT = {tiles.F16: LOAD2, tiles.BF16: LOAD2, tiles.F32: LOAD4}
VECTOR = {tiles.F16: LOAD8, tiles.BF16: LOAD8, tiles.F32: LOAD16}


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    return hostbuild.shared("ingest_host.cpp", tmp_path_factory, {"ingest_host_paths": (i64, [u32] * 11 + [u64p])})


def replay(lib, case):
    """(case, counts uint64[7]) of one tile; every address it forms is legal"""
    w, h, sch, flags, mod, x, y, cw, ch, flips, och = case
    counts = np.zeros(7, dtype=np.uint64)
    rc = lib.ingest_host_paths(w, h, sch, flags, x, y, cw, ch, flips, och, mod, counts.ctypes.data_as(u64p))
    assert rc == tiles.ingest_tiles(cw, ch), (case, rc)
    items = tiles.ingest_items(cw, ch)
    assert int(counts[STORE16]) == (items if och == 4 else 0) and int(counts[STORE12]) == (0 if och == 4 else cw * ch // 4), case
    return case, [int(c) for c in counts]


def crossing(case):
    """whole items (four pixels) of the tile that lie in two rows"""
    cw, ch = case[7], case[8]
    return sum(1 for k in range(cw * ch // 4) if 4 * k % cw + 4 > cw)


def wide_cases():
    from wide_cases import ARENA, B32, tensor_offsets
    offs = tensor_offsets()
    assert all(0 <= o < ARENA for o in offs) and any(o >= B32 for o in offs)
    return ic.cases_of(ic.WIDE_SPECS, offs, ic.wide_tiles(), ic.WIDE_CHANNELS)


@pytest.fixture(scope="module")
def replayed(host_lib):
    lists = {"values": [], "mixed": [], "round trip": ic.round_trip_cases(), "wide": wide_cases(), "big": ic.big_cases(tiles.HWC) + ic.big_cases(tiles.CHW)}
    for dtype in ic.FLOATS:
        specs, hows = ic.value_specs(dtype)
        lists["values"] += ic.cases_of(specs, ic.offsets(specs, hows)[0], ic.value_tiles(specs), ic.VALUE_CHANNELS)
    for k0 in (0, 1):
        for how in (ic.ODD, ic.ALIGNED):
            specs = ic.mixed_specs(k0)
            lists["mixed"] += ic.cases_of(specs, ic.offsets(specs, how)[0], ic.tiles_of(specs, k0), ic.MIXED_CHANNELS)
    return {name: [replay(host_lib, c) for c in cases] for name, cases in lists.items()}


def test_every_load_class_is_reached_by_a_gpu_case(replayed):
    every = [r for rs in replayed.values() for r in rs]
    assert len(every) >= 1000
    for dtype in ic.FLOATS:
        el, vec = ELEMENT[dtype], VECTOR[dtype]
        for layout, sch in ((tiles.CHW, 4), (tiles.CHW, 3), (tiles.HWC, 4)):           # the run of a plane, the pixel of four elements
            mine = [(c, n) for c, n in every if tiles.source_format(c[3])[:2] == (dtype, layout) and c[2] == sch and crossing(c) == 0 and c[7] * c[8] % 4 == 0]
            assert any(n[vec] > 0 and n[el] == 0 for _, n in mine), ("no tile is read by vector loads alone", dtype, layout, sch)
            assert any(n[vec] == 0 and n[el] > 0 for _, n in mine), ("no tile is read by element loads alone", dtype, layout, sch)
            for c, n in mine:                                       # every element is loaded exactly once, four by a vector load
                assert 4 * n[vec] + n[el] == c[7] * c[8] * sch and n[LOAD2 if el == LOAD4 else LOAD4] == 0, (c, n)
        for c, n in every:                                          # HWC, three elements: never a vector load
            if tiles.source_format(c[3])[:2] == (dtype, tiles.HWC) and c[2] == 3:
                assert n[vec] == 0 and n[el] == 3 * c[7] * c[8], (c, n)
        assert any(tiles.source_format(c[3])[:2] == (dtype, tiles.HWC) and c[2] == 3 for c, _ in every)
    # u8: the aligned dwords that hold the bytes - one where the four bytes lie in one dword, else two
    for layout, sch in ((tiles.CHW, 4), (tiles.CHW, 3), (tiles.HWC, 4)):
        mine = [(c, n) for c, n in every if tiles.source_format(c[3])[:2] == (tiles.U8, layout) and c[2] == sch and crossing(c) == 0 and c[7] * c[8] % 4 == 0]
        units = lambda c: c[7] * c[8] // 4 * sch if layout == tiles.CHW else c[7] * c[8]      # noqa: E731  (runs of a plane, or pixels)
        assert any(n[LOAD4] == units(c) for c, n in mine), ("no tile is read by single dwords alone", layout, sch)
        assert any(n[LOAD4] == 2 * units(c) for c, n in mine), ("no tile is read by pairs of dwords alone", layout, sch)
        assert all(units(c) <= n[LOAD4] <= 2 * units(c) and n[LOAD2] == n[LOAD8] == n[LOAD16] == 0 for c, n in mine)


def test_items_cross_rows_and_last_items_are_partial(replayed):
    every = [r for rs in replayed.values() for r in rs]
    for name in ("values", "mixed", "big"):
        chw = [c for c, _ in replayed[name] if tiles.source_format(c[3])[1] == tiles.CHW]
        assert any(crossing(c) > 0 for c in chw), name                                # CHW items that lie in two rows: pixel by pixel
    for dtype in (tiles.U8,) + ic.FLOATS:
        mine = [(c, n) for c, n in every if tiles.source_format(c[3])[0] == dtype]
        assert {c[7] * c[8] % 4 for c, _ in mine} == {0, 1, 2, 3}, dtype              # a last item of 1, 2 and 3 pixels
        assert {n[STORE4] for c, n in mine if c[10] == 3} == {0, 1, 2, 3}, dtype       # which stores 1, 2 and 3 dwords at och 3
        for c, n in mine:
            last = c[7] * c[8] % 4
            assert n[STORE4] == ((3 * last + 3) // 4 if c[10] == 3 else 0), (c, n)
    # in the values module every dtype has all of it by itself
    for dtype in ic.FLOATS:
        mine = [(c, n) for c, n in replayed["values"] if tiles.source_format(c[3])[0] == dtype]
        assert {n[STORE4] for c, n in mine if c[10] == 3} == {0, 1, 2, 3} and {c[9] for c, _ in mine} == {0, 1, 2, 3}


def test_the_long_source_is_read_past_2_32(replayed):
    """part 2 of the wide file: tiles of each layout read elements whose byte offset in the image is at least 2^32, and their aliases
    2^32 bytes lower lie in the decoy windows"""
    for layout in (tiles.HWC, tiles.CHW):
        win = ic.BIG_WINDOWS[layout]
        high = {name: 0 for name in ("control", "fill", "straddle", "last")}
        for name, t in ic.big_tiles(layout):
            _, x, y, cw, ch = t[:5]
            for c in range(4):
                for yy, xx in ((y, x), (y, x + cw - 1), (y + ch - 1, x), (y + ch - 1, x + cw - 1)):
                    i = ic.big_index(layout, yy, xx, c)
                    assert 0 <= i < ic.BIG_SIDE ** 2 * 4
                    if i * 4 >= 1 << 32:
                        high[name] += 1
                        alias = i - (1 << 30)
                        row = alias // 4 // ic.BIG_SIDE if layout == tiles.HWC else alias // ic.BIG_SIDE % ic.BIG_SIDE
                        assert (layout == tiles.HWC or alias < ic.BIG_SIDE ** 2) and any(r0 <= row < r1 for r0, r1 in win["decoys"]), (layout, name, t, row)
        assert high["control"] == high["fill"] == 0 and high["last"] > 0 and high["straddle"] > 0, (layout, high)
        r0, r1 = win["straddle"]
        first = 1 << 30                                                # the element that begins at byte 2^32
        inside = [ic.big_index(layout, y, x, c) for y in range(r0, r1) for x in (0, ic.BIG_SIDE - 1) for c in (0, 3)]
        assert min(inside) < first < max(inside), layout              # the window's rows hold byte 2^32


# ------------------------------------------------------------------ the witnesses and the model conditions
def test_the_witnesses_tell_two_roundings_from_a_fused_multiply_add():
    x, two, fused = ic.f32_witnesses()
    assert x.size >= 100 and x.dtype == np.float32
    assert np.all(two != fused)
    assert np.array_equal(tiles.to_bytes(x, tiles.SYMMETRIC), two)                     # the model rounds twice
    assert np.float32(-0.9882352948188782) in x and int(two[x == np.float32(-0.9882352948188782)][0]) == 2
    assert np.array_equal(ic.fused_bytes(x), fused)
    P = ic.f32_patterns()
    assert np.isin(x.view(np.uint32), P.view(np.uint32)).all() and P.shape[1:] == (ic.F32_W, 4)
    assert np.isnan(P).any() and np.isinf(P).any() and (P.view(np.uint32) == 0x80000001).any() and (P.view(np.uint32) == 1).any()


@pytest.mark.parametrize("dtype", ic.FLOATS, ids=["f16", "bf16", "f32"])
def test_the_expectations_of_the_values_module_can_fail(dtype):
    from gpu_calls import conditions
    specs, hows = ic.value_specs(dtype)
    offs, _ = ic.offsets(specs, hows)
    assert [o % 256 == 0 for o in offs] == [h == ic.ALIGNED for h in hows] and {h for h in hows} == {ic.ALIGNED, ic.ONE}
    assert {(s[3][1], s[3][2], h) for s, h in zip(specs, hows)} == {(l, r, h) for l in (tiles.HWC, tiles.CHW) for r in ic.RANGES for h in (ic.ALIGNED, ic.ONE)}
    if dtype != tiles.F32:
        assert np.array_equal(np.sort(np.ascontiguousarray(ic.patterns(dtype)).view(np.uint16).reshape(-1)), np.arange(65536))
    conditions(dtype, specs, ic.value_tiles(specs), [tiles.convert(s[4], tiles.source_flags(*s[3])) for s in specs])


def test_a_tile_depends_on_its_rectangle_alone():
    """what part 2 of the wide file rests on: the tile of a rectangle is the tile of the cut-out window at (0, 0)"""
    r = np.random.default_rng(8)
    for layout in (tiles.HWC, tiles.CHW):
        f = tiles.source_flags(tiles.F32, layout, tiles.UNIT)
        A = r.uniform(-0.25, 1.25, size=(23, 37, 4)).astype(np.float32)
        for (x, y, cw, ch) in ((0, 0, 37, 23), (5, 3, 30, 11), (36, 22, 1, 1)):
            for flips in range(4):
                for och in (0, 3):
                    T = A if layout == tiles.HWC else np.ascontiguousarray(np.transpose(A, (2, 0, 1)))
                    W = A[y:y + ch, x:x + cw]
                    W = W if layout == tiles.HWC else np.ascontiguousarray(np.transpose(W, (2, 0, 1)))
                    assert np.array_equal(tiles.tile(T, (0, x, y, cw, ch, 1, f | flips), och), tiles.tile(W, (0, 0, 0, cw, ch, 1, f | flips), och))
