"""The host plans of the calls that work through bounded staging (qoi_amd/csrc/qoi_stage_plan.h: pack_plan, stage_plan, plan_rows, plan_items,
ranges_overlap) compiled with g++ (tests/host/plan_host.cpp) and compared on the CPU with their Python statements: qoi_amd/packplan.py: plan
for the sub-batches, qoi_amd/crops.py: plan for the rows.  The order of the table entries and their tiles, and the overlap check, are held
to what defines them.  The same source is built as a stand-alone program with the address and undefined-behaviour sanitizers and run (a
program of its own: nothing sanitized is loaded into this process)."""
import ctypes

import pytest

import hostbuild
from qoi_amd import crops, packplan

SRC = "plan_host.cpp"
DEFAULT = 1 << 30
ONE = 64 * 48 * 4                                   # the slot of the GPU suites' 13 equal images
EQUAL = [ONE] * 13
MIXED = [256, 24832, 512, 3328, 9472, 9216, 9472, 37120, 256]   # 37120: larger than any request below but 13 * ONE
LIMIT = 0x7FFFFFFF

u32, u64, ci = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int


def arr(t, values):
    return (t * max(len(values), 1))(*values)


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    P = ctypes.POINTER
    return hostbuild.shared(SRC, tmp_path_factory, {
        "plan_host_up256": (u64, [u64]),
        "plan_host_pack": (ci, [P(u64), ci, u64, P(ci)]),
        "plan_host_stage": (ci, [P(u64), ci, u64, P(ci), P(u64), P(u64)]),
        "plan_host_rows": (ci, [P(u32), ci, P(u32), u64, P(ci), P(ci), P(u64), P(ci), P(ci), P(u64), P(u64)]),
        "plan_host_items": (ci, [P(u32), ci, P(ci), ci, P(ci), ci, P(u64), P(u64), P(u32), P(u32), P(u32), P(u32)]),
        "plan_host_overlap": (ci, [P(u64), P(u64), ci])})


def stage(lib, slots, staging):
    """(firsts, at, need) of stage_plan"""
    n = len(slots)
    firsts, at, need = (ci * (n + 1))(), (u64 * max(n, 1))(), u64()
    k = lib.plan_host_stage(arr(u64, slots), n, staging, firsts, at, ctypes.byref(need))
    return list(firsts[:k]), list(at[:n]), need.value


def rows_plan(lib, widths, rows, staging):
    """(refs, ref_of, slots, firsts, at, need) of plan_rows"""
    n = len(widths)
    refs, ref_of, slots, firsts, at = (ci * n)(), (ci * n)(), (u64 * n)(), (ci * (n + 1))(), (u64 * n)()
    nf, need = ci(), u64()
    nr = lib.plan_host_rows(arr(u32, widths), n, arr(u32, rows), staging, refs, ref_of, slots, firsts, ctypes.byref(nf), at, ctypes.byref(need))
    return list(refs[:nr]), list(ref_of[:n]), list(slots[:nr]), list(firsts[:nf.value]), list(at[:nr]), need.value


def items_plan(lib, image_of, ref_of, firsts, tiles_of):
    """None if plan_items reports an overflow, else (by_ref, first_tile, [(entry, m, tiles)])"""
    n, k = len(image_of), len(firsts) - 1
    by_ref, first_tile, entry, m, tiles = (u64 * n)(), (u32 * n)(), (u32 * k)(), (u32 * k)(), (u32 * k)()
    if lib.plan_host_items(arr(u32, image_of), n, arr(ci, ref_of), len(ref_of), arr(ci, firsts), len(firsts), arr(u64, tiles_of),
                           by_ref, first_tile, entry, m, tiles):
        return None
    return list(by_ref), list(first_tile), list(zip(entry, m, tiles))


@pytest.mark.parametrize("slots", [EQUAL, MIXED], ids=["equal", "mixed"])
def test_sub_batch_plan(host_lib, slots):
    """pack_plan and stage_plan against packplan.plan: firsts, every at[i] and need; 0 is the default for stage_plan alone"""
    assert max(MIXED) > 3 * ONE + 1 and all(host_lib.plan_host_up256(s - 255) == s == packplan.slot(s - 255) for s in slots)
    for staging in (ONE, 3 * ONE, 3 * ONE + 1, 13 * ONE, 0, 1):
        want = packplan.plan(slots, staging if staging else DEFAULT)
        want_firsts = [first for first, _ in want] + [len(slots)]
        want_at = [sum(slots[first:i]) for first, count in want for i in range(first, first + count)]
        firsts, at, need = stage(host_lib, slots, staging)
        assert firsts == want_firsts and at == want_at, staging
        assert need == max(sum(slots[first:first + count]) for first, count in want), staging
        if staging:
            got = (ci * (len(slots) + 1))()
            k = host_lib.plan_host_pack(arr(u64, slots), len(slots), staging, got)
            assert list(got[:k]) == want_firsts, staging
    assert [len(stage(host_lib, EQUAL, s)[0]) - 1 for s in (ONE, 3 * ONE, 3 * ONE + 1, 13 * ONE, 0, 1)] == [13, 5, 5, 1, 1, 13]


def test_rows_plan(host_lib):
    """plan_rows against crops.plan: items that name images out of order, an image named by several items, unreferenced images between
    referenced ones (and in front of the first)"""
    shapes = [(9, 5), (64, 48), (7, 7), (131, 1), (9, 9), (1, 97), (333, 7), (64, 48)]
    cs = [(6, 0, 0, 333, 7, 0), (5, 0, 90, 1, 7, 0), (1, 3, 2, 16, 10, 0), (5, 0, 0, 1, 40, 0), (3, 100, 0, 31, 1, 0), (1, 0, 30, 64, 18, 0), (7, 1, 1, 2, 2, 0)]
    needed = crops.rows_needed(shapes, cs)
    assert list(needed) == [1, 3, 5, 6, 7] and needed[1] == 48 and needed[5] == 97 and needed[7] == 3
    rows = [needed.get(i, 0) for i in range(len(shapes))]
    seen = set()
    for staging in (0, 1, 12288, 13000, 13056, 22528, 40000):
        images, slots, subs, largest = crops.plan(shapes, cs, staging)
        refs, ref_of, got_slots, firsts, at, need = rows_plan(host_lib, [w for w, _ in shapes], rows, staging)
        assert refs == images and got_slots == slots and need == largest, staging
        assert ref_of == [images.index(i) if i in images else -1 for i in range(len(shapes))]
        assert firsts == [first for first, _ in subs] + [len(images)], staging
        assert at == [sum(slots[first:r]) for first, count in subs for r in range(first, first + count)], staging
        seen.add(len(subs))
    assert seen >= {1, 2, 5}


def check_items(lib, image_of, ref_of, firsts, tiles_of):
    got = items_plan(lib, image_of, ref_of, firsts, tiles_of)
    assert got is not None
    by_ref, first_tile, subs = got
    assert sorted(by_ref) == list(range(len(image_of))) and len(subs) == len(firsts) - 1
    e = 0
    for k, (entry, m, tiles) in enumerate(subs):
        assert entry == e                                                     # the entries of a sub-batch are contiguous ...
        mine = [j for j in range(len(image_of)) if firsts[k] <= ref_of[image_of[j]] < firsts[k + 1]]
        assert sorted(by_ref[e:e + m], key=lambda j: ref_of[image_of[j]]) == by_ref[e:e + m]
        assert sorted(by_ref[e:e + m]) == mine                                # ... and hold exactly its items,
        for r in set(ref_of[image_of[j]] for j in mine):                      # those of one image in the caller's order
            of_r = [j for j in by_ref[e:e + m] if ref_of[image_of[j]] == r]
            assert of_r == sorted(of_r)
        t = 0
        for x in range(e, e + m):
            assert first_tile[x] == t                                         # from 0 in each sub-batch, the running sum
            t += tiles_of[by_ref[x]]
        assert tiles == t
        e += m
    assert e == len(image_of)
    return by_ref, first_tile, subs


def test_item_assignment(host_lib):
    widths, rows = [64, 7, 131, 9, 1, 333], [48, 0, 1, 0, 97, 7]
    image_of, tiles_of = [5, 4, 0, 4, 2, 0, 5, 2, 4], [3, 1, 4, 1, 5, 9, 2, 6, 5]
    counts = set()
    for staging in (0, 1, 12288, 13000, 13056, 40000):
        refs, ref_of, _, firsts, _, _ = rows_plan(host_lib, widths, rows, staging)
        by_ref, _, subs = check_items(host_lib, image_of, ref_of, firsts, tiles_of)
        assert by_ref == sorted(range(len(image_of)), key=lambda j: ref_of[image_of[j]])      # (sorted is stable)
        counts.add(len(subs))
    assert counts >= {1, 2, 4}


def test_item_assignment_of_the_identity_map(host_lib):
    """qoimi_decode_thumbnails: item j names image j and every image is referenced - entry == firsts[k], m == firsts[k + 1] - firsts[k]"""
    for slots in (EQUAL, MIXED):
        n = len(slots)
        for staging in (ONE, 3 * ONE, 3 * ONE + 1, 13 * ONE, 0, 1):
            firsts, _, _ = stage(host_lib, slots, staging)
            tiles_of = [1 + (7 * j) % 5 for j in range(n)]
            by_ref, first_tile, subs = check_items(host_lib, list(range(n)), list(range(n)), firsts, tiles_of)
            assert by_ref == list(range(n))
            assert [(entry, m) for entry, m, _ in subs] == [(firsts[k], firsts[k + 1] - firsts[k]) for k in range(len(firsts) - 1)]


def test_tile_overflow(host_lib):
    """reported when the running sum of a sub-batch reaches 0x7FFFFFFF and not one item earlier; synthetic counts, no memory"""
    ident, firsts = [0, 1, 2, 3], [0, 3, 4]
    plan = lambda tiles_of: items_plan(host_lib, ident, ident, firsts, tiles_of)
    assert plan([LIMIT - 9, 4, 4, LIMIT - 1]) == ([0, 1, 2, 3], [0, LIMIT - 9, LIMIT - 5, 0], [(0, 3, LIMIT - 1), (3, 1, LIMIT - 1)])
    assert plan([LIMIT - 9, 4, 5, 1]) is None                  # reached by the sub-batch's last item
    assert plan([LIMIT - 9, 9, 1, 1]) is None                  # reached before its last item
    assert plan([LIMIT - 9, 8, 0, 1]) is not None              # (a count of 0 is synthetic too: one below the limit stays one below)
    assert plan([1, 1, 1, LIMIT]) is None                      # the second sub-batch
    assert plan([LIMIT - 1, 0, 0, LIMIT - 1]) is not None
    assert plan([2 ** 40, 1, 1, 1]) is None


def test_ranges_overlap(host_lib):
    top = 2 ** 64 - 1                                           # SIZE_MAX
    overlap = lambda offsets, sizes: bool(host_lib.plan_host_overlap(arr(u64, offsets), arr(u64, sizes), len(offsets)))
    assert not overlap([0, 40, 100], [40, 60, 28])              # touching
    assert overlap([0, 40, 100], [41, 60, 28])                  # one byte
    assert overlap([0, 40, 100], [40, 61, 28])
    assert not overlap([100, 0, 40], [28, 40, 60])              # unsorted
    assert overlap([100, 0, 40], [28, 41, 60]) and overlap([100, 0, 40], [28, 40, 61]) and overlap([100, 0, 40], [28, 101, 1])
    assert not overlap([5], [top - 5]) and not overlap([top], [0])   # n = 1
    assert overlap([7, 7], [1, 1]) and not overlap([7, 7], [0, 0])
    # near SIZE_MAX: subtracted in the order given, top - 15 from 16 would wrap to 32 and hide the overlap
    assert not overlap([top - 15, 16], [15, top - 31])
    assert overlap([top - 15, 16], [15, top - 30])
    assert overlap([top - 15, top - 20], [15, 6]) and not overlap([top - 15, top - 20], [15, 5])


def test_sanitized_stand_alone_program(tmp_path):
    assert hostbuild.sanitized(SRC, "PLAN_HOST_MAIN", tmp_path) == "plan_host: 2001 plans ok\n"
