"""qoimi_encode_packed without a GPU: the sub-batch plan (qoi_amd/packplan.py, the normative statement of what the host code computes)
on the cases the contract names, and the two entry points in the header, api.EXPORTS and the Python class (tests/test_abi.py then checks
the built libraries against those by itself)."""
import os
import re

from qoi_amd import packplan
from qoi_amd.packplan import plan, slot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 64 * 48 * 5 + 22                  # the bound of a 64 x 48 RGBA image: 15382
S = 15616                             # ... rounded up to 256


def covers(p, n):
    """every image exactly once, in order, no empty sub-batch"""
    at = 0
    for first, count in p:
        assert first == at and count >= 1, p
        at += count
    assert at == n, p
    return True


def test_slot():
    assert slot(B) == S and slot(256) == 256 and slot(257) == 512 and slot(1) == 256 and slot(23) == 256
    assert packplan.SLOT_ALIGN == 256


def test_exact_fits():
    assert plan([B] * 12, 4 * S) == [(0, 4), (4, 4), (8, 4)]
    assert plan([B] * 12, 12 * S) == [(0, 12)]
    assert plan([B] * 12, 1 * S) == [(i, 1) for i in range(12)]
    assert plan([B] * 12, 4 * S + S - 1) == [(0, 4), (4, 4), (8, 4)]          # a part of a slot holds nothing
    assert plan([B] * 12, 4 * S - 1) == [(0, 3), (3, 3), (6, 3), (9, 3)]      # one byte short of four slots: three


def test_remainder_sub_batch():
    assert plan([B] * 13, 5 * S) == [(0, 5), (5, 5), (10, 3)]
    assert plan([B] * 13, 2 * S) == [(0, 2), (2, 2), (4, 2), (6, 2), (8, 2), (10, 2), (12, 1)]
    assert plan([B] * 13, 100 * S) == [(0, 13)]
    for staging in (1, S, 2 * S, 5 * S, 13 * S, 14 * S):
        p = plan([B] * 13, staging)
        assert covers(p, 13)
        assert [c for _, c in p[:-1]] == [max(1, staging // S)] * (len(p) - 1)    # equal shapes: max(1, staging / slot) images each


def test_request_below_one_slot_is_raised():
    for staging in (0, 1, S - 1):
        assert plan([B] * 5, staging) == [(i, 1) for i in range(5)], staging


def test_one_slot_larger_than_all_the_others():
    small, big = 1 * 1 * 5 + 22, 130 * 70 * 5 + 22
    assert slot(small) == 256 and slot(big) == 45568
    assert plan([small, small, big, small, small, small], 1024) == [(0, 2), (2, 1), (3, 3)]      # the large one alone, its neighbours around it
    assert plan([big, small, small], 512) == [(0, 1), (1, 2)]
    assert plan([small, small, big], 512) == [(0, 2), (2, 1)]


def test_mixed_bounds():
    bounds = [27, 507, 677, 4277, 11587, 15382, 11677, 45522, 36422]          # slots 256 512 768 4352 11776 15616 11776 45568 36608
    assert [slot(b) for b in bounds] == [256, 512, 768, 4352, 11776, 15616, 11776, 45568, 36608]
    assert plan(bounds, 20000) == [(0, 5), (5, 1), (6, 1), (7, 1), (8, 1)]
    assert plan(bounds, 30000) == [(0, 5), (5, 2), (7, 1), (8, 1)]
    assert plan(bounds, 1 << 20) == [(0, 9)]
    for staging in (0, 256, 1000, 5888, 5889, 17664, 45568, 82176):
        p = plan(bounds, staging)
        assert covers(p, len(bounds))
        for first, count in p:
            used = sum(slot(b) for b in bounds[first:first + count])
            assert count == 1 or used <= staging, (staging, p)                 # only a lone image may exceed the request
            if first + count < len(bounds):                                   # ... and a sub-batch closes only when the next slot does not fit
                assert used + slot(bounds[first + count]) > staging, (staging, p)


def test_single_image_and_none():
    assert plan([B], 0) == [(0, 1)] and plan([B], S) == [(0, 1)] and plan([B], 1 << 40) == [(0, 1)]
    assert plan([], 4096) == []


def test_entry_points_in_every_layer():
    from qoi_amd import api
    header = open(os.path.join(ROOT, "include", "qoi_mi355x.h")).read()
    for name in ("qoimi_encode_packed", "qoimi_encode_images_packed"):
        assert name in api.EXPORTS, name
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    for method in ("encode_packed", "encode_images_packed"):
        assert callable(getattr(api.Context, method))
    host = open(os.path.join(ROOT, "qoi_amd", "csrc", "qoi_host.hip")).read()
    for kernel in ("pack_offsets_append", "pack_copy_append"):                # named, so qoimi_get_profile counts the append launches
        assert '"%s"' % kernel in host, kernel
