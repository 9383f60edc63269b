"""What tests/test_gpu_memory_contract.py stands on, checked without a GPU: the full-slot images of tests/cases.py do fill their slots
(the reference encoder writes exactly qoimi_encode_bound bytes for them), and the guard checks of tests/gpu_util.py (GuardedRegion,
EdgeBatch.check_streams / check_pixels) fire for ONE altered byte wherever it lies - in front of the first slot, in the gap between
two slots, between a stream's end and its slot's bound, behind the last slot - and stay silent on an untouched buffer: the mask
arithmetic is tested on host arrays, not by running a wrong kernel."""
import numpy as np
import pytest

import cases
from gpu_util import GUARD, OUT_FILL, STREAM_FILL, EdgeBatch, GuardedRegion
from qoi_amd import api, synth
from gpu_pack import oracle  # noqa: F401  (fixtures)


@pytest.mark.parametrize("ch", [4, 3])
def test_full_slot_images_fill_their_slot(oracle, ch):
    for (w, h) in [(1, 1), (7, 3), (1023, 1), (1025, 3), (64, 9), (517, 313), (1024, 16)]:
        for seed in (0, 1, 2):
            f = cases.full_slot_image(w, h, ch, seed)
            assert f.shape == (h, w, ch) and f.dtype == np.uint8
            assert len(oracle.encode(f, w, h, ch)) == w * h * (ch + 1) + 22 == api.encode_bound(w, h, ch), (w, h, ch, seed)


def host_batch(oracle, ds):
    """three 7 x 3 RGBA images - full slot, constant, full slot - laid out as EdgeBatch lays them out, as the device would leave them"""
    b = EdgeBatch(None, 7, 3, 4, 3, po=3, so=5, oo=9, dp=0, ds=ds)
    frames = [cases.full_slot_image(7, 3, 4, 0), synth.frame_rgba("constant", 7, 3, 1), cases.full_slot_image(7, 3, 4, 2)]
    want = [oracle.encode(f, 7, 3, 4) for f in frames]
    assert len(want[0]) == b.bound == len(want[2]) and len(want[1]) < b.bound - 8
    host = np.full(b.sreg.size, STREAM_FILL, dtype=np.uint8)
    for s, at in zip(want, b.sreg.starts):
        host[at:at + len(s)] = np.frombuffer(s, dtype=np.uint8)
    return b, want, host


@pytest.mark.parametrize("ds", [0, 7])
def test_stream_guards_bite(oracle, ds):
    b, want, host = host_batch(oracle, ds)
    lens = [len(s) for s in want]
    assert b.sreg.size == GUARD + 5 + 3 * (b.bound + ds) + GUARD and b.sreg.starts[0] == GUARD + 5
    b.check_streams(host, lens, want, "untouched")                           # silent on what a correct library leaves
    s0, s1, s2 = b.sreg.starts
    spots = {
        "first byte of the buffer": (0, "outside the slots"),
        "the byte in front of slot 0": (s0 - 1, "outside the slots"),
        "the byte behind stream 1": (s1 + lens[1], "behind a stream"),
        "the last byte of slot 1's bound": (s1 + b.bound - 1, "behind a stream"),
        "the byte behind the last slot's bound": (s2 + b.bound, "outside the slots"),
        "the last byte of the buffer": (b.sreg.size - 1, "outside the slots"),
    }
    if ds:
        spots["the first byte of the gap behind slot 0"] = (s0 + b.bound, "outside the slots")
        spots["the last byte of the gap behind slot 1"] = (s2 - 1, "outside the slots")
        spots["the last byte of the gap behind slot 2"] = (s2 + b.bound + ds - 1, "outside the slots")
    for name, (k, level) in spots.items():
        for value in (0x00, STREAM_FILL ^ 1):
            bad = host.copy()
            assert bad[k] == STREAM_FILL, name
            bad[k] = value
            with pytest.raises(AssertionError, match=level):
                b.check_streams(bad, lens, want, name)
    # a byte altered inside a stream, a length off by one
    bad = host.copy(); bad[s0 + b.bound - 1] ^= 0x40                         # the full slot's last byte (the end marker's 0x01)
    with pytest.raises(AssertionError, match="differs from the reference"):
        b.check_streams(bad, lens, want, "last byte of a full slot")
    with pytest.raises(AssertionError):
        b.check_streams(host, [lens[0], lens[1] + 1, lens[2]], want, "length")


def test_pixel_guards_bite():
    b = EdgeBatch(None, 7, 3, 3, 3, po=3, so=5, oo=9)
    for och in (3, 4):
        region = GuardedRegion.strided(GUARD + b.oo, b.npx * och, b.n, OUT_FILL)         # EdgeBatch.decode's layout: images back to back
        want = [np.random.default_rng(i).integers(0, 256, size=b.npx * och, dtype=np.uint8) for i in range(3)]
        host = np.full(region.size, OUT_FILL, dtype=np.uint8)
        for px, at in zip(want, region.starts):
            host[at:at + px.size] = px
        b.check_pixels(host, region, want, "untouched")
        for k in (0, region.starts[0] - 1, region.starts[2] + b.npx * och, region.size - 1):
            bad = host.copy(); bad[k] = 0x11
            with pytest.raises(AssertionError, match="around the images"):
                b.check_pixels(bad, region, want, "guard")
        bad = host.copy(); bad[region.starts[1]] ^= 1                                    # image 1's first byte = the byte behind image 0
        with pytest.raises(AssertionError, match="image 1 differs"):
            b.check_pixels(bad, region, want, "pixel")


def test_region_with_free_offsets():
    """slots wherever the caller put them (qoimi_encode_images, a pack): back to back, and in any order"""
    r = GuardedRegion(200, [70, 64, 100], 0xEE)
    host = np.full(200, 0xEE, dtype=np.uint8)
    host[64:70] = 1; host[70:100] = 2; host[100:130] = 3
    r.assert_untouched(host, [30, 6, 30], "back to back")
    with pytest.raises(AssertionError, match="1 bytes written outside their range, the first at byte 129 .*0 bytes behind the 29 writable bytes of slot 2"):
        r.assert_untouched(host, [30, 6, 29], "one byte too many")
    with pytest.raises(AssertionError, match="1 bytes in front of the first slot"):
        bad = host.copy(); bad[63] = 0
        r.assert_untouched(bad, [30, 6, 30], "in front")
    with pytest.raises(AssertionError):
        r.assert_untouched(host[:199], [30, 6, 30], "not the whole buffer")
