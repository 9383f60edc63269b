"""qoi_amd/seekindex.py: points_from_pixels - the normative statement of qoimi_seek_index_from_pixels - on the CPU: for oracle-encoded images it
equals points over the oracle's decode of the stream (3- and 4-channel images; runs across rows, noise, flat; widths 1 and 63 to 65); for a
stream that does not decode to the pixels, byte_off and skip follow the stream, prev and table the pixels."""
import numpy as np
import pytest

from qoi_amd import seekindex as si
from model_cases import alpha_image, index_image, runs_image


def flat_image(w, h, ch, seed):
    return np.full((w * h, ch), 7 + seed % 200, dtype=np.uint8)


IMAGES = [(w, h, K) for w, h, K in [(1, 400, 128), (63, 20, 3), (64, 20, 3), (65, 20, 3), (129, 40, 16), (96, 17, 2)]]


@pytest.mark.parametrize("ch", [3, 4])
@pytest.mark.parametrize("make", [runs_image, alpha_image, flat_image, index_image], ids=["runs", "noise", "flat", "index"])
def test_equals_points_over_the_decode(port, ref, ch, make):
    for oracle in [o for o in (port, ref) if o is not None]:
        for w, h, K in IMAGES:
            px = make(w, h, ch, 3 * w + ch)
            s = oracle.encode(px, w, h, ch)
            full4, d = oracle.decode(s, 4)
            assert (d.width, d.height, d.channels) == (w, h, ch) and np.array_equal(full4.reshape(-1, 4)[:, :ch], px)
            want = si.points(s, w, h, K, full4)
            got = si.points_from_pixels(s, w, h, K, px, ch)
            assert len(got) == si.n_points(w, h, K) >= 1 and got.tobytes() == want.tobytes(), (w, h, K, ch)
            # any shape of the pixel array will do
            assert si.points_from_pixels(s, w, h, K, px.reshape(h, w, ch), ch).tobytes() == want.tobytes()
            if ch == 3:
                assert all(int(p["prev"]) >> 24 == 255 and all(int(v) == 0 or int(v) >> 24 == 255 for v in p["table"]) for p in got)


def test_runs_cross_the_seek_rows(port):
    w, h, K, ch = 64, 20, 3, 4
    px = runs_image(w, h, ch, 5)
    s = port.encode(px, w, h, ch)
    got = si.points_from_pixels(s, w, h, K, px, ch)
    assert any(int(p["skip"]) != 0 for p in got)


@pytest.mark.parametrize("ch", [3, 4])
def test_a_stream_of_other_pixels(port, ch):
    """the stream of image A with the pixels of image B: byte_off / skip are those of A's index, prev / table those of B's"""
    w, h, K = 65, 20, 3
    a, b = runs_image(w, h, ch, 1), alpha_image(w, h, ch, 2)
    sa, sb = port.encode(a, w, h, ch), port.encode(b, w, h, ch)
    pa, pb = si.points_from_pixels(sa, w, h, K, a, ch), si.points_from_pixels(sb, w, h, K, b, ch)
    mixed = si.points_from_pixels(sa, w, h, K, b, ch)
    for f in ("byte_off", "skip"):
        assert np.array_equal(mixed[f], pa[f]) and not np.array_equal(pa[f], pb[f])
    for f in ("prev", "table"):
        assert np.array_equal(mixed[f], pb[f]) and not np.array_equal(pa[f], pb[f])
    assert all(14 <= int(p["byte_off"]) <= len(sa) - 8 and int(p["skip"]) <= 61 for p in mixed)
    with pytest.raises(ValueError):
        si.points_from_pixels(sa, w, h, K, a[:, :2], 2)
