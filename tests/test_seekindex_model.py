"""The row seek index model (qoi_amd/seekindex.py) against the decoders, on the CPU: for every stream of the classes below, every seek point and
a sample of bands, the band stream decoded AS IT IS by the oracle (our port, and the unmodified reference where it is built) at 3 and at 4
channels gives, from row pad_rows on, exactly the rows of the full decode; band_info says what band_stream builds.  Stream classes: encoder
output with long runs across row boundaries, index-heavy content, 3- and 4-channel images with RGBA chunks, random hostile bodies, a wrong
end marker, streams cut anywhere (down to 22 bytes), a body of 0xFF bytes.  Widths 1, 2, 61 to 65, 127 to 129."""
import numpy as np
import pytest

from qoi_amd import seekindex as si
from model_cases import END, alpha_image, header, index_image, runs_image

WIDTHS = [1, 2, 61, 62, 63, 64, 65, 127, 128, 129]


def intervals(w):
    k = -(-128 // w)
    return [k, 2 * k + 1]


def height(w):
    return 5 * (-(-128 // w)) + 3


def streams_of(oracle, w):
    """(name, stream bytes, channels of the header)"""
    h = height(w)
    out = []
    for ch in (3, 4):
        for name, make in (("runs", runs_image), ("index", index_image), ("alpha", alpha_image)):
            s = oracle.encode(make(w, h, ch, 7 * w + ch), w, h, ch)
            assert s is not None
            out.append((f"{name}{ch}", s, ch))
    rng = np.random.default_rng(w)
    good = out[3][1]                                                        # runs4
    # a 3-channel header over a body with RGBA chunks: alpha changes although the header says 3
    out.append(("rgba_in_3", header(w, h, 3) + out[5][1][14:], 3))
    for k in range(3):
        body = rng.integers(0, 256, size=int(rng.integers(40, 3 * w * h)), dtype=np.uint8).tobytes()
        out.append((f"hostile{k}", header(w, h, 3 + k % 2) + body + END, 3 + k % 2))
    out.append(("runs_only", header(w, h, 4) + bytes(rng.integers(0xC0, 0xFE, size=w * h // 20 + 4, dtype=np.uint8)) + END, 4))
    out.append(("wrong_end", good[:-8] + b"\xee" * 8, 4))
    for cut in sorted({max(22, c) for c in (22, 23, 27, len(good) // 3, len(good) // 2 + 1, len(good) - 9, len(good) - 3)}):
        out.append((f"cut{cut}", good[:cut], 4))
    out.append(("all_ff", header(w, h, 4) + b"\xff" * (w * h + 11) + END, 4))
    out.append(("all_ff_short", header(w, h, 3) + b"\xff" * 203, 3))
    out.append(("no_chunk", header(w, h, 4) + END, 4))
    return h, out


def check_stream(oracle, name, s, w, h, ch):
    full4, d = oracle.decode(s, 4)
    assert full4 is not None and (d.width, d.height, d.channels) == (w, h, ch), name
    full3, _ = oracle.decode(s, 3)
    full = {4: full4.reshape(h, w, 4), 3: full3.reshape(h, w, 3)}
    bands_checked = 0
    for K in intervals(w):
        pts = si.points(s, w, h, K, full4)
        assert len(pts) == si.n_points(w, h, K) == -(-h // K) - 1 and len(pts) >= 1
        assert all(14 <= int(p["byte_off"]) <= len(s) - 8 and int(p["skip"]) <= 61 for p in pts)
        starts = [0] + [(k + 1) * K for k in range(len(pts))]
        for first in starts:
            # to the next seek row, one row, to the image's end, into the middle of a later interval
            for rows in sorted({min(K, h - first), 1, h - first, min(K + K // 2 + 1, h - first)}):
                band, pad = si.band_stream(s, w, h, ch, 0, K, pts, first, rows)
                info = si.band_info(len(s), w, h, ch, 0, K, pts, first, rows)
                assert info == {"size": len(band), "desc": (w, pad + rows, ch, 0), "pad_rows": pad}, (name, K, first, rows)
                assert pad <= K and (pad == 0) == (first == 0)
                for och in (3, 4):
                    got, bd = oracle.decode(band, och)
                    assert got is not None and (bd.width, bd.height, bd.channels) == (w, pad + rows, ch), (name, K, first, rows)
                    got = got.reshape(pad + rows, w, och)[pad:]
                    assert np.array_equal(got, full[och][first:first + rows]), (name, w, K, first, rows, och)
                bands_checked += 1
    return bands_checked


@pytest.mark.parametrize("w", WIDTHS)
def test_bands_decode_to_the_rows_of_the_full_decode(port, ref, w):
    for oracle in [o for o in (port, ref) if o is not None]:
        h, streams = streams_of(port, w)
        total = sum(check_stream(oracle, name, s, w, h, ch) for name, s, ch in streams)
        assert total > 400


def test_points_fall_inside_runs_and_behind_the_chunks(port):
    """the cases above are not all of one kind: points with skip != 0 (61 among them), points behind the last chunk, tails that are only
    the last 8 bytes"""
    w, h, K = 64, 13, 2
    body = b"\xfe\x01\x02\x03" + b"\xfd" * 4 + b"\xc4"                     # 1 + 4 * 62 + 5 = 254 pixels, then nothing
    s = header(w, h, 4) + body + END
    full4, _ = port.decode(s, 4)
    pts = si.points(s, w, h, K, full4)
    assert [int(p["skip"]) for p in pts[:2]] == [128 - 125, 0] and int(pts[0]["byte_off"]) == 14 + 4 + 2
    assert all(int(p["byte_off"]) == len(s) - 8 and int(p["skip"]) == 0 for p in pts[1:])
    assert si.band_stream(s, w, h, 4, 0, K, pts, 4, 3)[0].endswith(b"\xfd\xc0" + END) and si.band_info(len(s), w, h, 4, 0, K, pts, 4, 3)["size"] == 14 + 5 + 2 + 8
    s61 = header(63, 9, 4) + b"\xfd" * 10 + END                             # rows of 63: point 0 at pixel 189 = 3 * 62 + 3, point 1 at 378 = 6 * 62 + 6
    full4, _ = port.decode(s61, 4)
    assert [int(p["skip"]) for p in si.points(s61, 63, 9, 3, full4)] == [3, 6]
    s61 = header(61, 9, 4) + b"\xfd" * 10 + END                             # rows of 61, K = 3: point 0 at 183 = 2 * 62 + 59, point 1 at 366 = 5 * 62 + 56
    full4, _ = port.decode(s61, 4)
    assert [int(p["skip"]) for p in si.points(s61, 61, 9, 3, full4)] == [59, 56]
    s61 = header(123, 5, 4) + b"\xfd" * 10 + END                            # K = 2: point 0 at 246 = 3 * 62 + 60, point 1 at 492 = 7 * 62 + 58; K = 3: 369 = 5 * 62 + 59
    full4, _ = port.decode(s61, 4)
    assert [int(p["skip"]) for p in si.points(s61, 123, 5, 2, full4)] == [60, 58]
    s61 = header(185, 3, 4) + b"\xfd" * 10 + END                            # K = 1: point 0 at 185 = 2 * 62 + 61
    full4, _ = port.decode(s61, 4)
    assert [int(p["skip"]) for p in si.points(s61, 185, 3, 1, full4)] == [61, 60]


def test_the_table_is_the_last_pixel_per_slot(port):
    w, h, K = 16, 40, 8
    px = index_image(w, h, 4, 3)
    s = port.encode(px, w, h, 4)
    full4, _ = port.decode(s, 4)
    pts = si.points(s, w, h, K, full4)
    D = full4.reshape(-1, 4)
    words = D.view("<u4").reshape(-1)
    slots = si.hash_slot(D)
    for k, p in enumerate(pts):
        P = (k + 1) * K * w
        assert int(p["prev"]) == int(words[P - 1])
        for slot in range(64):
            hits = np.flatnonzero(slots[:P] == slot)
            assert int(p["table"][slot]) == (int(words[hits[-1]]) if hits.size else 0)
    assert any(int(v) == 0 for v in pts[-1]["table"])                       # slots never written


def test_bands_for_crops(port):
    w, h, K = 32, 50, 8
    s = port.encode(alpha_image(w, h, 4, 1), w, h, 4)
    full4, _ = port.decode(s, 4)
    pts = si.points(s, w, h, K, full4)
    descs = [(9, 9), (w, h), (w, h)]
    cs = [(1, 3, 20, 5, 7, 0), (1, 0, 17, 32, 2, 3), (2, 0, 0, 1, 1, 0), (2, 1, 49, 1, 1, 1)]
    bands, rebased = si.bands_for_crops(descs, cs, [0, K, 25], [None, pts, si.points(s, w, h, 25, full4)])
    assert bands == [(1, 16, 11), (2, 0, 50)]
    pad = si.pad_rows_of(pts[1], w)
    assert rebased == [(0, 3, 4 + pad, 5, 7, 0), (0, 0, 1 + pad, 32, 2, 3), (1, 0, 0, 1, 1, 0), (1, 1, 49, 1, 1, 1)]
    assert si.bands_for_crops(descs, cs, [0, K, 25]) == (bands, None)
    with pytest.raises(ValueError):
        si.bands_for_crops(descs, cs, [0, 3, 25])                           # 3 * 32 < 128
    assert si.n_points(32, 50, 4) == 12 and si.n_points(32, 48, 8) == 5 and si.n_points(32, 50, 3) == -1 and si.n_points(1, 128, 128) == 0
