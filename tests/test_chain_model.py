"""tests/chain_model.py against the reference decoder, and the certificates of tests/test_gpu_line_reader_hostile.py: that every
stream of that module reaches, by the model's conservative verdicts, the code its case is named after - proved here on the CPU."""
import math

import numpy as np
import pytest

import chain_model as cm
from gpu_pack import oracle  # noqa: F401  (fixtures)

SEGS = [1024, 2048, 4096]


def _not_flat(case):
    for k, (kind, (s, w, h)) in enumerate(case):
        assert (len(s) - cm.TRAILER) * 8 >= w * h, f"stream {k} ({kind}) is flat: {len(s)} bytes for {w * h} pixels"


def _three_per_wave(case, B):
    per = cm.wave_images([cm.n_segments(it[0], B) for _, it in case])
    assert min(per) >= 3, f"images per wavefront {per}"
    assert 5 <= len(case) <= 64


def test_len_of_is_the_decoders_chunk_length():
    for tag in range(256):
        want = 4 if tag == 0xFE else 5 if tag == 0xFF else 2 if 0x80 <= tag < 0xC0 else 1
        assert cm.len_of(tag) == want
    assert [cm.pixels_of(t) for t in (0x00, 0x7F, 0xBF, 0xC0, 0xFD, 0xFE, 0xFF)] == [1, 1, 1, 1, 62, 1, 1]


@pytest.mark.parametrize("sprite", [False, True])
def test_walk_lands_on_the_end_marker_of_encoder_made_streams(oracle, sprite):
    """from byte 14 the model's chain lands exactly on len - 8 and counts w * h pixels; entry() from there agrees with it"""
    for B, nseg, seed in [(1024, 10, 1), (2048, 9, 2), (4096, 8, 3), (1024, 30, 4)]:
        s, w, h = cm.clean(oracle, B, nseg, seed=seed, sprite=sprite)
        starts, land, npx = cm.walk(s)
        assert land == len(s) - cm.TRAILER, (B, nseg, land, len(s))
        assert npx == w * h, (B, nseg, npx, w * h)
        px, d = oracle.decode(s, 4)
        assert (d.width, d.height) == (w, h) and px.size == npx * 4
        at = set(starts)
        for j in range(1, nseg):
            assert cm.entry(s, cm.HEADER, cm.HEADER + j * B) in at


def test_model_pixels_equal_the_decoders_on_any_bytes(oracle):
    """random bytes are chunks too: a header that asks for the model's pixel count plus five gets the last pixel five times more"""
    rng = np.random.default_rng(5)
    for n in (1, 7, 300, 5000):
        s, w, h = cm.by_pixels(rng.integers(0, 256, n, dtype=np.uint8).tobytes(), extra=5)
        px, _ = oracle.decode(s, 4)
        px = px.reshape(-1, 4)
        assert px.shape[0] == w * h
        assert (px[-6:] == px[-6]).all()
        short, _ = oracle.decode(cm._stream(w - 5, 1, s[cm.HEADER:-cm.TRAILER]), 4)
        assert np.array_equal(short, px[:-5].reshape(-1))


@pytest.mark.parametrize("B", SEGS)
def test_clean_streams_meet_in_the_first_run_up(oracle, B):
    """encoder-made content: no segment is certified apart at 64 bytes (the GPU cases ask for no fallback there; that is measured)"""
    n = 0
    for kind, (s, _, _) in cm.retry_case(oracle, B):
        if kind == "c":
            v = cm.verdicts(s, B)
            assert all(a == "meets" for a, _ in v), [a for a, _ in v]
            n += len(v)
    assert n == 128


@pytest.mark.parametrize("B", SEGS)
def test_retry_streams_need_the_second_run_up_and_get_through_it(oracle, B):
    case = cm.retry_case(oracle, B)
    assert [k for k, _ in case] == list("crcrcrcrcrcrc")
    _not_flat(case)
    _three_per_wave(case, B)
    _three_per_wave([c for c in case if c[0] == "c"], B)          # the clean streams alone, as the case runs them first
    for k, (kind, (s, w, h)) in enumerate(case):
        nseg = cm.n_segments(s, B)
        assert 8 <= nseg <= 30 and 10 * 1024 <= len(s) <= 100 * 1024, (k, nseg, len(s))
        if kind != "r":
            continue
        assert cm.walk(s)[1:] == (len(s) - cm.TRAILER, w * h)
        v = cm.verdicts(s, B)
        apart64 = sum(1 for a, _ in v if a == "apart")
        meets192 = sum(1 for _, b in v[1:] if b == "meets")
        assert apart64 * 4 >= nseg, f"stream {k}: {apart64} of {nseg} segments certified apart at 64 bytes"
        assert meets192 == nseg - 1, f"stream {k}: {meets192} of {nseg - 1} segments certified to meet at 192 bytes: {v}"


@pytest.mark.parametrize("B", SEGS)
def test_never_meeting_streams_fail_both_run_ups(oracle, B):
    for case in (cm.never_case(oracle, B), cm.mixed_case(oracle, B)):
        _not_flat(case)
        _three_per_wave(case, B)
        for k, (kind, (s, w, h)) in enumerate(case):
            if kind != "h":
                continue
            assert 60 * 1024 - 5 <= len(s) <= 60 * 1024
            nseg = cm.n_segments(s, B)
            both, at192 = cm.count_apart(s, B)
            assert both == at192, (both, at192)
            assert both * 2 >= nseg, f"stream {k}: {both} of {nseg} segments certified apart at 64 and 192 bytes"
            assert both == nseg - 1, (both, nseg)                 # (all but the one the stream's first chunk is in reach of)
    assert {k for k, _ in cm.mixed_case(oracle, B)} == {"c", "r", "h"}
    for kind, (s, _, _) in cm.mixed_case(oracle, B):
        if kind == "r":
            v = cm.verdicts(s, B)
            assert sum(1 for a, _ in v if a == "apart") * 4 >= len(v) and all(b == "meets" for _, b in v[1:])


@pytest.mark.parametrize("B", SEGS)
def test_phase_streams_straddle_every_line_and_segment_end(oracle, B):
    """over the call - first stream at address 1 of an aligned buffer, an odd stride - a chunk of each of the lengths 2, 4 and 5 begins
    at every distance 1 .. len - 1 in front of a 128-byte line end, and in front of a segment end"""
    case = cm.phase_case(oracle, B)
    _not_flat(case)
    _three_per_wave(case, B)
    assert sum(1 for k, _ in case if k == "p") == 14 and all(len(cm.walk(it[0])[0]) == 3000 for k, it in case if k == "p")
    streams = [it[0] for _, it in case]
    stride = cm.phase_stride(streams)
    line, seg = cm.straddles(streams, [1 + i * stride for i in range(len(streams))], B)
    assert cm.ALL_STRADDLES <= line, f"line ends: missing {sorted(cm.ALL_STRADDLES - line)}"
    assert cm.ALL_STRADDLES <= seg, f"segment ends at {B}: missing {sorted(cm.ALL_STRADDLES - seg)}"
    tags = set()
    for s in streams:
        tags |= {s[p] >> 6 if s[p] < 0xFE else s[p] for p in cm.walk(s)[0]}
    assert tags == {0, 1, 2, 3, 0xFE, 0xFF}                          # INDEX, DIFF, LUMA, RUN, RGB, RGBA


@pytest.mark.parametrize("where", list(cm.END_LANES))
@pytest.mark.parametrize("B", SEGS)
def test_ends_fall_on_the_lane_they_are_sized_for(oracle, B, where):
    case, cuts = cm.ends_case(oracle, B, where)
    _not_flat(case)
    _three_per_wave(case, B)
    nsegs = [cm.n_segments(it[0], B) for _, it in case]
    assert [case[i][0] for i, _ in cuts] == ["x1", "x2", "x3", "x4", "xl", "xa", "xs"]
    for i, crit in cuts:
        assert (sum(nsegs[:i]) + crit) % cm.WAVE == cm.END_LANES[where], (i, case[i][0])
        assert case[i - 1][0] == "c" and (i + 1 == len(case) or case[i + 1][0] == "c")
    for i, crit in cuts[:5]:                                          # the cut chunk begins in the stream's last segment, its tail is the end marker's
        s = case[i][1][0]
        starts, land, _ = cm.walk(s)
        assert land > len(s) - cm.TRAILER and (starts[-1] - cm.HEADER) // B == crit == nsegs[i] - 1, (i, land, len(s))
    xs = case[cuts[6][0]][1]
    assert math.isclose(cm.walk(xs[0])[2] / (xs[1] * xs[2]), 0.03, rel_tol=0.01)
    xa = case[cuts[5][0]][1]
    assert cm.walk(xa[0])[2] > xa[1] * xa[2] and cm.walk(xa[0])[1] == len(xa[0]) - cm.TRAILER


@pytest.mark.parametrize("B", SEGS)
def test_sub_batch_calls_split_in_three_or_more(oracle, B):
    for name, case in (("retry", cm.retry_case(oracle, B)), ("never", cm.never_case(oracle, B))):
        rep = cm.repeats_for_sub_batches([len(it[0]) for _, it in case], B)
        lens = [len(it[0]) for _, it in case] * rep
        assert len(lens) <= 64
        parts = cm.sub_batches(lens, B)
        assert len(parts) >= 3 and sum(parts) == len(lens), f"{name} at {B}: sub-batches of {parts} images"


@pytest.mark.parametrize("B", SEGS)
def test_overlap_pair_is_two_streams_in_one_range(oracle, B):
    (s, w, h), (t, tw, th), off = cm.overlap_pair(oracle, B)
    assert s[off:off + len(t)] == t and off + len(t) < len(s) - cm.TRAILER
    assert cm.walk(s)[2] == w * h and (len(s) - cm.TRAILER) * 8 >= w * h
    assert 8 <= cm.n_segments(s, B) <= 30 and cm.n_segments(t, B) == 8
    assert oracle.decode(s, 4)[0].size == w * h * 4 and oracle.decode(t, 4)[0].size == tw * th * 4
