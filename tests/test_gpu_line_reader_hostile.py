"""The batch transcoder's line reader (dec_transcode<2>, LineReaderT in qoi_decode.hip) on streams that defeat its run-up - the
companion of tests/test_transcode_line_fetch.py, whose streams all synchronise in the first 64 bytes.  Here: streams that need the
second run-up (every other lane of the wavefront then restarts its reader where it stands), streams whose chains never meet (the
lane is redone by the plain parse while its 63 neighbours go on through the line reader), every chunk length across every line and
segment end, streams that end inside a chunk / carry chunks past their last pixel / end after 3 % of their pixels, and the entry
through qoimi_decode_images (tight, shuffled, repeated and overlapping packs) and through sub-batches.

Every call holds five images or more (the batch path), runs at 1 KiB, 2 KiB and 4 KiB segments (the `segments` counter proves it:
a flat image would leave the forced size) and is compared byte for byte with the reference decoder, a guard behind every image.
The streams come from tests/chain_model.py; tests/test_chain_model.py certifies on the CPU what each of them reaches."""
import os

import numpy as np
import pytest

import chain_model as cm
from gpu_pack import api, lctx, oracle  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

GUARD = 16
_WANT = {}


@pytest.fixture
def seg(request, lctx):  # noqa: F811
    """the segment size `lctx` was created with"""
    return int(request.node.callspec.params["lctx"])


def _want(oracle, case, och):  # noqa: F811
    """the reference decoder's pixels of a case's streams: computed once per stream, shared, never written to"""
    out = []
    for _, (s, w, h) in case:
        key = (s, och)
        if key not in _WANT:
            a = oracle.decode(s, och)[0]
            assert a is not None and a.size == w * h * och
            a.setflags(write=False)
            _WANT[key] = a
        out.append(_WANT[key])
    return out


def _sized(case, B):
    """five images or more, 64 at most, and every wavefront (64 consecutive segments) holds segments of three images or more"""
    per = cm.wave_images([cm.n_segments(it[0], B) for _, it in case])
    assert 5 <= len(case) <= 64 and min(per) >= 3, (len(case), per)


def _strided(case, lead=0, odd=False):
    stride = (max(len(it[0]) for _, it in case) + 15) // 16 * 16 + (1 if odd else 0)
    return [lead + i * stride for i in range(len(case))]


def _run_at(api, ctx, B, case, want, och, soffs, via="batch", listed=None):  # noqa: F811
    """stream i of `case` at byte soffs[i] of one buffer, the images `listed` (default: all, in order) decoded in ONE call - through
    decode_batch (`soffs` a constant stride apart) or decode_images; pixels against `want`, the guard behind every image, the call's
    segment count.  Returns sync_fallback_segments."""
    import torch
    listed = list(range(len(case))) if listed is None else listed
    streams = [it[0] for _, it in case]
    host = np.zeros(max(o + len(s) for o, s in zip(soffs, streams)) + 256, dtype=np.uint8)
    for o, s in zip(soffs, streams):
        host[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
    buf = torch.from_numpy(host).cuda()
    pstride = max(want[i].size for i in listed) + GUARD
    out = torch.full((len(listed) * pstride,), 0xAB, dtype=torch.uint8, device="cuda")
    sizes = [len(streams[i]) for i in listed]
    descs = [api.QoiDesc(case[i][1][1], case[i][1][2], 4, 0) for i in listed]
    if via == "batch":
        stride = soffs[1] - soffs[0]
        assert listed == list(range(len(case))) and all(soffs[i] == soffs[0] + i * stride for i in listed)
        ctx.decode_batch(buf.data_ptr() + soffs[0], stride, sizes, descs, och, out.data_ptr(), pstride)
    else:
        ctx.decode_images(buf.data_ptr(), [soffs[i] for i in listed], sizes, descs, och, out.data_ptr(), [k * pstride for k in range(len(listed))])
    got = out.cpu().numpy()
    for k, i in enumerate(listed):
        g = got[k * pstride:k * pstride + want[i].size]
        if not np.array_equal(g, want[i]):
            bad = int(np.argmax(g != want[i]))
            raise AssertionError(f"image {k} (stream {i}, kind {case[i][0]}, {sizes[k]} bytes, {cm.n_segments(streams[i], B)} segments): first differing byte {bad} of {g.size}")
        assert (got[k * pstride + want[i].size:(k + 1) * pstride] == 0xAB).all(), ("wrote behind image", k, i)
    st = ctx.decode_stats()
    assert st["segments"] == sum(cm.n_segments(streams[i], B) for i in listed), "the call did not run at the forced segment size"
    return st["sync_fallback_segments"]


@pytest.mark.parametrize("och", [4, 3])
def test_second_run_up_beside_innocent_lanes(api, lctx, seg, oracle, och):  # noqa: F811
    """clean, retry, clean, retry ... clean: the retry streams (a meeting place every 121 bytes) fail the 64-byte run-up in a quarter of
    their segments or more and pass the 192-byte one in all (test_chain_model.py); the clean lanes beside them restart where they stand"""
    case = cm.retry_case(oracle, seg)
    clean = [c for c in case if c[0] == "c"]
    _sized(case, seg)
    _sized(clean, seg)
    assert _run_at(api, lctx, seg, clean, _want(oracle, clean, och), och, _strided(clean)) == 0
    assert _run_at(api, lctx, seg, case, _want(oracle, case, och), och, _strided(case)) == 0


def _never_bounds(case, B):
    certified = sum(cm.count_apart(it[0], B)[0] for kind, it in case if kind == "h")
    most = sum(cm.n_segments(it[0], B) for kind, it in case if kind == "h")
    assert certified * 2 >= most
    return certified, most


def test_never_meeting_beside_innocent_lanes(api, lctx, seg, oracle):  # noqa: F811
    """60 KiB of QOI_OP_RGBA chunks whose alpha byte reads as a QOI_OP_RGBA tag between clean streams: those lanes fail both run-ups and
    are redone by the plain parse, their neighbours stay with the line reader and add nothing to the count"""
    case = cm.never_case(oracle, seg)
    _sized(case, seg)
    lo, hi = _never_bounds(case, seg)
    fb = _run_at(api, lctx, seg, case, _want(oracle, case, 4), 4, _strided(case))
    assert lo <= fb <= hi, (lo, fb, hi)


def test_retry_never_meeting_and_clean_share_wavefronts(api, lctx, seg, oracle):  # noqa: F811
    case = cm.mixed_case(oracle, seg)
    _sized(case, seg)
    assert {k for k, _ in case} == {"c", "r", "h"}
    lo, hi = _never_bounds(case, seg)
    fb = _run_at(api, lctx, seg, case, _want(oracle, case, 4), 4, _strided(case, odd=True))
    assert lo <= fb <= hi, (lo, fb, hi)


def test_every_chunk_length_at_every_phase(api, lctx, seg, oracle):  # noqa: F811
    """3000 chunks each: QOI_OP_RGB at the four phases, the 12-byte cycle RGB / LUMA / RGBA / DIFF, INDEX and short runs between RGBA
    chunks, random bytes - from buffer byte 1 at an odd stride: a chunk of every length begins at every distance in front of a line end
    and of a segment end"""
    case = cm.phase_case(oracle, seg)
    _sized(case, seg)
    streams = [it[0] for _, it in case]
    stride = cm.phase_stride(streams)
    soffs = [1 + i * stride for i in range(len(case))]
    line, at_seg = cm.straddles(streams, soffs, seg)
    assert cm.ALL_STRADDLES <= line and cm.ALL_STRADDLES <= at_seg, (sorted(cm.ALL_STRADDLES - line), sorted(cm.ALL_STRADDLES - at_seg))
    _run_at(api, lctx, seg, case, _want(oracle, case, 4), 4, soffs)


@pytest.mark.parametrize("where", list(cm.END_LANES))
def test_stream_ends(api, lctx, seg, oracle, where):  # noqa: F811
    """streams cut after 1 .. 4 bytes of a QOI_OP_RGBA chunk and after one of a QOI_OP_LUMA chunk (the chunk's tail is the end marker's,
    qoi.h:539-575), chunks behind the last pixel, chunks for 3 % of the pixels - the segment in question on the wavefront's last, a
    middle and its first lane"""
    case, cuts = cm.ends_case(oracle, seg, where)
    _sized(case, seg)
    nsegs = [cm.n_segments(it[0], seg) for _, it in case]
    assert all((sum(nsegs[:i]) + crit) % cm.WAVE == cm.END_LANES[where] for i, crit in cuts)
    _run_at(api, lctx, seg, case, _want(oracle, case, 4), 4, _strided(case))


def test_packs_through_decode_images(api, lctx, seg, oracle):  # noqa: F811
    """the streams of the second run-up through qoimi_decode_images: packed back to back from buffer byte 1, the same listed shuffled and
    descending, one stream three times, and an image that is a sub-range of its predecessor's stream (out of the descriptor's reach)"""
    case = cm.retry_case(oracle, seg)
    want = _want(oracle, case, 4)
    n = len(case)
    base = _run_at(api, lctx, seg, case, want, 4, _strided(case))
    tight = [1 + sum(len(it[0]) for _, it in case[:i]) for i in range(n)]
    assert len({o % 128 for o in tight}) >= n - 2 and {o % 2 for o in tight} == {0, 1}     # (nearly as many address residues as streams)
    assert _run_at(api, lctx, seg, case, want, 4, tight, via="images") == base
    shuffled = [int(i) for i in np.random.default_rng(3).permutation(n)]
    assert _run_at(api, lctx, seg, case, want, 4, tight, via="images", listed=shuffled) == base
    assert _run_at(api, lctx, seg, case, want, 4, tight, via="images", listed=list(range(n))[::-1]) == base
    # one stream in three places of the output: beside the strided call of the same list (three copies of the stream in its buffer)
    thrice = case[:3] + [case[3]] * 3 + case[4:]
    _sized(thrice, seg)
    want3 = _want(oracle, thrice, 4)
    base3 = _run_at(api, lctx, seg, thrice, want3, 4, _strided(thrice))
    listed = [0, 1, 2, 3, 3, 3] + list(range(4, n))
    assert _run_at(api, lctx, seg, case, want, 4, tight, via="images", listed=listed) == base3
    # overlapping input: the long stream, then the short one that lies inside it - the call's last wavefront ends with the short stream's
    # last byte, in front of the long one's
    long_item, short_item, inside = cm.overlap_pair(oracle, seg)
    over = case[:-2] + [("o", long_item), ("o", short_item)]
    _sized(over, seg)
    nsegs = [cm.n_segments(it[0], seg) for _, it in over]
    assert sum(nsegs) % cm.WAVE > nsegs[-1] or sum(nsegs) % cm.WAVE == 0, "no segment of the long stream in the short one's last wavefront"
    soffs = [1 + sum(len(it[0]) for _, it in over[:i]) for i in range(len(over) - 1)]
    soffs.append(soffs[-1] + inside)
    assert _run_at(api, lctx, seg, over, _want(oracle, over, 4), 4, soffs, via="images") > 0


def test_sub_batches_between_wavefront_sharing_images(api, lctx, seg, oracle):  # noqa: F811
    """the second run-up call and the never-meeting call under a 1 MiB record cap: three sub-batches or more, cut between images that
    shared a wavefront - the same pixels and the same count as in one piece"""
    os.environ["QOIMI_SEG_BYTES"] = str(seg)
    os.environ["QOIMI_DEC_FUSED"] = "0"
    os.environ["QOIMI_DEC_REC_CAP_MB"] = "1"
    try:
        capped = api.Context(0)
    finally:
        del os.environ["QOIMI_SEG_BYTES"], os.environ["QOIMI_DEC_FUSED"], os.environ["QOIMI_DEC_REC_CAP_MB"]
    try:
        for one in (cm.retry_case(oracle, seg), cm.never_case(oracle, seg)):
            lens = [len(it[0]) for _, it in one]
            case = one * cm.repeats_for_sub_batches(lens, seg)
            _sized(case, seg)
            parts = cm.sub_batches([len(it[0]) for _, it in case], seg)
            assert len(parts) >= 3, parts
            nsegs = [cm.n_segments(it[0], seg) for _, it in case]
            assert any(sum(nsegs[:sum(parts[:k])]) % cm.WAVE for k in range(1, len(parts))), "every cut falls between two wavefronts"
            want = _want(oracle, case, 4)
            whole = _run_at(api, lctx, seg, case, want, 4, _strided(case))
            assert _run_at(api, capped, seg, case, want, 4, _strided(case)) == whole
    finally:
        capped.close()
