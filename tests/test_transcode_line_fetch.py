"""The batch transcoder's line-granular stream reader (dec_transcode<2>, LineReader in qoi_decode.hip) on the device: every case
goes through qoimi_decode_batch on the batch path (QOIMI_DEC_FUSED=0) at 1 KiB, 2 KiB and 4 KiB segments and is compared with the
reference decoder's pixels.  What the cases aim at: the last line of a stream partial / exactly full / one byte into the next; a
lane's first line entered at every offset; chunks that straddle every line end at every phase; lanes out of the wavefront
descriptor's reach (they take the plain reader); wavefronts with idle lanes and lanes that end mid-line."""
import numpy as np
import pytest
from gpu_pack import lctx, oracle  # noqa: F401  (fixtures)
from model_cases import line_stream as _stream, line_walk as _walk

pytestmark = pytest.mark.gpu


def _diff_body(n, seed):
    """n one-byte chunks (QOI_OP_DIFF): n pixels"""
    rng = np.random.default_rng(seed)
    b = (0x40 | rng.integers(0, 64, n)).astype(np.uint8)
    b[b == 0x6A] = 0x6B                                   # (0x6A is "no change": keep the pixels moving)
    return b.tobytes()


# this module's own api: the body of gpu_pack.api without the lint mark on its torch import - nothing else differs.  lctx (gpu_pack) asks
# for `api` by name and so gets this one here.
@pytest.fixture(scope="module")
def api():
    import torch
    from qoi_amd import api as _api
    assert torch.cuda.is_available()
    return _api


_WANT = {}


def _want(oracle, key, streams):
    """the reference decoder's pixels of a case's streams: computed once, shared by the three segment sizes, never written to"""
    if key not in _WANT:
        ws = [oracle.decode(s, 4)[0] for s in streams]
        for a in ws:
            a.setflags(write=False)
        _WANT[key] = ws
    return _WANT[key]


def _run(api, ctx, streams, descs, want, stride, lead=0):
    """the streams `stride` bytes apart from byte `lead` of a buffer, decoded in ONE call; pixels against `want`, guard bytes behind"""
    import torch
    n = len(streams)
    host = np.zeros(lead + n * stride + 256, dtype=np.uint8)
    for i, s in enumerate(streams):
        assert len(s) <= stride
        host[lead + i * stride:lead + i * stride + len(s)] = np.frombuffer(s, dtype=np.uint8)
    buf = torch.from_numpy(host).cuda()
    pstride = max(a.size for a in want)
    out = torch.full((n * pstride + 8,), 0xAB, dtype=torch.uint8, device="cuda")
    ctx.decode_batch(buf.data_ptr() + lead, stride, [len(s) for s in streams], descs, 4, out.data_ptr(), pstride)
    got = out.cpu().numpy()
    for i in range(n):
        assert np.array_equal(got[i * pstride:i * pstride + want[i].size], want[i]), (i, len(streams[i]), descs[i].width, descs[i].height)
    assert int(got[n * pstride]) == 0xAB, "wrote past the last image"


TAILS = [0, 1, 15, 16, 17, 127, 128, 129]


@pytest.mark.parametrize("base", [0, 3072])
def test_last_line_partial_full_and_one_over(api, lctx, oracle, base):
    """streams of 14 + 8 + base + {0, 1, 15, 16, 17, 127, 128, 129} bytes (one-byte chunks), eight in one call"""
    streams, descs = [], []
    for k, t in enumerate(TAILS):
        n = base + t
        streams.append(_stream(max(n, 1), 1, _diff_body(n, 100 + k)))
        descs.append(api.QoiDesc(max(n, 1), 1, 4, 0))
    stride = (max(len(s) for s in streams) + 15) // 16 * 16
    _run(api, lctx, streams, descs, _want(oracle, ("tails", base), streams), stride)


@pytest.mark.parametrize("odd", [False, True])
def test_first_line_entered_at_every_offset(api, lctx, oracle, odd):
    """128 streams in one call, the stride the bound rounded up to 16 (eight residues mod 128) - and that plus one: every residue"""
    w, h = 48, 40
    if "offsets/streams" not in _WANT:
        _WANT["offsets/streams"] = [oracle.encode(_walk(w, h, 200 + i), w, h, 4) for i in range(128)]
    streams = _WANT["offsets/streams"]
    stride = (max(len(s) for s in streams) + 8 + 15) // 16 * 16 + (1 if odd else 0)
    _run(api, lctx, streams, [api.QoiDesc(w, h, 4, 0)] * 128, _want(oracle, "offsets", streams), stride)


def test_chunks_straddle_every_line_end(api, lctx, oracle):
    """QOI_OP_RGBA only (five bytes: a chunk across every line end at every phase within 128 chunks), the same with a one-byte
    chunk every 37th (the run-up's chains meet: the segments stay with the line reader), QOI_OP_LUMA only; odd alignment"""
    rng = np.random.default_rng(7)
    n = 3000
    rgba = bytearray()
    mixed = bytearray()
    for i in range(n):
        c = bytes([0xFF]) + rng.integers(0, 256, 4, dtype=np.uint8).tobytes()
        rgba += c
        mixed += c if i % 37 else bytes([0x40 | int(rng.integers(0, 64))])
    luma = bytearray()
    for i in range(n):
        luma += bytes([0x80 | int(rng.integers(0, 64)), int(rng.integers(0, 256))])
    streams = [_stream(n, 1, rgba), _stream(n, 1, mixed), _stream(n, 1, luma), _stream(n, 1, mixed[5:] + mixed[:5]), _stream(n, 1, luma[2:] + luma[:2])]
    descs = [api.QoiDesc(n, 1, 4, 0)] * len(streams)
    stride = (max(len(s) for s in streams) + 15) // 16 * 16 + 1
    _run(api, lctx, streams, descs, _want(oracle, "straddle", streams), stride, lead=1)


def test_streams_gigabytes_apart(api, lctx, oracle):
    """streams 2.5 GiB apart (tests/test_gpu_parity.py::test_decode_streams_gigabytes_apart at batch segments): lanes of one
    wavefront lie 4 GiB and more behind its first stream - out of the descriptor's reach, they take the plain reader"""
    import torch
    w, h, n = 64, 40, 4
    stride = 5 << 29
    imgs = [_walk(w, h, 300 + i, alpha=True) for i in range(n)]
    streams = [oracle.encode(px, w, h, 4) for px in imgs]
    buf = torch.zeros((n - 1) * stride + 65536, dtype=torch.uint8, device="cuda")
    for i, st in enumerate(streams):
        buf[i * stride:i * stride + len(st)] = torch.from_numpy(np.frombuffer(st, dtype=np.uint8).copy()).cuda()
    out = torch.full((n * w * h * 4 + 8,), 0xAB, dtype=torch.uint8, device="cuda")
    lctx.decode_batch(buf.data_ptr(), stride, [len(st) for st in streams], [api.QoiDesc(w, h, 4, 0)] * n, 4, out.data_ptr(), w * h * 4)
    got = out.cpu().numpy()
    for i in range(n):
        assert np.array_equal(got[i * w * h * 4:(i + 1) * w * h * 4], imgs[i].reshape(-1)), i
    assert int(got[n * w * h * 4]) == 0xAB, "wrote past the last image"
    assert lctx.decode_stats()["sync_fallback_segments"] > 0, "no segment lay out of the descriptor's reach: the test does not test"
    del buf


def test_small_images_beside_a_large_one(api, lctx, oracle):
    """64 images of 64 x 48 and one of 2048 x 1536 in one call: wavefronts with idle lanes and lanes that end mid-line"""
    key = "mixed_sizes"
    if key not in _WANT:
        small = [(64, 48, _walk(64, 48, 400 + i, alpha=(i % 5 == 0))) for i in range(64)]
        big = (2048, 1536, _walk(2048, 1536, 499))
        imgs = small[:32] + [big] + small[32:]
        _WANT[key + "/streams"] = [oracle.encode(px, w, h, 4) for w, h, px in imgs]
        _WANT[key + "/dims"] = [(w, h) for w, h, _ in imgs]
    streams = _WANT[key + "/streams"]
    descs = [api.QoiDesc(w, h, 4, 0) for w, h in _WANT[key + "/dims"]]
    stride = (max(len(s) for s in streams) + 15) // 16 * 16
    _run(api, lctx, streams, descs, _want(oracle, key, streams), stride)
