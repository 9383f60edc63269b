"""GPU parity tests (-m gpu): the HIP path, called through the C-ABI, against the oracle.

* drop-in qoi_encode: stream BYTE-IDENTICAL to the reference encoder's (golden vectors)
* drop-in qoi_decode: pixels bit-identical to the reference decoder's for every golden
  stream incl. truncated / malformed / adversarial ones; NULL exactly where it returns NULL
* device-resident batch API at BASELINE sizes: synthetic frames generated on the GPU,
  compared with the oracle (live) and through the round-trip property qoibench.c:408-417
"""
import os
import zlib

import numpy as np
import pytest

import cases
from gpu_pack import api, ctx, oracle  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ drop-in encode
def test_encode_golden_byte_identical(api, golden):
    for c in cases.encode_cases():
        s = api.qoi_encode(c["pixels"], api.QoiDesc(c["w"], c["h"], c["ch"], c["cs"]))
        assert s is not None, (c["name"], api.last_error())
        want = golden[f"enc/{c['name']}/stream"].tobytes()
        assert s == want, (c["name"], len(s), len(want), first_diff(s, want))


def first_diff(a, b):
    n = min(len(a), len(b))
    for i in range(n):
        if a[i] != b[i]:
            return i, a[max(0, i - 4):i + 8].hex(), b[max(0, i - 4):i + 8].hex()
    return n, None, None


def test_encode_rejections(api):
    px = np.zeros(64, dtype=np.uint8)
    for c in cases.encode_arg_cases():
        assert api.qoi_encode(px, api.QoiDesc(c["w"], c["h"], c["ch"], c["cs"])) is None, c["name"]


# ------------------------------------------------------------------ drop-in decode
def test_decode_golden_bit_exact(api, golden, encoded_streams):
    n = 0
    for c in cases.decode_cases(encoded_streams):
        px, d = api.qoi_decode(c["stream"], c["channels"], c["size"])
        ok = bool(golden[f"dec/{c['name']}/ok"][0])
        assert (px is not None) == ok, (c["name"], api.last_error())
        if len(c["stream"]) >= 22 and c["channels"] in (0, 3, 4):
            assert [d.width, d.height, d.channels, d.colorspace] == list(golden[f"dec/{c['name']}/desc"]), c["name"]
        if ok:
            want = golden[f"dec/{c['name']}/pixels"]
            assert np.array_equal(px, want), (c["name"], int(np.argmax(px != want)))
        n += 1
    assert n > 150


@pytest.mark.parametrize("seg,l2m", [(64, "1"), (333, "1"), (64, "2")])
def test_decode_small_segments(api, golden, encoded_streams, seg, l2m):
    """Same golden streams with tiny decode segments: every segment boundary case + restart loop (l2m 2: with the
    multi-workgroup state chain that calls of a few large images use)."""
    os.environ["QOIMI_SEG_BYTES"] = str(seg)
    os.environ["QOIMI_DEC_L2M"] = l2m
    try:
        import torch
        c = api.Context(0)
        for case in cases.decode_cases(encoded_streams):
            if not bool(golden[f"dec/{case['name']}/ok"][0]):
                continue
            desc = golden[f"dec/{case['name']}/desc"]
            d = api.QoiDesc(int(desc[0]), int(desc[1]), int(desc[2]), int(desc[3]))
            och = case["channels"] or d.channels
            s = torch.from_numpy(np.frombuffer(case["stream"] + b"\0" * 8, dtype=np.uint8).copy()).cuda()
            out = torch.full((d.width * d.height * och + 8,), 0xAB, dtype=torch.uint8, device="cuda")
            c.decode_batch(s.data_ptr(), s.numel(), [len(case["stream"])], [d], case["channels"],
                           out.data_ptr(), d.width * d.height * och)
            got = out[:d.width * d.height * och].cpu().numpy()
            assert np.array_equal(got, golden[f"dec/{case['name']}/pixels"]), (case["name"], seg)
            assert int(out[d.width * d.height * och]) == 0xAB, "wrote past the image"
        c.close()
    finally:
        del os.environ["QOIMI_SEG_BYTES"]
        del os.environ["QOIMI_DEC_L2M"]


def test_decode_record_dense_segments(api, oracle):
    """A QOI_OP_RGBA chunk that starts on the last byte of a decode segment full of one-byte chunks: B + 1 chunk records
    from B stream bytes (cases.dense_record_streams) - at every segment size the cost model can pick."""
    import torch
    for name, B, stream, w, h in cases.dense_record_streams():
        want, _ = oracle.decode(stream, 4)
        os.environ["QOIMI_SEG_BYTES"] = str(B)
        try:
            c = api.Context(0)
            d = api.QoiDesc(w, h, 4, 0)
            s = torch.from_numpy(np.frombuffer(stream + b"\0" * 8, dtype=np.uint8).copy()).cuda()
            out = torch.full((w * h * 4 + 8,), 0xAB, dtype=torch.uint8, device="cuda")
            c.decode_batch(s.data_ptr(), s.numel(), [len(stream)], [d], 4, out.data_ptr(), w * h * 4)
            assert np.array_equal(out[:w * h * 4].cpu().numpy(), want), name
            assert int(out[w * h * 4]) == 0xAB, "wrote past the image"
            c.close()
        finally:
            del os.environ["QOIMI_SEG_BYTES"]


@pytest.mark.parametrize("seg", [None, "64", "128"])
def test_decode_record_pairs(api, oracle, seg):
    """QOI_OP_RGB / QOI_OP_RGBA become pairs of records on even record indices and P3 / P4 take blocks of pairs on a short path
    (cases.pair_streams): all-pair streams, pairs displaced by one-byte chunks, mixtures - 3- and 4-channel output."""
    import torch
    if seg is not None:
        os.environ["QOIMI_SEG_BYTES"] = seg
    try:
        c = api.Context(0)
        for name, stream, w, h in cases.pair_streams():
            s = torch.from_numpy(np.frombuffer(stream + b"\0" * 8, dtype=np.uint8).copy()).cuda()
            for och in (4, 3):
                want, _ = oracle.decode(stream, och)
                out = torch.full((w * h * och + 8,), 0xAB, dtype=torch.uint8, device="cuda")
                c.decode_batch(s.data_ptr(), s.numel(), [len(stream)], [api.QoiDesc(w, h, 4, 0)], och, out.data_ptr(), w * h * och)
                assert np.array_equal(out[:w * h * och].cpu().numpy(), want), (name, och)
                assert int(out[w * h * och]) == 0xAB, "wrote past the image"
        c.close()
    finally:
        if seg is not None:
            del os.environ["QOIMI_SEG_BYTES"]


@pytest.mark.parametrize("seg", [None, "64", "128", "512", "4096"])
@pytest.mark.parametrize("run_desc", ["1", "0"])
def test_decode_flat_images_run_descriptors(api, oracle, seg, run_desc):
    """Flat images (less than a byte per eight pixels) write their long runs through run descriptors (dec_segments_rec<OCH, true>,
    dec_expand_runs): cases.flat_run_streams - runs merged over the 62 cap, every head alignment and tail length, runs that open the
    image, run over its end or stop short of it, alpha levels - one by one at every segment size, 3- and 4-channel output, and all of
    them in ONE call beside a photograph and a noise image (which take the lane-written path).  run_desc 0: the same without
    descriptors (QOIMI_DEC_RUN_DESC=0)."""
    import torch
    from qoi_amd import synth
    if seg is not None:
        os.environ["QOIMI_SEG_BYTES"] = seg
    os.environ["QOIMI_DEC_RUN_DESC"] = run_desc
    try:
        c = api.Context(0)
        streams = list(cases.flat_run_streams())
        for name, stream, w, h in streams:
            if seg in ("64", "128") and len(stream) > 100000:
                continue
            s = torch.from_numpy(np.frombuffer(stream + b"\0" * 8, dtype=np.uint8).copy()).cuda()
            for och in (4, 3):
                want, _ = oracle.decode(stream, och)
                out = torch.full((w * h * och + 8,), 0xAB, dtype=torch.uint8, device="cuda")
                c.decode_batch(s.data_ptr(), s.numel(), [len(stream)], [api.QoiDesc(w, h, 4, 0)], och, out.data_ptr(), w * h * och)
                got = out[:w * h * och].cpu().numpy()
                assert np.array_equal(got, want), (name, och, seg, int(np.argmax(got != want)))
                assert int(out[w * h * och]) == 0xAB, "wrote past the image"
        # one call: the flat images between a photograph and a noise image
        extra = [(k, oracle.encode(synth.frame_rgba(k, 320, 200, 9), 320, 200, 4), 320, 200) for k in ("photo", "noise")]
        items = [extra[0]] + streams[:6] + [extra[1]] + streams[6:]
        sstride = max(len(x[1]) for x in items) + 64
        for och in (4, 3):
            pstride = max(x[2] * x[3] for x in items) * och + 32
            buf = torch.zeros(len(items) * sstride, dtype=torch.uint8, device="cuda")
            for i, (_, st, _, _) in enumerate(items):
                buf[i * sstride:i * sstride + len(st)].copy_(torch.from_numpy(np.frombuffer(st, dtype=np.uint8).copy()))
            out = torch.full((len(items) * pstride,), 0xAB, dtype=torch.uint8, device="cuda")
            c.decode_batch(buf.data_ptr(), sstride, [len(x[1]) for x in items], [api.QoiDesc(x[2], x[3], 4, 0) for x in items], och, out.data_ptr(), pstride)
            host = out.cpu().numpy()
            for i, (name, st, w, h) in enumerate(items):
                want, _ = oracle.decode(st, och)
                assert np.array_equal(host[i * pstride:i * pstride + w * h * och], want), (name, och, seg, "batch")
                assert (host[i * pstride + w * h * och:(i + 1) * pstride] == 0xAB).all(), (name, "wrote past the image")
        c.close()
    finally:
        if seg is not None:
            del os.environ["QOIMI_SEG_BYTES"]
        del os.environ["QOIMI_DEC_RUN_DESC"]


def test_round_trip_random_host_api(api, oracle):
    rng = np.random.default_rng(7)
    for it in range(40):
        w = int(rng.integers(1, 300)); h = int(rng.integers(1, 60)); ch = 3 + int(rng.integers(0, 2))
        if it % 3 == 0:
            px = rng.integers(0, 256, size=(w * h, ch), dtype=np.uint8)
        elif it % 3 == 1:
            pal = rng.integers(0, 256, size=(int(rng.integers(1, 50)), ch), dtype=np.uint8)
            px = pal[rng.integers(0, len(pal), size=w * h)]
        else:
            px = np.cumsum(rng.integers(-3, 4, size=(w * h, ch)), axis=0).astype(np.uint8)
        s = api.qoi_encode(px, api.QoiDesc(w, h, ch, 0))
        assert s == oracle.encode(px, w, h, ch), (it, w, h, ch)
        for chn in (0, 3, 4):
            got, _ = api.qoi_decode(s, chn)
            want, _ = oracle.decode(s, chn)
            assert np.array_equal(got, want), (it, chn)


@pytest.mark.parametrize("tight", ["1", "0"])
def test_host_encode_result_outgrows_the_expected_size(api, oracle, tight):
    """QOIMI_ENCODE_TIGHT_BUFFER=1: qoi_encode sizes its malloc by the calling thread's previous stream (qoi_host.hip): a flat frame,
    then noise (the stream is two hundred times longer than expected: the exact-size path), then flat again - byte-identical every
    time; the same with the default, the reference's worst-case allocation (qoi.h:374-379), of which only the expected pages are populated."""
    from qoi_amd import synth
    w, h = 1920, 1080
    import threading
    os.environ["QOIMI_ENCODE_TIGHT_BUFFER"] = tight
    bad = []

    def work():                       # a fresh thread: its context reads the variable when it is created (once, not per call)
        for kind in ("constant", "noise", "constant", "photo", "noise"):
            px = synth.frame_rgba(kind, w, h, 11).reshape(-1, 4)
            s = api.qoi_encode(px, api.QoiDesc(w, h, 4, 0))
            if s != oracle.encode(px, w, h, 4):
                bad.append(kind)
    try:
        t = threading.Thread(target=work)
        t.start(); t.join()
        assert not bad, bad
    finally:
        del os.environ["QOIMI_ENCODE_TIGHT_BUFFER"]


def _hook_scenario(*args):
    """The failure-injection hooks (QOIMI_TEST_*) exist in the TEST flavour of the library only (make TEST_HOOKS=1): scenarios that
    need them run in a child process that selects that build before its first call (tests/libsel.py, tests/hook_scenarios.py)."""
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "hook_scenarios.py")] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


@pytest.mark.parametrize("n,w,h", [(1, 1920, 1080), (3, 1280, 720), (12, 1280, 720)])
def test_a_placement_wait_that_gives_up_is_encoded_again_order_free(api, n, w, h):
    """QOIMI_TEST_SPIN_BOUND=1: every placement wait (tree by workgroup index for fewer than 8 images, look-back for more) that needs a
    second poll gives up, ends the launch's other waits and leaves err set; qoimi_encode_status then encodes the call again order-free -
    QOIMI_OK, the reference's bytes, and qoimi_encode_retries counts it (tests/hook_scenarios.py: spin_bound)."""
    out = _hook_scenario("spin_bound", n, w, h)
    assert "retries" in out


# ------------------------------------------------------------------ device batch API
@pytest.mark.parametrize("kind", ["photo", "noise", "uiflat", "constant", "photo_hard", "sprite_alpha"])
def test_4k_frame_device_path(api, ctx, oracle, kind):
    """BASELINE config 2: one 3840x2160 RGBA frame, encode + decode on the GPU, bit-exact."""
    import torch
    from gpu_util import DeviceBatch
    from qoi_amd import synth
    w, h = 3840, 2160
    b = DeviceBatch(ctx, w, h, 4, 1)
    ctx.synth_frames(synth.KIND_ID[kind], synth.DEFAULT_SEED, 5, 1, w, h, b.pixels.data_ptr(), b.pixel_stride, b.stream)
    host = synth.frame_rgba(kind, w, h, 5)
    assert np.array_equal(b.pixels[:w * h * 4].cpu().numpy(), host.reshape(-1)), "device generator != synth.py"
    lens = b.encode()
    want = oracle.encode(host, w, h, 4)
    got = b.stream_bytes(0, lens[0])
    assert len(got) == len(want) and got == want, (kind, lens[0], len(want))
    out = torch.zeros(b.pixel_stride, dtype=torch.uint8, device="cuda")
    b.decode_into(out, lens)
    assert torch.equal(out[:w * h * 4], b.pixels[:w * h * 4]), kind
    assert ctx.decode_stats()["segments"] > 0


@pytest.mark.parametrize("slabs", ["1", "3"])
def test_tree_placement_three_levels(api, oracle, slabs):
    """Tree placement with sets past one block of 64 groups (more than 4096 sets per image): three 2800 x 1600 images at one slab
    per set (4375 sets each: 69 groups, 2 blocks) - a photograph, noise (every set spills through the pool) and a flat UI frame
    (the generic pass, which places by its own tree) - byte-identical to the reference; 3 and 4 channels."""
    import torch
    from gpu_util import DeviceBatch
    from qoi_amd import synth
    old = {k: os.environ.get(k) for k in ("QOIMI_ENC_SET_SLABS", "QOIMI_ENC_LOOKBACK")}
    os.environ["QOIMI_ENC_SET_SLABS"] = slabs
    os.environ["QOIMI_ENC_LOOKBACK"] = "2"
    try:
        c = api.Context(0)
        w, h = 2800, 1600
        for ch in (4, 3):
            kinds = ["photo", "noise", "uiflat"]
            frames = [np.ascontiguousarray(synth.frame_rgba(k, w, h, 77 + i)[:, :, :ch]) for i, k in enumerate(kinds)]
            b = DeviceBatch(c, w, h, ch, len(kinds))
            for i, f in enumerate(frames):
                b.upload(i, f)
            lens = b.encode()
            torch.cuda.synchronize()
            for i, f in enumerate(frames):
                want = oracle.encode(f, w, h, ch)
                assert b.stream_bytes(i, lens[i]) == want, (slabs, ch, kinds[i], int(lens[i]), len(want))
        c.close()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.parametrize("env", [{}, {"QOIMI_ENC_LOOKBACK": "0"}, {"QOIMI_ENC_LOOKBACK": "0", "QOIMI_ENC_SET_SLABS": "1"}, {"QOIMI_ENC_LOOKBACK": "1"},
                                 {"QOIMI_ENC_LOOKBACK": "2", "QOIMI_ENC_SET_SLABS": "1"}, {"QOIMI_ENC_WARM": "0", "QOIMI_ENC_SET_SLABS": "2"},
                                 {"QOIMI_ENC_PROBE": "0"}])
def test_start_value_runs_past_the_first_set(api, oracle, env):
    """An image that OPENS with pixels of the start value {0,0,0,255} (qoi.h:396-399) - a letterboxed frame's black rows - for longer
    than its first set: those pixels are repeats of a value no edge has put into the colour table, so the first later pixel of that
    value must NOT find itself there (qoi.h:430-436: the slot is still zero, a literal chunk follows).  Round 4's encoder fuzz
    (tests/fuzz_encode.py) found the plain form of a step writing it through its all-lanes probe: QOI_OP_INDEX 53 instead of the
    reference's chunk, round trip exact, four bytes short.  Opening runs around every set size, 3 and 4 channels, every placement."""
    import torch
    from gpu_util import DeviceBatch
    from qoi_amd import synth
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        c = api.Context(0)
        w, h = 1000, 40
        for ch in (4, 3):
            opens = [1000, 1024, 1025, 2047, 3072, 3073, 8191, 8192, 8193, 20000, 39999]
            frames = []
            for k, n0 in enumerate(opens):
                a = np.zeros((w * h, 4), dtype=np.uint8); a[:, 3] = 255
                rest = synth.frame_rgba("photo" if k % 2 else "uiflat", w, h, 50 + k).reshape(-1, 4)
                a[n0:] = rest[n0:]
                a[n0 + 1::97] = (0, 0, 0, 255)                 # the start value again, as an edge pixel, here and there
                a[n0:, 3] = 255
                frames.append(np.ascontiguousarray(a.reshape(h, w, 4)[:, :, :ch]))
            # a letterboxed frame: black rows on top and bottom, a photograph between them
            lb = synth.frame_rgba("photo", w, h, 99).copy(); lb[:12] = (0, 0, 0, 255); lb[-9:] = (0, 0, 0, 255); lb[:, :, 3] = 255
            frames.append(np.ascontiguousarray(lb[:, :, :ch]))
            for n in (1, len(frames)):                       # alone (tree / order-free) and as a batch (look-back)
                b = DeviceBatch(c, w, h, ch, n)
                use = frames[-n:]
                for i, f in enumerate(use):
                    b.upload(i, f)
                lens = b.encode()
                torch.cuda.synchronize()
                for i, f in enumerate(use):
                    want = oracle.encode(f, w, h, ch)
                    assert b.stream_bytes(i, lens[i]) == want, (env, ch, n, i, int(lens[i]), len(want))
        c.close()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def test_batch_1080p_frames(api, ctx, oracle):
    """BASELINE config 3 shape (batch of 1920x1080 frames), 12 distinct frames, mixed content."""
    import torch
    from gpu_util import DeviceBatch
    from qoi_amd import synth
    w, h, n = 1920, 1080, 12
    b = DeviceBatch(ctx, w, h, 4, n)
    kinds = ["photo", "noise", "uiflat", "constant"]
    for i in range(n):
        ctx.synth_frames(synth.KIND_ID[kinds[i % 4]], synth.DEFAULT_SEED, 100 + i, 1, w, h,
                         b.pixels.data_ptr() + i * b.pixel_stride, b.pixel_stride, b.stream)
    lens = b.encode()
    for i in (0, 1, 2, 3, 11):
        host = synth.frame_rgba(kinds[i % 4], w, h, 100 + i)
        assert b.stream_bytes(i, lens[i]) == oracle.encode(host, w, h, 4), i
    out = torch.zeros(n * b.pixel_stride, dtype=torch.uint8, device="cuda")
    b.decode_into(out, lens)
    assert torch.equal(out.view(n, -1)[:, :w * h * 4], b.pixels.view(n, -1)[:, :w * h * 4])


def test_three_channel_device_path(api, ctx, oracle):
    import torch
    from gpu_util import DeviceBatch
    from qoi_amd import synth
    w, h = 1000, 700
    host = synth.frame_rgb("photo", w, h, 9)
    b = DeviceBatch(ctx, w, h, 3, 2)
    b.upload(0, host); b.upload(1, host[::-1].copy())
    lens = b.encode()
    assert b.stream_bytes(0, lens[0]) == oracle.encode(host, w, h, 3)
    for och in (3, 4):
        stride = (w * h * och + 255) // 256 * 256
        out = torch.zeros(2 * stride, dtype=torch.uint8, device="cuda")
        b.decode_into(out, lens, och)
        want, _ = oracle.decode(b.stream_bytes(0, lens[0]), och)
        assert np.array_equal(out[:w * h * och].cpu().numpy(), want)


def test_16k_frame_round_trip(api, ctx):
    """BASELINE config 4: 16384x16384 (268 Mpx, near the 400 Mpx cap) - scan / LDS stress.
    Oracle-free size-independent property: decode(encode(x)) == x, plus stream well-formedness."""
    import torch
    from gpu_util import DeviceBatch
    from qoi_amd import synth
    w = h = 16384
    b = DeviceBatch(ctx, w, h, 4, 1)
    ctx.synth_frames(synth.KIND_ID["photo"], synth.DEFAULT_SEED, 1, 1, w, h, b.pixels.data_ptr(), b.pixel_stride, b.stream)
    lens = b.encode()
    n = int(lens[0])
    head = b.stream_bytes(0, 14)
    assert head[:4] == b"qoif" and int.from_bytes(head[4:8], "big") == w and int.from_bytes(head[8:12], "big") == h
    tail = b.streams[n - 8:n].cpu().numpy().tobytes()
    assert tail == b"\0\0\0\0\0\0\0\x01"
    assert 1.0 < n / (w * h) < 1.5
    out = torch.zeros(b.pixel_stride, dtype=torch.uint8, device="cuda")
    b.decode_into(out, lens)
    assert torch.equal(out[:w * h * 4], b.pixels[:w * h * 4])
    # checksum-of-checksums against the CPU oracle on a 1/64 strip of the same frame is
    # covered at 4K; here the whole-image property is the check.


def test_16k_frame_stream_is_the_reference_stream(api, ctx, ref):
    """BASELINE config 4 against the reference ENCODER: the 16384 x 16384 stream (335 MB) equals what qoi.h:356 writes for
    the same pixels, byte for byte (the reference takes a few seconds for it on one host core)."""
    import torch
    from gpu_util import DeviceBatch
    from qoi_amd import synth
    if ref is None:
        pytest.skip("oracle/_ref/libqoiref.so not built")
    w = h = 16384
    b = DeviceBatch(ctx, w, h, 4, 1)
    ctx.synth_frames(synth.KIND_ID["photo"], synth.DEFAULT_SEED, 2, 1, w, h, b.pixels.data_ptr(), b.pixel_stride, b.stream)
    lens = b.encode()
    n = int(lens[0])
    host_px = b.pixels[:w * h * 4].cpu().numpy()
    want = ref.encode(host_px, w, h, 4)
    assert len(want) == n
    got = b.streams[:n].cpu().numpy()
    assert np.array_equal(got, np.frombuffer(want, dtype=np.uint8))
    del want, got, host_px
    torch.cuda.empty_cache()


@pytest.mark.parametrize("env", [
    {"QOIMI_ENC_WARM": "0", "QOIMI_ENC_LOOKBACK": "1"},   # entry states from per-slab summaries + scans for every image (look-back placement)
    {"QOIMI_ENC_LOOKBACK": "0"},                          # order-free placement: sets park their bytes, enc_offsets + enc_compact place them
    {"QOIMI_ENC_LOOKBACK": "0", "QOIMI_ENC_WARM": "0"},   # ... with the entry states from the summary passes
    {"QOIMI_ENC_SET_SLABS": "4", "QOIMI_ENC_LOOKBACK": "1"},   # four slabs per wavefront, look-back placement (forced: a call of four images takes the tree)
    {"QOIMI_ENC_SET_SLABS": "8", "QOIMI_ENC_WARM": "0", "QOIMI_ENC_LOOKBACK": "1"},
    {"QOIMI_ENC_SET_SLABS": "3", "QOIMI_ENC_LOOKBACK": "0"},
    {"QOIMI_ENC_LOOKBACK": "2"},                          # tree placement (what calls of a few large images take): three windows of byte counts per set
    {"QOIMI_ENC_LOOKBACK": "2", "QOIMI_ENC_WARM": "0"},   # ... with the entry states from the summary passes
    {"QOIMI_ENC_LOOKBACK": "2", "QOIMI_ENC_SET_SLABS": "2", "QOIMI_ENC_PROBE": "0"},
    {"QOIMI_ENC_SET_SLABS": "4", "QOIMI_ENC_PROBE": "0", "QOIMI_ENC_LOOKBACK": "1"},
    {"QOIMI_ENC_TICKET": "0", "QOIMI_ENC_LOOKBACK": "1"},  # look-back with sets by workgroup index instead of by ticket
    {"QOIMI_ENC_PROBE": "0"},                             # order-independent colour-table probe (ds_or masks)
    {"QOIMI_DEC_FINE": "0", "QOIMI_SEG_BYTES": "2048"},   # lane-per-segment P1/P2 instead of 128-byte pieces
    {"QOIMI_SEG_BYTES": "1024"},                          # P1/P2 on 8 pieces per segment
    {"QOIMI_SEG_BYTES": "4096"},                          # what large batches choose: 32 pieces per segment
    {"QOIMI_SEG_BYTES": "128"},                           # the piece is the segment (single-frame calls choose this)
    {"QOIMI_SEG_BYTES": "512"},                           # lane-per-segment P1/P2 (4 pieces: no piece path)
    {"QOIMI_DEC_REFINE": "0", "QOIMI_SEG_BYTES": "2048"},  # repair rounds without alpha hints
    {"QOIMI_DEC_REC_CAP_MB": "1"},                        # record arena capped at 1 MiB: the batch is decoded in sub-batches
    {"QOIMI_SEG_BYTES": "320"},                           # a segment size without the 128-byte piece parse: full parse, transcode from S1's phases
    {"QOIMI_P3_PLAIN": "0"},                              # P3 on records in its general form from the first chunk on
    {"QOIMI_DEC_L2M": "2"},                               # the per-image level of the state chain as eight workgroups per image (calls of a few large images take it)
    {"QOIMI_DEC_L2M": "2", "QOIMI_SEG_BYTES": "128"},     # ... with many groups per image, several rounds (uiflat)
    {"QOIMI_DEC_L2M": "0"},                               # ... never
    {"QOIMI_ENC_PERSIST": "3", "QOIMI_ENC_LOOKBACK": "1"},  # three workgroups walk all units (grid-stride loop of enc_sets; look-back with tickets)
    {"QOIMI_ENC_SPREAD": "0", "QOIMI_ENC_LOOKBACK": "1"},  # the four wavefronts of a workgroup take their tickets from ONE image (the default: from consecutive images)
    {"QOIMI_ENC_SPREAD": "0", "QOIMI_ENC_SET_SLABS": "2", "QOIMI_ENC_LOOKBACK": "1"},
    {"QOIMI_ENC_SPREAD": "0", "QOIMI_ENC_PERSIST": "3", "QOIMI_ENC_LOOKBACK": "1"},  # ... in the grid-stride loop
    {"QOIMI_ENC_PIPE": "1", "QOIMI_ENC_PERSIST": "3", "QOIMI_ENC_LOOKBACK": "1"},   # experiment: a wavefront asks for its next set's look-back window in front of its current set's placement
    {"QOIMI_ENC_PIPE": "1", "QOIMI_ENC_PERSIST": "1", "QOIMI_ENC_LOOKBACK": "1", "QOIMI_ENC_SET_SLABS": "1"},
    {"QOIMI_ENC_GEN_SLABS": "16", "QOIMI_ENC_LOOKBACK": "1"},   # sixteen slabs per set in the pass over flagged images (what calls of 3 x 65536 slabs take)
    {"QOIMI_ENC_GEN_SLABS": "3", "QOIMI_ENC_LOOKBACK": "1"},
    {"QOIMI_ENC_UNI": "1"},                               # ONE encode pass, a set whose look-back window does not do takes the state look-back by itself
    {"QOIMI_ENC_UNI": "1", "QOIMI_ENC_LOOKBACK": "1"},
    {"QOIMI_ENC_UNI": "1", "QOIMI_ENC_LOOKBACK": "1", "QOIMI_ENC_SET_SLABS": "1"},
    {"QOIMI_ENC_G2": "0"},                                # flagged (flat) images through the summary passes (enc_slab_summary + scans + ENTRY 0) instead of the state look-back
    {"QOIMI_ENC_G2": "0", "QOIMI_ENC_LOOKBACK": "1"},
    {"QOIMI_ENC_LOOKBACK": "1"},                          # look-back placement (forced for four images): flat images by state look-back with tickets
    {"QOIMI_ENC_LOOKBACK": "1", "QOIMI_ENC_SET_SLABS": "1"},
    {"QOIMI_ENC_TREE_TICKET": "0"},                       # tree placement with its units by workgroup index (the drop-in qoi_encode's form; tickets are the default)
    {"QOIMI_DEC_RUN_DESC": "0"},                          # every long run written lane by lane
    {"QOIMI_DEC_RUN_DESC": "1"},                          # run descriptors for flat images only
    {"QOIMI_DEC_FUSED": "0"},                             # calls of a few images through the three-level chains of the batch path (default: dec_scan_entry + four wavefronts per group in the state chain)
    {"QOIMI_DEC_FUSED": "0", "QOIMI_SEG_BYTES": "128"},
    {"QOIMI_SEG_BYTES": "128"},                           # the single-pass look-back at the lone frame's segment size (the noise image makes the call fall back to the chains)
    {"QOIMI_SEG_BYTES": "1024"},
    {"QOIMI_DEC_SPLIT": "0", "QOIMI_SEG_BYTES": "128"},   # one transcoder lane per segment (default for 128-byte segments of small calls: two)
    {"QOIMI_DEC_S3_RIDE": "1", "QOIMI_SEG_BYTES": "128"},  # experiment: the per-image level of the state chain on the group level's launch (last arrivers)
    {"QOIMI_DEC_S3_RIDE": "1"},
    {"QOIMI_DEC_TR_SCAN": "1", "QOIMI_SEG_BYTES": "128"},  # experiment: dec_scan_entry's work as the epilogue of the two-lane transcoder
    {"QOIMI_DEC_TR_SCAN": "1"},
])
def test_selectable_paths(api, oracle, env):
    """Every selectable kernel path gives the same bytes / pixels (mixed batch: photo, noise, uiflat, constant)."""
    import torch
    from gpu_util import DeviceBatch
    from qoi_amd import synth
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        c = api.Context(0)
        w, h, n = 1024, 600, 4
        b = DeviceBatch(c, w, h, 4, n)
        kinds = ["photo", "noise", "uiflat", "constant"]
        for i in range(n):
            c.synth_frames(synth.KIND_ID[kinds[i]], synth.DEFAULT_SEED, 40 + i, 1, w, h,
                           b.pixels.data_ptr() + i * b.pixel_stride, b.pixel_stride, b.stream)
        lens = b.encode()
        for i in range(n):
            host = synth.frame_rgba(kinds[i], w, h, 40 + i)
            assert b.stream_bytes(i, lens[i]) == oracle.encode(host, w, h, 4), (env, kinds[i])
        out = torch.zeros(n * b.pixel_stride, dtype=torch.uint8, device="cuda")
        b.decode_into(out, lens)
        assert torch.equal(out.view(n, -1)[:, :w * h * 4], b.pixels.view(n, -1)[:, :w * h * 4]), env
        c.close()
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.mark.parametrize("seg", ["", "64", "80", "112", "128", "256", "512", "1024"])
@pytest.mark.parametrize("fused", ["1", "0"])
def test_small_calls_single_pass_lookback(api, oracle, seg, fused):
    """Calls of one to four images take dec_scan_entry (pixel offsets + speculated slots by a single-pass look-back over tagged words,
    every image on a multiple of 256 segments) and a state chain of four wavefronts per group - round 6.  Images of different shapes whose
    streams all synchronise (photographs, UI frames, a constant frame, soft-alpha sprites), a 1 x 1 image, a stream cut short (the
    pixels the chunks never reach repeat the last pixel, qoi.h:544) and a stream too long for its image; the same calls again on the same
    context (the look-back words carry the call's number, the counter header is zeroed by the call before), 3- and 4-channel output,
    against the reference decoder.  QOIMI_DEC_FUSED=0: the same through the three-level chains."""
    import torch
    from qoi_amd import synth
    env = {"QOIMI_DEC_FUSED": fused}
    if seg:
        env["QOIMI_SEG_BYTES"] = seg
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        c = api.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    shapes = [("photo", 1280, 720), ("uiflat", 640, 400), ("sprite_alpha", 333, 251), ("constant", 64, 64), ("photo_hard", 1, 1), ("photo", 97, 3), ("photo_hard", 800, 600), ("noise", 200, 150)]          # (noise: the transcoder cannot synchronise it - the five-phase parse, at every segment size)
    streams, descs = [], []
    for i, (kind, w, h) in enumerate(shapes):
        px = synth.frame_rgba(kind, w, h, 70 + i)
        st = oracle.encode(px, w, h, 4)
        streams.append(st); descs.append((w, h))
    # a stream cut short inside its chunks and one that goes on behind its image's last pixel (another image's chunks appended)
    cut = streams[0][:len(streams[0]) // 3] + streams[0][-8:]
    streams.append(cut); descs.append(descs[0])
    long_s = streams[1][:-8] + streams[5][14:]
    streams.append(long_s); descs.append(descs[1])
    stride_s = (max(len(s) for s in streams) + 255) // 256 * 256
    stride_p = (max(w * h for w, h in descs) * 4 + 255) // 256 * 256
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(5)
    for rep in range(6):
        n = int(rng.integers(1, 5))
        pick = [int(x) for x in rng.choice(len(streams), size=n, replace=False)]
        for och in (4, 3):
            d_s = torch.zeros(n * stride_s, dtype=torch.uint8, device="cuda")
            d_p = torch.full((n * stride_p,), 0xA5, dtype=torch.uint8, device="cuda")
            for k, i in enumerate(pick):
                d_s[k * stride_s:k * stride_s + len(streams[i])] = torch.frombuffer(bytearray(streams[i]), dtype=torch.uint8).cuda()
            c.decode_batch(d_s.data_ptr(), stride_s, [len(streams[i]) for i in pick], [api.QoiDesc(descs[i][0], descs[i][1], 4, 0) for i in pick],
                           och, d_p.data_ptr(), stride_p, stream)
            for k, i in enumerate(pick):
                want, _ = oracle.decode(streams[i], och)
                got = d_p[k * stride_p:k * stride_p + descs[i][0] * descs[i][1] * och].cpu().numpy()
                assert np.array_equal(got, want), (seg, fused, rep, och, i)
    c.close()


@pytest.mark.parametrize("env", [{}, {"QOIMI_DEC_CLASS_SPLIT": "0"}, {"QOIMI_DEC_REC_CAP_MB": "1"}, {"QOIMI_SEG_BYTES": "256"}])
def test_mixed_call_class_by_class(api, oracle, env):
    """A call of more than four images that mixes flat images (UI frames, constant frames) with others is decoded class by class, each
    class at the segment size of its own bytes; an image's place in the caller's buffers travels in the image table.  Eleven images of
    different shapes, the classes interleaved, a flat stream cut short (its last pixel repeated, qoi.h:544) and a photograph's stream cut
    short; 3- and 4-channel output; twice on one context; against the reference decoder.  Also as one pass over everything (round 5), with
    the record arena capped (sub-batches inside a class) and at a forced segment size."""
    import torch
    from qoi_amd import synth
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        c = api.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    shapes = [("photo", 640, 360), ("uiflat", 800, 600), ("noise", 120, 90), ("constant", 512, 512), ("sprite_alpha", 333, 251), ("uiflat", 1280, 720),
              ("photo_hard", 400, 300), ("constant", 31, 17), ("photo", 97, 3)]
    streams, descs = [], []
    for i, (kind, w, h) in enumerate(shapes):
        streams.append(oracle.encode(synth.frame_rgba(kind, w, h, 90 + i), w, h, 4)); descs.append((w, h))
    streams.append(streams[1][:len(streams[1]) // 2] + streams[1][-8:]); descs.append(descs[1])          # a flat stream cut short
    streams.append(streams[0][:len(streams[0]) // 3] + streams[0][-8:]); descs.append(descs[0])
    n = len(streams)
    stride_s = (max(len(s) for s in streams) + 255) // 256 * 256
    stride_p = (max(w * h for w, h in descs) * 4 + 255) // 256 * 256
    stream = torch.cuda.current_stream().cuda_stream
    d_s = torch.zeros(n * stride_s, dtype=torch.uint8, device="cuda")
    for k in range(n):
        d_s[k * stride_s:k * stride_s + len(streams[k])] = torch.frombuffer(bytearray(streams[k]), dtype=torch.uint8).cuda()
    for rep in range(2):
        for och in (4, 3):
            d_p = torch.full((n * stride_p + 64,), 0xA5, dtype=torch.uint8, device="cuda")
            c.decode_batch(d_s.data_ptr(), stride_s, [len(s) for s in streams], [api.QoiDesc(w, h, 4, 0) for w, h in descs], och, d_p.data_ptr(), stride_p, stream)
            host = d_p.cpu().numpy()
            for k in range(n):
                want, _ = oracle.decode(streams[k], och)
                got = host[k * stride_p:k * stride_p + descs[k][0] * descs[k][1] * och]
                assert np.array_equal(got, want), (env, rep, och, k)
                tail = host[k * stride_p + descs[k][0] * descs[k][1] * och:(k + 1) * stride_p]
                assert (tail == 0xA5).all(), ("wrote behind the image", env, och, k)
    c.close()


def test_small_calls_adapt_to_the_previous_call(api, oracle):
    """What a call of a few images learns from the one before it on the same context: a frame with long runs by the thousand (a sprite's
    transparent bands) makes the next call leave run descriptors for dec_expand_runs, a call whose transcoder could not synchronise every
    segment (a stream of equally long multi-byte chunks built against it) makes the next one take the chains at once; both switch back.
    Sprite, photograph, the hostile stream, sprite, sprite, photograph ... on one context, 3- and 4-channel output, against the reference
    decoder every time."""
    import torch
    from qoi_amd import synth
    c = api.Context(0)
    items = []
    for kind, w, h, seed in [("sprite_alpha", 1600, 900, 11), ("photo", 640, 360, 12), ("noise", 256, 200, 13)]:
        items.append((oracle.encode(synth.frame_rgba(kind, w, h, seed), w, h, 4), w, h))
    # QOI_OP_RGBA chunks whose alpha byte reads as another QOI_OP_RGBA tag: five chains that never meet, whatever the run-up
    w, h = 300, 200
    hostile = bytearray(b"qoif" + w.to_bytes(4, "big") + h.to_bytes(4, "big") + bytes([4, 0]))
    for i in range(w * h):
        hostile += bytes([0xFF, (i * 7) & 0xFF, 0xFF, (i * 13) & 0xFF, 0xFF])
    hostile += bytes([0, 0, 0, 0, 0, 0, 0, 1])
    items.append((bytes(hostile), w, h))
    order = [0, 1, 3, 0, 0, 1, 2, 3, 1, 0]
    stream = torch.cuda.current_stream().cuda_stream
    for rep, k in enumerate(order):
        st, w, h = items[k]
        for och in (4, 3):
            d_s = torch.frombuffer(bytearray(st) + bytearray(64), dtype=torch.uint8).cuda()
            d_p = torch.full((w * h * och + 64,), 0xA5, dtype=torch.uint8, device="cuda")
            c.decode_batch(d_s.data_ptr(), d_s.numel(), [len(st)], [api.QoiDesc(w, h, 4, 0)], och, d_p.data_ptr(), w * h * och + 64, stream)
            want, _ = oracle.decode(st, och)
            got = d_p.cpu().numpy()
            assert np.array_equal(got[:w * h * och], want), (rep, k, och)
            assert (got[w * h * och:] == 0xA5).all(), ("wrote behind the image", rep, k, och)
    c.close()


def test_small_calls_on_alternating_streams(api, oracle):
    """A call of a few images returns on the result words its last launch writes to pinned memory; that launch (it zeroes the counter
    header for the context's next call) may still be retiring.  One context, calls in turn on two streams and on the default stream, no
    waits in between on the caller's side, photographs and noise (the noise call falls back to the chains and leaves no zeroed header):
    every image exact - the context waits for the previous call's stream by itself when the stream changes."""
    import torch
    from qoi_amd import synth
    c = api.Context(0)
    w, h = 1024, 768
    items = []
    for i, kind in enumerate(["photo", "photo_hard", "noise", "photo", "uiflat"]):
        px = synth.frame_rgba(kind, w, h, 900 + i)
        st = oracle.encode(px, w, h, 4)
        items.append((torch.frombuffer(bytearray(st + b"\0" * 8), dtype=torch.uint8).cuda(), len(st), torch.from_numpy(px.reshape(-1).copy()).cuda()))
    streams = [torch.cuda.Stream(), torch.cuda.Stream(), None]
    outs = [torch.empty(w * h * 4, dtype=torch.uint8, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    for it in range(90):
        k = it % 3
        d_s, n, want = items[(it * 7) % len(items)]
        handle = streams[k].cuda_stream if streams[k] is not None else 0
        outs[k].fill_(0x5A) if it % 11 == 0 else None
        torch.cuda.synchronize() if it % 11 == 0 else None
        c.decode_batch(d_s.data_ptr(), d_s.numel(), [n], [api.QoiDesc(w, h, 4, 0)], 4, outs[k].data_ptr(), w * h * 4, handle)
        torch.cuda.synchronize()
        assert torch.equal(outs[k], want), (it, k)
    c.close()


def test_differential_fuzz(api, oracle):
    """tests/fuzz_decode.py (qoifuzz.c's input convention, but results are compared with the oracle):
    mutated / truncated / spliced streams, every `channels` argument incl. invalid ones."""
    sys_path = os.path.dirname(os.path.abspath(__file__))
    import importlib.util
    spec = importlib.util.spec_from_file_location("fuzz_decode", os.path.join(sys_path, "fuzz_decode.py"))
    fz = importlib.util.module_from_spec(spec); spec.loader.exec_module(fz)
    assert fz.run(300, 20260922, api=api, oracle=oracle) == 0


def test_decode_batch_mixed_shapes(api, ctx, oracle):
    """One decode batch of differently shaped images (incl. a truncated and a 22-byte stream), 3- and 4-channel output."""
    import torch
    from qoi_amd import synth
    shapes = [(640, 360, "photo"), (97, 1, "noise"), (1, 211, "uiflat"), (1030, 517, "constant"), (333, 444, "photo")]
    streams, descs = [], []
    for i, (w, h, kind) in enumerate(shapes):
        s = oracle.encode(synth.frame_rgba(kind, w, h, 60 + i), w, h, 4)
        if i == 4:
            s = s[:len(s) // 2]                         # truncated: remaining pixels repeat the last one (qoi.h:544)
        streams.append(s); descs.append(api.QoiDesc(w, h, 4, 0))
    streams.append(b"qoif" + (5).to_bytes(4, "big") + (3).to_bytes(4, "big") + bytes([4, 0]) + b"\0" * 7 + b"\x01")
    descs.append(api.QoiDesc(5, 3, 4, 0))
    sstride = (max(len(s) for s in streams) + 8 + 255) // 256 * 256
    for och in (4, 3):
        pstride = (max(d.width * d.height for d in descs) * och + 255) // 256 * 256
        buf = torch.zeros(len(streams) * sstride, dtype=torch.uint8, device="cuda")
        for i, s in enumerate(streams):
            buf[i * sstride:i * sstride + len(s)] = torch.from_numpy(np.frombuffer(s, dtype=np.uint8).copy()).cuda()
        out = torch.full((len(streams) * pstride,), 0xCD, dtype=torch.uint8, device="cuda")
        ctx.decode_batch(buf.data_ptr(), sstride, [len(s) for s in streams], descs, och, out.data_ptr(), pstride)
        for i, s in enumerate(streams):
            want, _ = oracle.decode(s, och)
            got = out[i * pstride:i * pstride + want.size].cpu().numpy()
            assert np.array_equal(got, want), (och, i, shapes[i] if i < len(shapes) else "size22")
            if want.size < pstride:
                assert int(out[i * pstride + want.size]) == 0xCD, "wrote past the image"


@pytest.mark.parametrize("slabs", [None, "2"])
def test_encode_images_mixed_shapes(api, oracle, slabs):
    """qoimi_encode_images: 60 images of 60 different shapes, 3 and 4 channels, every synthetic content class (flat ones take the
    summary passes), odd pixel / stream offsets - ONE call, every stream byte-identical to the reference encoder's; then all of the
    streams back through ONE qoimi_decode_batch call (4-channel output)."""
    import torch
    from qoi_amd import synth
    if slabs is not None:
        os.environ["QOIMI_ENC_SET_SLABS"] = slabs
    try:
        c = api.Context(0)
        rng = np.random.default_rng(77)
        shapes = [(1, 1), (1, 1500), (1023, 1), (1024, 1), (1025, 3), (64, 48), (3072, 1), (3073, 2), (1920, 1080), (2500, 1300), (640, 360), (37, 23)]
        while len(shapes) < 60:
            w, h = int(rng.integers(1, 1400)), int(rng.integers(1, 700))
            if (w, h) not in shapes:
                shapes.append((w, h))
        imgs, descs, pix_off, str_off = [], [], [], []
        po = so = 0
        for i, (w, h) in enumerate(shapes):
            ch = 3 if i % 3 == 1 else 4
            kind = synth.KINDS[i % len(synth.KINDS)]
            f = np.ascontiguousarray(synth.frame_rgba(kind, w, h, 500 + i)[:, :, :ch]).reshape(-1)
            po += int(rng.integers(0, 7)); so += int(rng.integers(0, 7))         # no alignment is promised for either
            imgs.append(f); descs.append(api.QoiDesc(w, h, ch, i & 1)); pix_off.append(po); str_off.append(so)
            po += f.size; so += api.encode_bound(w, h, ch)
        d_pix = torch.zeros(po + 64, dtype=torch.uint8, device="cuda")
        d_str = torch.full((so + 64,), 0xEE, dtype=torch.uint8, device="cuda")
        d_len = torch.zeros(len(shapes), dtype=torch.int32, device="cuda")
        for f, o in zip(imgs, pix_off):
            d_pix[o:o + f.size].copy_(torch.from_numpy(f))
        st = torch.cuda.current_stream().cuda_stream
        for rep in range(2):                                                    # twice: the second call reuses the arena
            c.encode_images(d_pix.data_ptr(), pix_off, descs, d_str.data_ptr(), str_off, d_len.data_ptr(), st)
            c.encode_status(st)
            lens = d_len.cpu().numpy()
            host = d_str.cpu().numpy()
            for i, (w, h) in enumerate(shapes):
                want = bytearray(oracle.encode(imgs[i], w, h, descs[i].channels))
                want[13] = descs[i].colorspace                                   # (the oracle helper encodes with colorspace 0)
                got = host[str_off[i]:str_off[i] + int(lens[i])].tobytes()
                assert got == bytes(want), (rep, i, shapes[i], descs[i].channels, synth.KINDS[i % len(synth.KINDS)], int(lens[i]), len(want))
        # the streams back, all shapes in one decode call
        sstride = max(int(x) for x in lens) + 64
        pstride = max(w * h for w, h in shapes) * 4 + 16
        buf = torch.zeros(len(shapes) * sstride, dtype=torch.uint8, device="cuda")
        for i in range(len(shapes)):
            buf[i * sstride:i * sstride + int(lens[i])].copy_(d_str[str_off[i]:str_off[i] + int(lens[i])])
        out = torch.full((len(shapes) * pstride,), 0xAB, dtype=torch.uint8, device="cuda")
        c.decode_batch(buf.data_ptr(), sstride, [int(x) for x in lens], descs, 4, out.data_ptr(), pstride, st)
        ho = out.cpu().numpy()
        for i, (w, h) in enumerate(shapes):
            px = imgs[i].reshape(-1, descs[i].channels)
            want = np.concatenate([px, np.full((w * h, 1), 255, dtype=np.uint8)], axis=1) if descs[i].channels == 3 else px
            assert np.array_equal(ho[i * pstride:i * pstride + w * h * 4], want.reshape(-1)), (i, shapes[i])
        c.close()
    finally:
        if slabs is not None:
            del os.environ["QOIMI_ENC_SET_SLABS"]


def test_decode_streams_gigabytes_apart(api, ctx, oracle):
    """Small streams 2.5 GiB apart in one batch: the lanes of ONE transcoder wavefront then hold streams that its 32-bit buffer
    descriptor does not reach (4 GiB from the wavefront's first stream) - those segments go the way of the unsynchronised ones
    (plain 64-bit addresses) and decode to the same pixels."""
    import torch
    rng = np.random.default_rng(5)
    w, h, n = 64, 40, 4
    stride = 5 << 29                                                       # 2.5 GiB
    imgs = [np.cumsum(rng.integers(-3, 4, size=(w * h, 4)), axis=0).astype(np.uint8) for _ in range(n)]
    streams = [oracle.encode(px, w, h, 4) for px in imgs]
    buf = torch.zeros((n - 1) * stride + 65536, dtype=torch.uint8, device="cuda")
    for i, st in enumerate(streams):
        buf[i * stride:i * stride + len(st)] = torch.from_numpy(np.frombuffer(st, dtype=np.uint8).copy()).cuda()
    out = torch.full((n * w * h * 4 + 8,), 0xAB, dtype=torch.uint8, device="cuda")
    ctx.decode_batch(buf.data_ptr(), stride, [len(st) for st in streams], [api.QoiDesc(w, h, 4, 0)] * n, 4, out.data_ptr(), w * h * 4)
    got = out.cpu().numpy()
    for i in range(n):
        assert np.array_equal(got[i * w * h * 4:(i + 1) * w * h * 4], imgs[i].reshape(-1)), i
    assert int(got[n * w * h * 4]) == 0xAB, "wrote past the last image"
    assert ctx.decode_stats()["sync_fallback_segments"] > 0, "no segment lay out of the descriptor's reach: the test does not test"
    del buf


def test_decode_batch_many_small_images(api, ctx, oracle):
    """300 images of 1..40 pixels a side in ONE decode batch (every per-image chain has a single short group; image
    tables, group bases and the per-image kernels see hundreds of entries), all content classes, both output forms."""
    import torch
    from qoi_amd import synth
    rng = np.random.default_rng(5)
    streams, descs = [], []
    for i in range(300):
        w, h = int(rng.integers(1, 41)), int(rng.integers(1, 41))
        kind = synth.KINDS[i % len(synth.KINDS)]
        px = synth.frame_rgba(kind, w, h, 1000 + i)
        if i % 7 == 3:
            px = px.copy(); px[..., 3] = rng.integers(0, 256, (h, w), dtype=np.uint8)      # busy alpha: RGBA chunks, INDEX alpha changes
        streams.append(oracle.encode(np.ascontiguousarray(px), w, h, 4)); descs.append(api.QoiDesc(w, h, 4, 0))
    sstride = (max(len(s) for s in streams) + 8 + 255) // 256 * 256
    buf = torch.zeros(len(streams) * sstride, dtype=torch.uint8, device="cuda")
    host = np.zeros(len(streams) * sstride, dtype=np.uint8)
    for i, s in enumerate(streams):
        host[i * sstride:i * sstride + len(s)] = np.frombuffer(s, dtype=np.uint8)
    buf.copy_(torch.from_numpy(host))
    for och in (4, 3):
        pstride = (40 * 40 * och + 255) // 256 * 256
        out = torch.full((len(streams) * pstride,), 0xCD, dtype=torch.uint8, device="cuda")
        ctx.decode_batch(buf.data_ptr(), sstride, [len(s) for s in streams], descs, och, out.data_ptr(), pstride)
        got_all = out.cpu().numpy()
        for i, s in enumerate(streams):
            want, _ = oracle.decode(s, och)
            assert np.array_equal(got_all[i * pstride:i * pstride + want.size], want), (och, i, descs[i].width, descs[i].height)
            assert got_all[i * pstride + want.size] == 0xCD or want.size == pstride, "wrote past the image"


def _hostile_stream(n_chunks, w, h):
    """QOI_OP_INDEX on slots whose content does not hash there (never-written slots hold {0,0,0,0}, which hashes to 0), mixed
    with relative chunks: every segment's slot speculation is wrong, the repair loop would verify one segment per round."""
    import struct
    body = bytearray()
    for i in range(n_chunks):
        k = i % 11
        body.append((5 + 3 * (i % 7)) if k in (0, 3, 7) else 0x6A + (i % 5) if k in (1, 4, 8) else 0xC0 + (i % 3) if k == 5 else (0x20 + i % 13))
    return b"qoif" + struct.pack(">II", w, h) + bytes([4, 0]) + bytes(body) + bytes([0, 0, 0, 0, 0, 0, 0, 1])


@pytest.mark.parametrize("rounds", ["1", "3"])
def test_decode_repair_loop_is_bounded(api, oracle, rounds):
    """a stream that defeats the speculation in every segment must not cost a round per segment.  With the round
    limit forced down the sequential last resort (dec_sequential) finishes the image - bit-exact like everything else."""
    import torch
    from qoi_amd import synth
    os.environ["QOIMI_DEC_MAX_ROUNDS"] = rounds
    os.environ["QOIMI_SEG_BYTES"] = "128"
    try:
        c = api.Context(0)
        w, h = 512, 300
        streams = [_hostile_stream(60000, w, h), oracle.encode(synth.frame_rgba("uiflat", w, h, 101), w, h, 4),
                   oracle.encode(synth.frame_rgba("photo", w, h, 5), w, h, 4)]
        sstride = (max(len(s) for s in streams) + 8 + 255) // 256 * 256
        host = np.zeros(len(streams) * sstride, dtype=np.uint8)
        for i, s in enumerate(streams):
            host[i * sstride:i * sstride + len(s)] = np.frombuffer(s, dtype=np.uint8)
        buf = torch.from_numpy(host).cuda()
        for och in (4, 3):
            pstride = (w * h * och + 255) // 256 * 256
            out = torch.full((len(streams) * pstride,), 0xCD, dtype=torch.uint8, device="cuda")
            c.decode_batch(buf.data_ptr(), sstride, [len(s) for s in streams], [api.QoiDesc(w, h, 4, 0)] * len(streams), och, out.data_ptr(), pstride)
            st = c.decode_stats()
            assert st["rounds"] <= int(rounds), st
            got = out.cpu().numpy()
            for i, s in enumerate(streams):
                want, _ = oracle.decode(s, och)
                assert np.array_equal(got[i * pstride:i * pstride + want.size], want), (och, i)
        c.close()
    finally:
        del os.environ["QOIMI_DEC_MAX_ROUNDS"]
        del os.environ["QOIMI_SEG_BYTES"]


@pytest.mark.parametrize("env", [{}, {"QOIMI_ENC_WARM": "0"}, {"QOIMI_ENC_LOOKBACK": "0"}, {"QOIMI_ENC_SET_SLABS": "4"},
                                 {"QOIMI_ENC_SET_SLABS": "2", "QOIMI_ENC_LOOKBACK": "0"}, {"QOIMI_ENC_LOOKBACK": "2"}, {"QOIMI_ENC_LOOKBACK": "1"},
                                 {"QOIMI_ENC_LOOKBACK": "1", "QOIMI_ENC_SET_SLABS": "4"}, {"QOIMI_ENC_G2": "0"}, {"QOIMI_ENC_G2": "0", "QOIMI_ENC_LOOKBACK": "2"},
                                 {"QOIMI_ENC_TREE_TICKET": "0", "QOIMI_ENC_LOOKBACK": "2"}, {"QOIMI_ENC_UNI": "1"}, {"QOIMI_ENC_UNI": "1", "QOIMI_ENC_LOOKBACK": "2"}])
def test_flat_frames_byte_identical(api, oracle, env):
    """Flat UI frames go through the generic entry-state path (per-slab summaries + scans).  Frame 60 of this sweep was
    encoded three bytes too long by every path until round 2: a 64-bit lane mask lost its upper half (sign extension of
    readfirstlane) whenever hash slot 31 had been written in a slab's group, and 32 slots of the entry table came out as zero -
    decodable, round-trip exact, but not the reference's bytes.  The sweep keeps that class of error visible."""
    import torch
    from gpu_util import DeviceBatch
    from qoi_amd import synth
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        c = api.Context(0)
        w, h, n = 1024, 600, 8
        b = DeviceBatch(c, w, h, 4, n)
        for base in (40, 56, 72):
            frames = [synth.frame_rgba("uiflat", w, h, base + i) for i in range(n)]
            for i in range(n):
                b.upload(i, frames[i])
            lens = b.encode()
            torch.cuda.synchronize()
            for i in range(n):
                want = oracle.encode(frames[i], w, h, 4)
                assert b.stream_bytes(i, lens[i]) == want, (env, base + i, int(lens[i]), len(want))
        c.close()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def test_state_lookback_granules_across_calls_and_shapes(api, oracle):
    """The state look-back's granules (enc_sets<ENTRY 2>) are told apart by the call's number and zeroed only where they come to lie
    somewhere new: one context, flat images, shapes and batch sizes alternating from call to call (tree and look-back placement, the
    arena growing in between) - every stream the reference's, call after call."""
    import torch
    from gpu_util import DeviceBatch
    from qoi_amd import synth
    c = api.Context(0)
    plan = [(640, 360, 2), (1024, 600, 9), (640, 360, 2), (640, 360, 2), (1024, 600, 9), (1920, 1080, 3), (1024, 600, 9), (1024, 600, 9), (37, 23, 1), (1024, 600, 12)]
    kinds = ["uiflat", "constant", "sprite_alpha", "uiflat", "photo"]
    for call, (w, h, n) in enumerate(plan):
        b = DeviceBatch(c, w, h, 4, n)
        frames = [synth.frame_rgba(kinds[(call + i) % len(kinds)], w, h, 700 + 13 * call + i) for i in range(n)]
        if call % 3 == 2:                                  # a letterboxed frame: opens with rows of the start value, ends in a long run
            frames[0] = frames[0].copy(); frames[0][: h // 3] = (0, 0, 0, 255); frames[0][-(h // 4):] = (9, 9, 9, 255)
        for i, f in enumerate(frames):
            b.upload(i, f)
        lens = b.encode()
        for i, f in enumerate(frames):
            assert b.stream_bytes(i, lens[i]) == oracle.encode(f, w, h, 4), (call, i, w, h, n)
    c.close()


def test_batches_behind_a_batch_of_flagged_images_only(api, oracle):
    """A look-back batch whose images were ALL sent to the pass over flagged images tells the context's next batch to run its first pass
    with a sixteenth of the workgroups (each looks at sixteen units: they will most likely find flags only).  Flat batches in a row, then
    photographs behind them (several sets per wavefront for once), then photographs again: every stream the reference's."""
    from gpu_util import DeviceBatch
    from qoi_amd import synth
    c = api.Context(0)
    w, h, n = 1024, 600, 9
    for call, kind in enumerate(["uiflat", "uiflat", "constant", "photo", "photo", "sprite_alpha", "sprite_alpha", "uiflat"]):
        b = DeviceBatch(c, w, h, 4, n)
        frames = [synth.frame_rgba(kind, w, h, 5200 + 17 * call + i) for i in range(n)]
        for i, f in enumerate(frames):
            b.upload(i, f)
        lens = b.encode()
        for i, f in enumerate(frames):
            assert b.stream_bytes(i, lens[i]) == oracle.encode(f, w, h, 4), (call, kind, i)
    c.close()


def test_small_calls_take_one_pass_behind_a_call_that_met_flat_stretches(api, oracle):
    """Calls of a few images (tree placement): the first set of a call whose look-back window does not determine its entry state leaves
    the call's number in a pinned host word, the first set of every such call the number of the call that has started in the word behind
    it; while the two are less than eight calls apart the small calls run the one-pass kernel (no second launch over flagged images),
    eight calls of photographs later the two passes are back.  Which kernel ran shows in the profile; the streams are the reference's
    either way."""
    from gpu_util import DeviceBatch
    from qoi_amd import synth
    c = api.Context(0)
    w, h = 1280, 720
    seq = ["photo", "uiflat", "uiflat", "constant"] + ["photo"] * 12 + ["sprite_alpha", "sprite_alpha"]
    second_pass = []
    for call, kind in enumerate(seq):
        b = DeviceBatch(c, w, h, 4, 1)
        f = synth.frame_rgba(kind, w, h, 4100 + call)
        b.upload(0, f)
        c.set_profiling(True)
        lens = b.encode()
        prof = c.get_profile(b.stream)
        c.set_profiling(False)
        assert b.stream_bytes(0, lens[0]) == oracle.encode(f, w, h, 4), (call, kind)
        second_pass.append(prof.get("enc_slabs_generic", (0.0, 0))[1] > 0)          # (two passes: the second launch is there even where it finds nothing to do)
    # photo, uiflat: two passes (nothing known yet); one pass up to the eighth call behind the constant frame (call 3); the first sprite finds two passes again
    want = [True, True] + [False] * 2 + [False] * 8 + [True] * 4 + [True, False]
    assert second_pass == want, second_pass
    c.close()


@pytest.mark.parametrize("env", [{}, {"QOIMI_ENC_SPREAD": "0"}])
def test_random_sweep_of_contents_and_shapes(api, oracle, env):
    """A seeded sweep over every synthetic content kind at shapes from a few pixels to several 64-slab groups, 3 and 4 channels:
    encode byte-identical to the reference, decode of that stream bit-identical to the pixels.  (The fixed shapes of the other
    tests never put hash slot 31 into the entry path that lost its upper mask half; a sweep would have.)"""
    import torch
    from gpu_util import DeviceBatch
    from qoi_amd import synth
    rng = np.random.default_rng(20260923)
    shapes = [(1, 1), (3, 2), (64, 16), (65, 17), (1023, 1), (1, 1025), (257, 255), (640, 360), (1024, 600), (1400, 900), (2048, 130)]
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)                      # (read when the context is created)
    try:
        c = api.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    checked = 0
    for (w, h) in shapes:
        for ch in (4, 3):
            n = 5
            kinds = [synth.KINDS[int(k)] for k in rng.integers(0, len(synth.KINDS), n)]
            seeds = [int(x) for x in rng.integers(0, 1 << 20, n)]
            frames = [np.ascontiguousarray(synth.frame_rgba(kinds[i], w, h, seeds[i])[:, :, :ch]) for i in range(n)]
            b = DeviceBatch(c, w, h, ch, n)
            for i in range(n):
                b.upload(i, frames[i])
            lens = b.encode()
            torch.cuda.synchronize()
            for i in range(n):
                want = oracle.encode(frames[i], w, h, ch)
                assert b.stream_bytes(i, lens[i]) == want, ("encode", w, h, ch, kinds[i], seeds[i], int(lens[i]), len(want))
            out = torch.full((n * b.pixel_stride,), 0xCD, dtype=torch.uint8, device="cuda")
            stride = b.decode_into(out, lens, ch)
            got = out.cpu().numpy()
            for i in range(n):
                assert np.array_equal(got[i * stride:i * stride + w * h * ch], frames[i].reshape(-1)), ("decode", w, h, ch, kinds[i], seeds[i])
                checked += 1
    c.close()
    assert checked == len(shapes) * 2 * 5


@pytest.mark.parametrize("slabs", [1, 2, 3, 4, 5, 8])
@pytest.mark.parametrize("lookback", ["1", "0", "nospread", "2"])
def test_set_sizes_and_placements(api, oracle, slabs, lookback):
    """A wavefront encodes a SET of R consecutive slabs (R = 1..8; the library picks it from the batch size, here it is forced) and
    places its bytes by look-back (bytes beyond the staging buffer spill through the set's scratch slot), by the tree of byte
    counts ("2") or order-free.  Shapes
    with a partial last set / last group / last step, every content class in 3 and 4 channels: byte-identical to the reference."""
    import torch
    from gpu_util import DeviceBatch
    from qoi_amd import synth
    old = {k: os.environ.get(k) for k in ("QOIMI_ENC_SET_SLABS", "QOIMI_ENC_LOOKBACK", "QOIMI_ENC_SPREAD")}
    os.environ["QOIMI_ENC_SET_SLABS"] = str(slabs)
    os.environ["QOIMI_ENC_LOOKBACK"] = "1" if lookback == "nospread" else lookback
    os.environ["QOIMI_ENC_SPREAD"] = "0" if lookback == "nospread" else "1"
    try:
        c = api.Context(0)
        for (w, h) in ((1400, 900), (517, 313), (64, 9), (1024, 16)):
            for ch in (4, 3):
                kinds = ["photo", "noise", "uiflat", "constant", "photo", "noise"]
                n = len(kinds)
                frames = [np.ascontiguousarray(synth.frame_rgba(kinds[i], w, h, 300 + 7 * i + slabs)[:, :, :ch]) for i in range(n)]
                if ch == 4:
                    frames[4] = frames[4].copy(); frames[4][::3, ::5, 3] = 128          # alpha changes: QOI_OP_RGBA among short chunks
                b = DeviceBatch(c, w, h, ch, n)
                for i in range(n):
                    b.upload(i, frames[i])
                lens = b.encode()
                torch.cuda.synchronize()
                for i in range(n):
                    want = oracle.encode(frames[i], w, h, ch)
                    assert b.stream_bytes(i, lens[i]) == want, (slabs, lookback, w, h, ch, kinds[i], int(lens[i]), len(want))
        c.close()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _mixed_frame(rng, w, h, ch, seed):
    """A photograph with stretches of noise, flat colour, alpha steps and every-other-pixel noise: bytes per pixel change inside
    a set, so look-back sets spill part of their bytes and keep the rest staged."""
    from qoi_amd import synth
    a = synth.frame_rgba("photo", w, h, seed).reshape(-1, 4).copy()
    b = synth.frame_rgba("noise", w, h, seed + 1).reshape(-1, 4)
    n, pos = a.shape[0], 0
    while pos < n:
        L, k = int(rng.integers(1, 6000)), int(rng.integers(0, 5))
        if k == 1:
            a[pos:pos + L] = b[pos:pos + L]
        elif k == 2:
            a[pos:pos + L] = a[pos]
        elif k == 3:
            a[pos:pos + L, 3] = rng.integers(0, 256)
        elif k == 4:
            a[pos:pos + L:2] = b[pos:pos + L:2]
        pos += L
    return np.ascontiguousarray(a.reshape(h, w, 4)[:, :, :ch])


@pytest.mark.parametrize("env", [{}, {"QOIMI_ENC_LOOKBACK": "1"}, {"QOIMI_ENC_SET_SLABS": "3", "QOIMI_ENC_LOOKBACK": "1"}, {"QOIMI_ENC_SET_SLABS": "8", "QOIMI_ENC_LOOKBACK": "1"},
                                 {"QOIMI_ENC_SET_SLABS": "4", "QOIMI_ENC_LOOKBACK": "0"},
                                 {"QOIMI_ENC_SPREAD": "0", "QOIMI_ENC_LOOKBACK": "1"}, {"QOIMI_ENC_SPREAD": "0", "QOIMI_ENC_SET_SLABS": "3", "QOIMI_ENC_LOOKBACK": "1"},
                                 {"QOIMI_ENC_LOOKBACK": "2", "QOIMI_ENC_SET_SLABS": "1"}, {"QOIMI_ENC_LOOKBACK": "2", "QOIMI_ENC_SET_SLABS": "3"}])
def test_mixed_content_partial_spills(api, oracle, env):
    """Sets whose bytes only partly fit the LDS staging buffer ."""
    import torch
    from gpu_util import DeviceBatch
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        c = api.Context(0)
        rng = np.random.default_rng(31)
        for (w, h, ch) in ((1920, 1080, 4), (1000, 999, 3), (4096, 33, 4)):
            n = 6
            frames = [_mixed_frame(rng, w, h, ch, 2000 + i) for i in range(n)]
            b = DeviceBatch(c, w, h, ch, n)
            for i in range(n):
                b.upload(i, frames[i])
            lens = b.encode()
            torch.cuda.synchronize()
            for i in range(n):
                want = oracle.encode(frames[i], w, h, ch)
                assert b.stream_bytes(i, lens[i]) == want, (env, w, h, ch, i, int(lens[i]), len(want))
            out = torch.full((n * b.pixel_stride,), 0xCD, dtype=torch.uint8, device="cuda")
            stride = b.decode_into(out, lens, ch)
            got = out.cpu().numpy()
            for i in range(n):
                assert np.array_equal(got[i * stride:i * stride + w * h * ch], frames[i].reshape(-1)), (env, w, h, ch, i)
        c.close()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def test_one_context_through_changing_content(api, oracle):
    """One context encodes noise, noise, photo, photo, noise, flat frames in turn (workspace layout and placement stay the
    same from call to call); every stream stays byte-identical to the reference's."""
    import torch
    from gpu_util import DeviceBatch
    from qoi_amd import synth
    c = api.Context(0)
    w, h, n = 1024, 600, 3
    b = DeviceBatch(c, w, h, 4, n)
    for step, kind in enumerate(("noise", "noise", "noise", "photo", "photo", "noise", "uiflat")):
        frames = [synth.frame_rgba(kind, w, h, 40 + step * 3 + i) for i in range(n)]
        for i in range(n):
            b.upload(i, frames[i])
        lens = b.encode()
        torch.cuda.synchronize()
        for i in range(n):
            want = oracle.encode(frames[i], w, h, 4)
            got = b.stream_bytes(i, lens[i])
            assert got == want, (step, kind, i, len(got), len(want))
    c.close()


def test_flat_ui_frames_verify_in_few_rounds(api, oracle):
    """UI frames whose alpha levels go through the colour table: the refinement passes (P3 + S3 repeated, and appended to the
    first round for flat images) keep them at a handful of rounds - they took 13 with one pass per round.  Checked for the
    passes switched off as well (more rounds, the same pixels)."""
    import torch
    from qoi_amd import synth
    w, h, n = 1920, 1080, 6
    streams = [oracle.encode(synth.frame_rgba("uiflat", w, h, 80 + i), w, h, 4) for i in range(n)]
    sstride = (max(len(s) for s in streams) + 8 + 255) // 256 * 256
    host = np.zeros(n * sstride, dtype=np.uint8)
    for i, s in enumerate(streams):
        host[i * sstride:i * sstride + len(s)] = np.frombuffer(s, dtype=np.uint8)
    want = [oracle.decode(s, 4)[0] for s in streams]
    rounds = {}
    for env in ({}, {"QOIMI_DEC_INNER": "1", "QOIMI_DEC_INNER1": "0"}):
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        os.environ["QOIMI_SEG_BYTES"] = "512"
        try:
            c = api.Context(0)
            buf = torch.from_numpy(host).cuda()
            pstride = (w * h * 4 + 255) // 256 * 256
            out = torch.full((n * pstride,), 0xCD, dtype=torch.uint8, device="cuda")
            c.decode_batch(buf.data_ptr(), sstride, [len(s) for s in streams], [api.QoiDesc(w, h, 4, 0)] * n, 4, out.data_ptr(), pstride)
            rounds[len(env)] = c.decode_stats()["rounds"]
            got = out.cpu().numpy()
            for i in range(n):
                assert np.array_equal(got[i * pstride:i * pstride + want[i].size], want[i]), (env, i)
            c.close()
        finally:
            del os.environ["QOIMI_SEG_BYTES"]
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
    assert rounds[0] <= 6 and rounds[0] <= rounds[2], rounds


def test_hostile_stream_finishes_in_bounded_rounds(api, ctx, oracle):
    """The same hostile stream with the default limits: the number of rounds stays below the limit of the library however
    many segments mis-speculate (round 1 would have taken one round per segment: thousands)."""
    import torch
    w, h = 1024, 600
    s = _hostile_stream(500000, w, h)
    buf = torch.from_numpy(np.frombuffer(s + b"\0" * 8, dtype=np.uint8).copy()).cuda()
    out = torch.full((w * h * 4 + 8,), 0xCD, dtype=torch.uint8, device="cuda")
    ctx.decode_batch(buf.data_ptr(), buf.numel(), [len(s)], [api.QoiDesc(w, h, 4, 0)], 4, out.data_ptr(), w * h * 4)
    assert ctx.decode_stats()["rounds"] <= 6          # two rounds in a row without progress: the rest is decoded sequentially
    want, _ = oracle.decode(s, 4)
    assert np.array_equal(out[:w * h * 4].cpu().numpy(), want)


def test_decode_batch_over_65535_images(api, ctx, oracle):
    """70 000 tiny images in one decode call (a grid dimension of round 1 stopped at 65 535), a third of them truncated so
    that the tail fill (qoi.h:544) runs for them."""
    import torch
    rng = np.random.default_rng(11)
    protos = []
    for k in range(7):
        px = rng.integers(0, 256, size=(3, 3, 4), dtype=np.uint8)
        if k % 2:
            px[:, :, 3] = 255
        s = oracle.encode(np.ascontiguousarray(px), 3, 3, 4)
        if k % 3 == 0:
            s = s[:14 + (len(s) - 22) // 2] + s[-8:]                    # half of the chunks, then the end marker
        protos.append((s, oracle.decode(s, 4)[0]))
    n = 70000
    sstride = 256
    host = np.zeros(n * sstride, dtype=np.uint8)
    sizes = []
    for i in range(n):
        s = protos[i % 7][0]
        host[i * sstride:i * sstride + len(s)] = np.frombuffer(s, dtype=np.uint8)
        sizes.append(len(s))
    buf = torch.from_numpy(host).cuda()
    descs = [api.QoiDesc(3, 3, 4, 0)] * n
    pstride = 256
    out = torch.full((n * pstride,), 0xCD, dtype=torch.uint8, device="cuda")
    ctx.decode_batch(buf.data_ptr(), sstride, sizes, descs, 4, out.data_ptr(), pstride)
    got = out.cpu().numpy().reshape(n, pstride)
    for k in range(7):
        assert (got[k::7, :36] == protos[k][1][None, :]).all(), k
    assert (got[:, 36:] == 0xCD).all(), "wrote past an image"


@pytest.mark.parametrize("shape", [(1, 1), (7, 3), (63, 65), (1024, 1), (1, 1025), (257, 129)])
def test_encode_batch_many_small_images(api, ctx, oracle, shape):
    """Batches of 96 small frames of one shape, every content class in turn plus busy-alpha frames: every stream
    byte-identical to the reference's (slabs shorter than a wavefront's 1024 pixels, images of a single slab)."""
    import torch
    from gpu_util import DeviceBatch
    from qoi_amd import synth
    w, h = shape
    n = 96
    b = DeviceBatch(ctx, w, h, 4, n)
    rng = np.random.default_rng(w * 131 + h)
    frames = []
    for i in range(n):
        px = synth.frame_rgba(synth.KINDS[i % len(synth.KINDS)], w, h, 2000 + i).copy()
        if i % 5 == 4:
            px[..., 3] = rng.integers(0, 4, (h, w), dtype=np.uint8) * 85
        frames.append(np.ascontiguousarray(px))
        b.pixels[i * b.pixel_stride:i * b.pixel_stride + w * h * 4] = torch.from_numpy(frames[-1].reshape(-1)).cuda()
    lens = b.encode()
    for i in range(n):
        want = oracle.encode(frames[i], w, h, 4)
        assert int(lens[i]) == len(want), (shape, i)
        assert b.stream_bytes(i, len(want)) == want, (shape, i)


def test_failed_lds_order_recheck_is_counted_and_reported_once(api):
    """The repeat of the LDS exchange-order self-test (qoi_host_encode.hip, qoi_ctx.h: enc_poll_recheck; include/qoi_mi355x.h): forced to fail by the test hook with a
    repeat after every call.  The call that notices is encoded with the order-independent probe and succeeds, the calls made with
    the suspect probe since the last passed check are counted (all of them - the one made before the repeat was launched too),
    and the next qoimi_encode_status reports the event exactly once (tests/hook_scenarios.py: recheck_fail, on the test flavour)."""
    _hook_scenario("recheck_fail")


def test_spilling_sets_share_a_scratch_pool(api, oracle):
    """Look-back placement: sets that outgrow their LDS staging buffer spill to a slot of a POOL (qoi_encode.hip pool_take) instead of a
    worst-case slot per set.  21 600 noise sets - more than the pool's 8192 slots - so slots are handed out again and again inside
    one launch (the bytes a set reads back must be its own, not what this CU's L1 kept of the slot's earlier holder), next to
    photographs that never spill; and the workspace of a larger batch stays far below a slot per set."""
    import torch
    from gpu_util import DeviceBatch
    from qoi_amd import synth
    old = os.environ.get("QOIMI_ENC_SET_SLABS")
    os.environ["QOIMI_ENC_SET_SLABS"] = "1"
    try:
        c = api.Context(0)
        w, h, n = 1280, 720, 26
        b = DeviceBatch(c, w, h, 4, n)
        kinds = ["noise"] * 24 + ["photo", "uiflat"]
        for i in range(n):
            c.synth_frames(synth.KIND_ID[kinds[i]], synth.DEFAULT_SEED, 900 + i, 1, w, h, b.pixels.data_ptr() + i * b.pixel_stride, b.pixel_stride, b.stream)
        for rep in range(2):
            lens = b.encode()
            for i in (0, 7, 13, 23, 24, 25):
                assert b.stream_bytes(i, lens[i]) == oracle.encode(synth.frame_rgba(kinds[i], w, h, 900 + i), w, h, 4), (rep, i)
        out = torch.zeros(n * b.pixel_stride, dtype=torch.uint8, device="cuda")
        b.decode_into(out, lens)
        assert torch.equal(out.view(n, -1)[:, :w * h * 4], b.pixels.view(n, -1)[:, :w * h * 4])
        c.close()
    finally:
        if old is None:
            os.environ.pop("QOIMI_ENC_SET_SLABS", None)
        else:
            os.environ["QOIMI_ENC_SET_SLABS"] = old
    c = api.Context(0)
    w, h, n = 1920, 1080, 128
    b = DeviceBatch(c, w, h, 4, n)
    c.synth_frames(synth.KIND_ID["photo"], synth.DEFAULT_SEED, 0, n, w, h, b.pixels.data_ptr(), b.pixel_stride, b.stream)
    b.encode()
    ws = c.workspace_bytes()["encode"]
    assert ws < 1000 << 20, ws           # state granules and records 0.13 GB + pool 0.67 GB (8193 slots of sixteen worst-case slabs: what a set of the pass
                                         # over flagged images may spill in a call this large; a worst-case slot per set: 1.3 GB more)
    c.close()


def test_encoder_fuzz_short_campaign(api):
    """A short campaign of tests/fuzz_encode.py (random patchwork images, shapes, channel counts, batch sizes 1..12, forced and
    free placement / set sizes): every stream byte-identical to the reference encoder's, every round trip exact.  Longer runs are
    kept under profiles/ (r04_fuzz_encode.txt)."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "fuzz_encode.py"), "--iters", "60", "--seed", "11",
                        "--max-pixels", "3000000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "every stream byte-identical" in r.stdout


def test_encoder_fuzz_batches_of_eight_and_more(api):
    """60 seconds of tests/fuzz_encode.py with 8 or more images in half of the calls: look-back placement with per-image tickets and
    the four wavefronts of a workgroup on consecutive images - the path every benchmark batch takes - against the reference encoder,
    byte for byte."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "fuzz_encode.py"), "--iters", "100000", "--seconds", "60", "--seed", "21",
                        "--batch8-half", "--max-pixels", "2500000"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "every stream byte-identical" in r.stdout


def test_stream_hashes_equal_their_numpy_restatement(api, ctx):
    """qoimi_hash_streams (what bench.py compares whole batches with) against synth.stream_hash64 on streams of odd lengths."""
    import torch
    from qoi_amd import synth
    rng = np.random.default_rng(5)
    n, stride = 9, 5000
    lens = [0, 1, 7, 8, 9, 22, 4095, 4096, 4999]
    host = rng.integers(0, 256, size=n * stride, dtype=np.uint8)
    d = torch.from_numpy(host).cuda()
    dl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    out = torch.zeros(n, dtype=torch.int64, device="cuda")
    ctx.hash_streams(d.data_ptr(), stride, dl.data_ptr(), n, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint64)
    for i in range(n):
        assert int(got[i]) == synth.stream_hash64(host[i * stride:i * stride + lens[i]].tobytes()), i


def test_decoder_batch_fuzz_short_campaign(api):
    """A short campaign of tests/fuzz_decode_batch.py: hostile valid-grammar streams (chunk soups no encoder would write, too short and
    too long for their image) through qoimi_decode_batch in batches, random segment sizes, 3- and 4-channel output - every image equal
    to the reference decoder's.  Longer runs: profiles/r04_fuzz_decode_batch.txt."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "fuzz_decode_batch.py"), "--iters", "60", "--seed", "12"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "every image equal" in r.stdout
