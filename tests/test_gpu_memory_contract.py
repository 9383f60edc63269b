"""The memory contract of the device calls (-m gpu), at the edges the header allows and the other GPU tests never reach: include/
qoi_mi355x.h states no alignment for d_pixels, d_streams or their strides, takes stream_stride == qoimi_encode_bound(desc) with no
slack, and promises that nothing outside an image's or a stream's own range is written.  Here every base is odd, the strides are
minimal (or odd), streams fill their slots to the last byte with the next stream's header right behind them (cases.full_slot_image),
and every buffer is looked at WHOLE: the reference's bytes where they belong, the fill byte everywhere else (gpu_util.EdgeBatch,
gpu_util.GuardedRegion; the mask arithmetic itself is tested without a GPU in tests/test_guard_masks.py).  Expected streams and pixels
come from the `ref` / `port` oracles."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
from gpu_util import GUARD, OUT_FILL, STREAM_FILL, EdgeBatch, GuardedRegion
from gpu_pack import api, oracle  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

SHAPES = [(517, 313), (1025, 3), (7, 3)]          # 159 slabs (three groups of 64 sets, partial last slab and last set) / 4 slabs / a few pixels
ROTATION = ("full", "constant", "uiflat", "photo", "full")      # a full slot in front of another header, a flat image behind a full slot


class Vault:
    """Images by (kind, w, h, ch, k) and what the reference makes of them, each computed once and handed out read-only."""

    def __init__(self, api, oracle):
        self.api, self.oracle = api, oracle
        self._img, self._stream, self._px = {}, {}, {}

    def image(self, kind, w, h, ch, k):
        key = (kind, w, h, ch, k)
        if key not in self._img:
            from qoi_amd import synth
            if kind == "full":
                f = cases.full_slot_image(w, h, ch, k % 3)           # seeds 0..2: checked against the reference below
            else:
                f = synth.frame_rgba(kind, w, h, 20 + k)[:, :, :ch]
            f = np.ascontiguousarray(f).reshape(-1)
            f.setflags(write=False)
            self._img[key] = f
        return self._img[key]

    def stream(self, kind, w, h, ch, k):
        key = (kind, w, h, ch, k)
        if key not in self._stream:
            s = self.oracle.encode(self.image(*key), w, h, ch)
            if kind == "full":
                assert len(s) == self.api.encode_bound(w, h, ch), ("the image does not fill its slot: the test does not test", key, len(s))
            self._stream[key] = s
        return self._stream[key]

    def pixels(self, kind, w, h, ch, k, och):
        key = (kind, w, h, ch, k, och)
        if key not in self._px:
            px, _ = self.oracle.decode(self.stream(kind, w, h, ch, k), och)
            px.setflags(write=False)
            self._px[key] = px
        return self._px[key]

    def batch(self, w, h, ch, n):
        """the keys of a call of n images: the rotation of the module's docstring"""
        return [(ROTATION[k % len(ROTATION)], w, h, ch, k) for k in range(n)]


@pytest.fixture(scope="module")
def vault(api, oracle):
    return Vault(api, oracle)


def context_under(api, env):
    """a context created under `env` (the knobs are read once, by qoimi_ctx_create); the environment is restored at once"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return api.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def odd_offsets(j):
    """three offsets in 1..15 that change from call to call"""
    return 1 + j % 15, 1 + (7 * j + 2) % 15, 1 + (11 * j + 5) % 15


# ------------------------------------------------------------------ qoimi_encode_batch / qoimi_decode_batch
FORMS = [
    {},                                                           # the library's choice: tree for 1 and 3 images, look-back for 9
    {"QOIMI_ENC_LOOKBACK": "0"},                                  # order-free: scratch slot per set, enc_offsets + enc_compact
    {"QOIMI_ENC_LOOKBACK": "1"},                                  # look-back: pool spills, copy-out straight from the LDS
    {"QOIMI_ENC_LOOKBACK": "1", "QOIMI_ENC_SET_SLABS": "1"},
    {"QOIMI_ENC_LOOKBACK": "1", "QOIMI_ENC_SET_SLABS": "3"},
    {"QOIMI_ENC_LOOKBACK": "2"},                                  # tree, units by ticket
    {"QOIMI_ENC_LOOKBACK": "2", "QOIMI_ENC_TREE_TICKET": "0"},    # tree, units by workgroup index
    {"QOIMI_ENC_UNI": "1"},                                       # the one-pass kernel
    {"QOIMI_ENC_PROBE": "0"},                                     # the order-independent colour-table probe
    {"QOIMI_ENC_G2": "0", "QOIMI_ENC_LOOKBACK": "1"},             # flat images through the summary passes
]


def form_id(env):
    return ",".join(f"{k[len('QOIMI_ENC_'):]}={v}" for k, v in env.items()) or "default"


@pytest.mark.parametrize("ch", [4, 3])
@pytest.mark.parametrize("env", FORMS, ids=form_id)
def test_encode_batch_at_the_edges(api, vault, env, ch):
    """Every placement form x 1, 3, 9 images x three shapes x (no slack, odd slack): odd pixel, stream and output bases whose
    `address & 15` differs from image to image, full-slot images in front of other streams' headers and flat images behind them.
    Lengths and stream bytes are the reference's; not a byte in front of the first slot, behind a slot's bound, in the gaps between
    slots or between a stream's end and its slot's bound is written.  The streams then go back through qoimi_decode_batch from where
    they lie into an odd output base with pixel_stride == npx*och exactly, 3- and 4-channel output: the reference decoder's pixels,
    nothing written around the images."""
    c = context_under(api, env)
    try:
        j = 0
        for (w, h) in SHAPES:
            for n in (1, 3, 9):
                for dp, ds in ((0, 0), (5, 7)):
                    j += 1
                    po, so, oo = odd_offsets(j)
                    what = f"{form_id(env)}, {n} x {w}x{h}x{ch}, strides +{dp} +{ds}, bases +{po} +{so} +{oo}"
                    keys = vault.batch(w, h, ch, n)
                    b = EdgeBatch(c, w, h, ch, n, po, so, oo, dp, ds)
                    assert n == 1 or len(set(b.stream_address_residues())) > 1, ("every stream at the same address & 15: the test does not test", what)
                    for i, key in enumerate(keys):
                        b.upload(i, vault.image(*key))
                    lens, host = b.encode()
                    b.check_streams(host, lens, [vault.stream(*key) for key in keys], what + f", stream address & 15 = {b.stream_address_residues()}")
                    for och in (3, 4):
                        out, region = b.decode(lens, och)
                        b.check_pixels(out, region, [vault.pixels(*key, och) for key in keys], what + f", decoded to {och} channels")
    finally:
        c.close()


# ------------------------------------------------------------------ qoimi_encode_images / qoimi_encode_images_packed
MIXED = [("full", 517, 313, 4), ("constant", 64, 48, 4), ("full", 7, 3, 3), ("uiflat", 257, 9, 3), ("photo", 333, 7, 4), ("full", 1025, 3, 4),
         ("uiflat", 640, 360, 4), ("full", 1023, 1, 3), ("photo", 37, 23, 3), ("full", 1, 1, 4), ("constant", 1, 1, 3), ("full", 64, 9, 3),
         ("full", 1024, 16, 4), ("photo", 200, 150, 4), ("full", 517, 313, 3), ("constant", 129, 5, 3), ("full", 1025, 3, 3), ("uiflat", 96, 70, 4)]


def mixed_call(api, vault):
    """-> keys, descriptors, pixel offsets (every residue mod 4 for either channel count), the device pixel buffer"""
    import torch
    keys = [(kind, w, h, ch, i) for i, (kind, w, h, ch) in enumerate(MIXED)]
    descs = [api.QoiDesc(w, h, ch, 0) for (_, w, h, ch, _) in keys]
    seen, pix_off, at = {3: 0, 4: 0}, [], GUARD + 1
    for key in keys:
        ch = key[3]
        at += (seen[ch] - at) % 4                   # the k-th image of a channel count at an address = k (mod 4)
        seen[ch] += 1
        pix_off.append(at)
        at += vault.image(*key).size
    for ch in (3, 4):
        assert {o % 4 for o, key in zip(pix_off, keys) if key[3] == ch} == {0, 1, 2, 3}
    d_pix = torch.zeros(at + GUARD, dtype=torch.uint8, device="cuda")
    assert d_pix.data_ptr() % 16 == 0
    for o, key in zip(pix_off, keys):
        f = vault.image(*key)
        d_pix[o:o + f.size].copy_(torch.from_numpy(f.copy()))
    return keys, descs, pix_off, d_pix


@pytest.mark.parametrize("slabs", [None, "2"])
def test_encode_images_slots_back_to_back(api, vault, slabs):
    """qoimi_encode_images, shapes and channel counts mixed, full-slot images among flat ones and photographs: stream_offsets[i + 1] ==
    stream_offsets[i] + bound_i from an odd first offset - a full slot ends on the byte in front of the next header - pixel offsets at
    every residue mod 4; twice on one context.  The reference's bytes, the fill byte everywhere else."""
    import torch
    c = context_under(api, {} if slabs is None else {"QOIMI_ENC_SET_SLABS": slabs})
    try:
        keys, descs, pix_off, d_pix = mixed_call(api, vault)
        want = [vault.stream(*key) for key in keys]
        bounds = [api.encode_bound(d.width, d.height, d.channels) for d in descs]
        assert sum(len(s) == b for s, b in zip(want, bounds)) >= 8
        starts = [GUARD + 5 + int(x) for x in np.cumsum([0] + bounds[:-1])]
        region = GuardedRegion(starts[-1] + bounds[-1] + GUARD, starts, STREAM_FILL)
        st = torch.cuda.current_stream().cuda_stream
        for rep in range(2):
            d_str = torch.full((region.size,), STREAM_FILL, dtype=torch.uint8, device="cuda")
            d_len = torch.zeros(len(keys), dtype=torch.int32, device="cuda")
            assert d_str.data_ptr() % 16 == 0
            c.encode_images(d_pix.data_ptr(), pix_off, descs, d_str.data_ptr(), starts, d_len.data_ptr(), st)
            c.encode_status(st)
            lens, host = d_len.cpu().numpy(), d_str.cpu().numpy()
            assert [int(x) for x in lens] == [len(s) for s in want], (slabs, rep)
            for i, s in enumerate(want):
                assert host[starts[i]:starts[i] + len(s)].tobytes() == s, (slabs, rep, i, keys[i])
            region.assert_untouched(host, bounds, f"encode_images (slabs {slabs}, call {rep}): outside the slots")
            region.assert_untouched(host, [len(s) for s in want], f"encode_images (slabs {slabs}, call {rep}): behind a stream")
    finally:
        c.close()


@pytest.mark.parametrize("staging", [0, 1 << 20])
def test_encode_images_packed_exact_capacity(api, vault, staging):
    """qoimi_encode_images_packed on the same call, align 1, an odd destination and packed_capacity exactly d_packed_off[n]: the pack
    is the reference's streams back to back, and nothing in front of it, at or behind d_packed + packed_capacity is written.  Through
    the default staging and through 1 MiB of it (several sub-batches: the largest slot alone is 0.8 MB)."""
    import torch
    c = api.Context(0)
    try:
        keys, descs, pix_off, d_pix = mixed_call(api, vault)
        want = [vault.stream(*key) for key in keys]
        total = sum(len(s) for s in want)
        region = GuardedRegion(GUARD + 7 + total + GUARD, [GUARD + 7], STREAM_FILL)
        packed = torch.full((region.size,), STREAM_FILL, dtype=torch.uint8, device="cuda")
        assert packed.data_ptr() % 16 == 0
        off = torch.zeros(len(keys) + 1, dtype=torch.int64, device="cuda")
        d_len = torch.zeros(len(keys), dtype=torch.int32, device="cuda")
        got_off, got_len = c.encode_images_packed(d_pix.data_ptr(), pix_off, descs, 1, packed.data_ptr() + GUARD + 7, total, off.data_ptr(),
                                                  d_len.data_ptr(), staging, torch.cuda.current_stream().cuda_stream)
        model = np.cumsum([0] + [len(s) for s in want]).astype(np.uint64)
        assert np.array_equal(got_off, model) and np.array_equal(off.cpu().numpy().astype(np.uint64), model), staging
        assert [int(x) for x in got_len] == [len(s) for s in want] and np.array_equal(d_len.cpu().numpy(), got_len), staging
        host = packed.cpu().numpy()
        for i, s in enumerate(want):
            a = GUARD + 7 + int(model[i])
            assert host[a:a + len(s)].tobytes() == s, (staging, i, keys[i])
        region.assert_untouched(host, [total], f"encode_images_packed (staging {staging}): around the pack")
    finally:
        c.close()


# ------------------------------------------------------------------ the utilities the benchmark's verification rests on
def test_synth_frames_into_odd_strides(api):
    """qoimi_synth_frames, three frames into an odd base with pixel_stride = npx*4 + 3, every kind, 37 x 23 and 257 x 9: the frames
    equal synth.frame_rgba, the three bytes between frames and the guards around them are untouched."""
    import torch
    from qoi_amd import synth
    c = api.Context(0)
    try:
        st = torch.cuda.current_stream().cuda_stream
        for j, (w, h) in enumerate([(37, 23), (257, 9)]):
            for kind in synth.KINDS:
                npx, po = w * h, 1 + (5 * synth.KIND_ID[kind] + 3 * j) % 15
                region = GuardedRegion.strided(GUARD + po, npx * 4 + 3, 3, OUT_FILL)
                buf = torch.full((region.size,), OUT_FILL, dtype=torch.uint8, device="cuda")
                assert buf.data_ptr() % 16 == 0
                c.synth_frames(synth.KIND_ID[kind], synth.DEFAULT_SEED, 7, 3, w, h, buf.data_ptr() + GUARD + po, npx * 4 + 3, st)
                torch.cuda.synchronize()
                host = buf.cpu().numpy()
                for f in range(3):
                    want = synth.frame_rgba(kind, w, h, 7 + f).reshape(-1)
                    assert np.array_equal(host[region.starts[f]:region.starts[f] + npx * 4], want), (kind, w, h, f, po)
                region.assert_untouched(host, [npx * 4] * 3, f"synth_frames {kind} {w}x{h} at +{po}")
    finally:
        c.close()


@pytest.mark.parametrize("ch", [4, 3])
def test_hash_streams_at_odd_bases_and_strides(api, vault, ch):
    """qoimi_hash_streams over the odd-based, odd-strided streams qoimi_encode_batch left (nine images, full slots among them, no
    slack and odd slack): synth.stream_hash64 of the reference's streams."""
    import torch
    from qoi_amd import synth
    c = api.Context(0)
    try:
        for j, ((w, h), (dp, ds)) in enumerate([((517, 313), (0, 0)), ((1025, 3), (5, 7)), ((7, 3), (0, 0))]):
            po, so, oo = odd_offsets(3 * j + 2)
            keys = vault.batch(w, h, ch, 9)
            b = EdgeBatch(c, w, h, ch, 9, po, so, oo, dp, ds)
            for i, key in enumerate(keys):
                b.upload(i, vault.image(*key))
            lens, host = b.encode()
            want = [vault.stream(*key) for key in keys]
            b.check_streams(host, lens, want, f"{w}x{h}x{ch} +{ds}")
            out = torch.zeros(9, dtype=torch.int64, device="cuda")
            c.hash_streams(b.d_streams, b.stream_stride, b.lens.data_ptr(), 9, out.data_ptr(), b.stream)
            torch.cuda.synchronize()
            got = out.cpu().numpy().view(np.uint64)
            assert [int(x) for x in got] == [synth.stream_hash64(s) for s in want], (w, h, ch, ds, so)
    finally:
        c.close()


# ------------------------------------------------------------------ the retry of qoimi_encode_status
@pytest.mark.parametrize("n,w,h", [(1, 517, 313), (9, 517, 313)])
def test_a_retried_call_keeps_to_tight_odd_buffers(api, n, w, h):
    """tests/hook_scenarios.py: spin_bound_tight - a placement wait gives up (tree by workgroup index for one image, look-back for
    nine), qoimi_encode_status encodes the call again order-free with the odd bases and minimal strides it remembered, a full-slot
    image in the call: the reference's bytes, no byte outside a stream written, qoimi_encode_retries counts it."""
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "hook_scenarios.py"), "spin_bound_tight", str(n), str(w), str(h)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "retries" in r.stdout


# ------------------------------------------------------------------ the fuzzer's modes no test ran
def run_fuzz(*args):
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "fuzz_encode.py")] + list(args), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def test_encoder_fuzz_odd_strides(api):
    """tests/fuzz_encode.py --odd-strides: random images (full-slot ones among them), shapes, batch sizes and placements at odd bases
    with odd or no slack in the strides; bytes, round trips and the fill bytes behind every stream and image."""
    out = run_fuzz("--odd-strides", "--iters", "25", "--seed", "41", "--max-pixels", "600000")
    assert "every stream byte-identical" in out and "MISMATCH" not in out, out[-2000:]


def test_encoder_fuzz_dropin(api):
    """tests/fuzz_encode.py --dropin: qoi_encode / qoi_decode on host pointers, sizes jumping up and down."""
    out = run_fuzz("--dropin", "--iters", "25", "--seed", "42", "--max-pixels", "600000")
    assert "fuzz_encode --dropin" in out and "every stream byte-identical" in out and "MISMATCH" not in out, out[-2000:]
