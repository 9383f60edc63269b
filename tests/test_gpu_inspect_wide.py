"""qoimi_inspect_streams on the GPU (-m gpu) where the fixtures of tests/test_gpu_inspect.py leave the carried values trivial: block maps
that are neither constant nor commuting across the lane, wavefront and tile edges of inspect_scan, a stream of more than 64 blocks per lane
trip of inspect_reduce with repeated INDEX pairs across exactly those block edges, and pixel sums from 2**32 up to the largest stream an
`int` size allows.  Every expectation is streaminfo.inspect_stream, or a closed form that a CPU test in this file
holds equal to it at small lengths.  Every test first asserts from tests/inspect_maps.py - the kernels' phase maps restated in plain
Python - that its input REACHES what it is there for: a later edit of a generator that turns an input trivial fails the test."""
import numpy as np
import pytest

import cases
import inspect_maps as im
from inspect_maps import BLOCK
from qoi_amd import streaminfo as si
from gpu_calls import assert_info
from gpu_pack import dev
from gpu_pack import api, ctx  # noqa: F401  (fixtures)

gpu = pytest.mark.gpu          # (not the module: test_closed_form_is_the_model needs no GPU)
HEAD = cases.header(640, 360)
# one-block bodies that leave 0, 3, 4, 1 and 2 bytes over: the constant maps in front of the patterned streams differ
FILLERS = [bytes([0xC0]), bytes([0xFE]), bytes([0xFF]), bytes([0x80]), bytes([0xFE, 0x00])]
WAVE_STAGES = ("without before", "without excl", "without own", "excl reversed", "own reversed")
TILE_STAGES = ("without carry", "before reversed")


class Call:
    """The streams of one inspect_streams call, back to back in one buffer (pad bytes of 0x5C where a start alignment is asked for), the
    index of every stream's first block in the kernels' block table and the published block maps of the whole call."""

    def __init__(self):
        self.blob, self.offs, self.bodies, self.first_blk, self.maps = bytearray(b"\x5c" * 3), [], [], [], []
        self._maps, self._models = {}, {}

    @property
    def n_blocks(self):
        return len(self.maps)

    def add(self, body, start_mod4=None):
        if start_mod4 is not None:
            self.blob += b"\x5c" * ((start_mod4 - len(self.blob)) % 4)
        self.offs.append(len(self.blob))
        self.blob += HEAD + body + cases.END
        self.bodies.append(body)
        self.first_blk.append(len(self.maps))
        if body not in self._maps:
            self._maps[body] = im.block_maps(body)
        self.maps += self._maps[body]
        return len(self.bodies) - 1

    def fill_to(self, index, rng):
        """one-block streams until the next stream's first block has `index`"""
        assert self.n_blocks <= index
        kinds = rng.integers(len(FILLERS), size=index - self.n_blocks)
        for k in kinds:
            self.add(FILLERS[int(k)])

    def model(self, s):
        body = self.bodies[s]
        if body not in self._models:
            self._models[body] = si.info_record(si.inspect_stream(HEAD + body + cases.END))
        return self._models[body]

    def check(self, ctx):
        """one call; every info against the model"""
        sizes = [len(HEAD) + len(b) + len(cases.END) for b in self.bodies]
        d = dev(np.frombuffer(bytes(self.blob) + b"\x5c", dtype=np.uint8).copy())
        infos, first = ctx.inspect_streams(d.data_ptr(), self.offs, sizes)
        want = np.array([self.model(s) for s in range(len(self.bodies))], dtype=si.INFO_DTYPE)
        bad = np.flatnonzero(infos != want)
        if bad.size:
            s = int(bad[0])
            assert_info(infos[s], si.inspect_stream(HEAD + self.bodies[s] + cases.END), (s, self.first_blk[s], len(self.bodies[s])))
        flagged = np.flatnonzero(want["flags"])
        assert first == (int(flagged[0]) if flagged.size else None)
        return infos


def caught(call, streams, probed=None):
    """{mistake of inspect_scan: [block indices]}: the non-first blocks of `streams` whose entry phase that mistake changes AND whose own
    counts differ between the true and the changed phase (inspect_maps.Scan.wrong); the true phase of the scan is the walk's.  probed: only the blocks with these indices."""
    scan, out = im.Scan(call.maps), {}
    for s in streams:
        body = call.bodies[s]
        true = im.entries(body)
        for k, blk in enumerate(im.blocks(body)):
            if k == 0:
                continue
            i = call.first_blk[s] + k
            if probed is not None and i not in probed:
                continue
            assert scan.entry(i) == true[k], (s, k)
            for name, phase in scan.wrong(i).items():
                if phase != true[k] and im.counts(blk, phase)[:2] != im.counts(blk, true[k])[:2]:
                    out.setdefault(name, []).append(i)
    return out


def non_first(call, streams):
    return sorted(call.first_blk[s] + k for s in streams for k in range(1, len(im.blocks(call.bodies[s]))))


def assert_reach(got, names, lo, hi, what):
    for name in names:
        hit = [i for i in got.get(name, []) if lo <= i <= hi]
        print(what, name, "caught at blocks", hit)
        assert hit, (what, name, "no probed block in", (lo, hi), "would show it")


# ------------------------------------------------------------------ 1: the lane and wavefront edges of inspect_scan
@gpu
def test_wave_edge_long_stream(ctx):
    """One stream of 640 blocks (10.5 MB: two merging stretches between stretches of 0xFF), so the phase of its blocks 505 .. 520 has come
    through the eight maps of a thread, 64 lanes and s_wave; behind it one-block streams and a patterned stream across block 1024 (wavefront 2).
    Reach: every mistake of WAVE_STAGES - a stage dropped, a composition reversed - changes the entry phase and the counts of a block in
    505 .. 520, and of one in 1019 .. 1037 (`excl` is the identity for the eight blocks of lane 0, 1024 .. 1031)."""
    rng = np.random.default_rng(4101)
    call = Call()
    long = call.add(im.patterned_body(rng, 640 * BLOCK - 2, merges=2))
    call.fill_to(1017, rng)
    short = call.add(im.patterned_body(rng, 20 * BLOCK + 1, merges=2))
    assert call.first_blk[long] == 0 and len(im.blocks(call.bodies[long])) == 640 and call.n_blocks == 1017 + 21
    assert not any(im.is_constant(m) for m in call.maps[1:640]), "a constant map inside the long stream forgets what is in front of it"
    got = caught(call, [long, short], probed=set(range(505, 521)) | set(range(1019, 1038)))
    assert_reach(got, WAVE_STAGES, 505, 520, "long stream")
    assert_reach(got, WAVE_STAGES, 1019, 1037, "across block 1024")
    call.check(ctx)


@gpu
def test_wave_edge_short_streams_and_every_start_alignment(ctx):
    """503 one-block streams, then a patterned stream of 19 blocks (non-first blocks 504 .. 521: it starts in wavefront 0 and ends in
    wavefront 1).  Behind it the patterned streams of every start alignment: body lengths k * 16384 + r, r = -3 .. 3, at all four byte
    alignments of the stream's first byte.  Reach as above for 505 .. 520; every aligned stream has a non-first block that is entered
    at a phase other than 0."""
    rng = np.random.default_rng(4202)
    call = Call()
    call.fill_to(503, rng)
    a = call.add(im.patterned_body(rng, 19 * BLOCK - 1, merges=2))
    assert non_first(call, [a]) == list(range(504, 522))
    aligned = []
    for mod4 in range(4):
        for r in range(-3, 4):
            k = 3 + (mod4 + r) % 2
            s = call.add(im.patterned_body(rng, k * BLOCK + r, merges=1 + (r & 1)), start_mod4=mod4)
            assert call.offs[s] % 4 == mod4 and len(call.bodies[s]) % BLOCK == r % BLOCK
            assert any(e != 0 for e in im.entries(call.bodies[s])[1:])
            aligned.append(s)
    assert len(aligned) == 28
    got = caught(call, [a])
    assert_reach(got, WAVE_STAGES, 505, 520, "short stream")
    call.check(ctx)


# ------------------------------------------------------------------ 2: the tile edge of inspect_scan
@gpu
def test_tile_edge(ctx):
    """One-block streams up to block 8182, a patterned stream of 20 blocks across the edge of tile 0 (non-first blocks 8184 .. 8202), one-block
    streams again and a second patterned stream across block 16384.  Reach: `carry` dropped, or composed with `before` in the wrong order,
    changes phase and counts of a block in 8192 .. 8200 and of one from 16384; the tile totals composed in the wrong order
    (carry = compose(total, carry)) show from the third tile only: a block from 16384."""
    rng = np.random.default_rng(4303)
    call = Call()
    call.fill_to(8183, rng)
    a = call.add(im.patterned_body(rng, 20 * BLOCK - 3, merges=2))
    call.fill_to(8700, rng)
    c = call.add(im.patterned_body(rng, 13 * BLOCK + 3, merges=2))
    call.fill_to(16377, rng)
    b = call.add(im.patterned_body(rng, 16 * BLOCK + 2, merges=2))
    assert non_first(call, [a]) == list(range(8184, 8203)) and non_first(call, [b]) == list(range(16378, 16394))
    assert non_first(call, [c]) == list(range(8701, 8714))
    got = caught(call, [a, c, b])
    assert_reach(got, ("without carry",), 8192, 8200, "tile 1")
    assert_reach(got, ("before reversed",), 8704, 8713, "tile 1, wavefront 1")
    assert_reach(got, ("without carry", "tiles reversed"), 16384, 16393, "tile 2")
    assert not [i for i in got.get("tiles reversed", []) if i < 16384]
    call.check(ctx)


# ------------------------------------------------------------------ 3: inspect_reduce beyond one trip
def index_body(n_blocks, edges):
    """n_blocks * 16384 bytes of INDEX chunks, 0x15 and 0x2A in turn; at every block edge of `edges` (k: between blocks k - 1 and k) the
    byte in front is repeated and the turn goes on from there: one repeated pair per edge and no other"""
    j = np.arange(n_blocks * BLOCK)
    flips = np.zeros(j.size, dtype=np.int64)
    for k in edges:
        flips[k * BLOCK:] += 1
    return np.where((j + flips) % 2 == 0, 0x15, 0x2A).astype(np.uint8).tobytes()


@gpu
def test_reduce_beyond_one_trip(ctx):
    """131 blocks of INDEX bytes: a lane of inspect_reduce makes up to three trips.  Repeated pairs across the block edges 63|64, 64|65,
    127|128 and 128|129 - the last block of a trip against the first of the next, looked up in the previous partial - and nowhere else;
    a second stream without them."""
    edges = (64, 65, 128, 129)
    planted, plain = index_body(131, edges), index_body(131, ())
    for k in range(1, 131):
        assert (planted[k * BLOCK] == planted[k * BLOCK - 1]) == (k in edges) and plain[k * BLOCK] != plain[k * BLOCK - 1]
    arr = np.frombuffer(planted, dtype=np.uint8)
    assert int(np.count_nonzero(arr[1:] == arr[:-1])) == len(edges)       # ... all of them across a block edge
    call = Call()
    s0, s1 = call.add(planted), call.add(plain)
    infos = call.check(ctx)
    assert int(infos[s0]["repeat_index"]) == len(edges) and int(infos[s1]["repeat_index"]) == 0
    assert int(infos[s0]["flags"]) == si.SI_PIXELS_OVER | si.SI_REPEATED_INDEX and int(infos[s1]["flags"]) == si.SI_PIXELS_OVER


# ------------------------------------------------------------------ 4: sums from 2**32
RUN62 = 0xFD                        # the longest run: 62 pixels
INDEX_TAG, DIFF_TAG = 0x15, 0x6A    # one-byte chunks planted in the mixed bodies: body byte j is INDEX where j % 7 == 3, else DIFF where j % 11 == 5


def closed_form(body, mixed):
    """The model's fields for a body of `body` bytes of 0xFD, `mixed`: with the planted INDEX and DIFF bytes.  Every chunk is one byte."""
    def count(n, mod, rem):
        return (n - rem + mod - 1) // mod if n > rem else 0
    n_index = count(body, 7, 3) if mixed else 0
    n_diff = count(body, 11, 5) - count(body, 77, 38) if mixed else 0          # j % 7 == 3 and j % 11 == 5: j % 77 == 38
    runs = body - n_index - n_diff
    ops = [n_index, n_diff, 0, runs, 0, 0]
    return {"pixels": 62 * runs + n_index + n_diff, "run_pixels": 62 * runs, "ops": ops, "repeat_index": 0, "walk_end": 14 + body,
            "flags": si.SI_PIXELS_OVER if 62 * runs + n_index + n_diff > 640 * 360 else (si.SI_PIXELS_SHORT if 62 * runs + n_index + n_diff < 640 * 360 else 0)}


def host_body(body, mixed):
    a = np.full(body, RUN62, dtype=np.uint8)
    if mixed:
        a[5::11] = DIFF_TAG
        a[3::7] = INDEX_TAG
    return a.tobytes()


def test_closed_form_is_the_model():
    for body in list(range(0, 200)) + [3716, 3717, 3718, 16383, 16384, 16385, 69999, 70000]:
        for mixed in (False, True):
            want = si.inspect_stream(HEAD + host_body(body, mixed) + cases.END)
            assert closed_form(body, mixed) == want, (body, mixed)


def device_stream(buf, at, size, mixed):
    """a stream of `size` bytes at buf[at:], filled on the device as host_body fills it"""
    import torch
    body = size - 22
    view = buf[at + 14:at + 14 + body]
    view.fill_(RUN62)
    if mixed:
        view[5::11] = DIFF_TAG
        view[3::7] = INDEX_TAG
    buf[at:at + 14].copy_(torch.from_numpy(np.frombuffer(HEAD, dtype=np.uint8).copy()))
    buf[at + 14 + body:at + size].copy_(torch.from_numpy(np.frombuffer(cases.END, dtype=np.uint8).copy()))


def check_device_streams(ctx, buf, placed):
    infos, first = ctx.inspect_streams(buf.data_ptr(), [at for (at, _, _) in placed], [size for (_, size, _) in placed])
    assert first == 0
    for k, (at, size, mixed) in enumerate(placed):
        want = closed_form(size - 22, mixed)
        assert want["run_pixels"] >= 1 << 32 and want["flags"] == si.SI_PIXELS_OVER
        assert_info(infos[k], want, (at, size, mixed))
    return infos


@gpu
def test_sums_from_2_to_the_32(ctx):
    """Two streams in one call, the second 3 bytes off dword alignment: 70 MB of 0xFD alone (chunks = body bytes, pixels = 62 * body =
    4.34e9) and 90 MB of 0xFD with INDEX and DIFF bytes planted by formula (ops[RUN], ops[INDEX] and ops[DIFF] distinct large numbers,
    pixels != run_pixels, both from 2**32).  The 64-bit butterfly of inspect_reduce and R.pixels leave 32 bits; PIXELS_OVER and no other flag."""
    import torch
    size, size_mixed = 70_000_000 + 22, 90_000_000 + 22
    assert 62 * (size - 22) >= 1 << 32
    buf = torch.full((size + 3 + size_mixed + 64,), 0x5C, dtype=torch.uint8, device="cuda")
    placed = [(0, size, False), (size + 3, size_mixed, True)]
    for at, sz, mixed in placed:
        device_stream(buf, at, sz, mixed)
    infos = check_device_streams(ctx, buf, placed)
    assert int(infos[0]["pixels"]) == int(infos[0]["run_pixels"]) == 62 * 70_000_000
    assert int(infos[1]["pixels"]) != int(infos[1]["run_pixels"]) and len({int(x) for x in infos[1]["ops"][[0, 1, 3]]}) == 3
    del buf
    torch.cuda.empty_cache()


@gpu
def test_largest_size(ctx):
    """size = 2**31 - 1, the largest `int`: 131072 blocks, 2048 per lane of inspect_reduce - the edge of the bound in its comment (a lane's
    32-bit run_lo reaches 2048 * 16384 * 62 = 2.08e9 < 2**32) - and walk_end near 2**31.  Once 0xFD alone, once mixed, in the same 2 GiB."""
    import torch
    size = (1 << 31) - 1
    assert -(-(size - 22) // BLOCK) == 131072 and 2048 * BLOCK * 62 < 1 << 32
    buf = torch.empty(size + 1, dtype=torch.uint8, device="cuda")
    for mixed in (False, True):
        device_stream(buf, 0, size, mixed)
        infos = check_device_streams(ctx, buf, [(0, size, mixed)])
        assert int(infos[0]["walk_end"]) == size - 8 and int(infos[0]["run_pixels"]) > 1 << 36
    del buf
    torch.cuda.empty_cache()
