"""tests/inspect_maps.py - the phase maps of qoi_inspect.hip in plain Python - held to streaminfo.inspect_stream, the normative model
of the walk (no GPU): the map of a body is the composition of the maps of any cut of it, a map's value is where the walk entered at that
phase ends, the counts of the blocks at their true phases add up to the model's, and the four stages of inspect_scan give every block
the phase the walk gives it."""
import numpy as np
import pytest

import cases
import inspect_maps as im
from inspect_maps import BLOCK
from qoi_amd import streaminfo as si

HEAD = cases.header(640, 360)


def bodies(encoded_streams):
    """(name, body): random bytes, random bytes dense in long chunks, the bodies of the hostile decode cases and patterned bodies"""
    out = []
    for seed in range(60):
        rng = np.random.default_rng(7000 + seed)
        n = int(rng.integers(0, 700)) if seed % 3 else int(rng.integers(BLOCK - 40, BLOCK + 40))
        out.append((f"random {seed}", rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()))
        out.append((f"long chunks {seed}", rng.choice(np.array([0xFF, 0xFE, 0xFF, 0x80, 0xC5, 0x15], dtype=np.uint8), size=n).tobytes()))
    for c in cases.decode_cases(encoded_streams):
        size = len(c["stream"]) if c["size"] is None else c["size"]
        if size >= 22:
            out.append((c["name"], bytes(c["stream"][14:size - 8])))
    for seed in range(120):
        rng = np.random.default_rng(7100 + seed)
        n = int(rng.integers(1, 2 * BLOCK)) if seed % 4 else int(rng.integers(1, 3)) * BLOCK + int(rng.integers(-3, 4))
        out.append((f"patterned {seed}", im.patterned_body(rng, n, merges=1 + seed % 3)))
    for unit in [im.ROTATE] + im.MERGING:
        out.append((f"unit {unit.hex()}", im.stretch(unit, BLOCK + 7)))
    return out


@pytest.fixture(scope="module")
def all_bodies(encoded_streams):
    b = bodies(encoded_streams)
    assert len(b) >= 300
    return b


def test_a_map_is_where_the_walk_ends(all_bodies):
    """piece_map (the backward sweep) against the forward walk of counts, and against the model's walk_end at phase 0"""
    for name, body in all_bodies:
        m = im.piece_map(body)
        assert m == tuple(im.counts(body, e)[5] for e in range(5)), name
        assert si.inspect_stream(HEAD + body + cases.END)["walk_end"] == 14 + len(body) + m[0], name
    assert im.piece_map(b"") == im.IDENTITY and im.piece_map(b"\xc0\xc0") == (0, 0, 0, 1, 2)


def test_the_maps_of_a_cut_compose_to_the_map_of_the_whole(all_bodies):
    rng = np.random.default_rng(7200)
    for name, body in all_bodies:
        whole = im.piece_map(body)
        for _ in range(3):
            cuts = sorted(int(x) for x in rng.integers(0, len(body) + 1, size=int(rng.integers(1, 6))))
            parts = [body[a:b] for a, b in zip([0] + cuts, cuts + [len(body)])]
            assert im.compose_all(im.piece_map(p) for p in parts) == whole, (name, cuts)
        assert im.compose_all(im.piece_map(b) for b in im.blocks(body)) == whole, name
    # composition is associative and not commutative
    a, b, c = (im.piece_map(im.stretch(u, 23)) for u in (im.MERGING[0], im.ROTATE, im.MERGING[2]))
    assert im.compose(im.compose(a, b), c) == im.compose(a, im.compose(b, c)) and im.compose(a, b) != im.compose(b, a)


def test_counts_at_the_true_phases_sum_to_the_model(all_bodies):
    for name, body in all_bodies:
        want = si.inspect_stream(HEAD + body + cases.END)
        got = im.info_from_blocks(body)
        assert got == {k: want[k] for k in got}, name


def test_the_issue_s_pattern():
    """FE FF FF FF C5 over 16391 bytes: phase 0 counts RGB and RUN, phases 1 .. 3 RGBA alone, phase 4 joins phase 0 - four images"""
    p = im.stretch(im.MERGING[0], 16391)
    assert im.counts(p, 0)[:2] == ([0, 0, 0, 3278, 3279, 0], 19668)
    assert all(im.counts(p, e)[0] == [0, 0, 0, 0, 0, 3278] for e in (1, 2, 3))
    m = im.piece_map(p)
    assert m[4] == m[0] and len(set(m)) == 4
    # every merging unit loses one or two live phases however long its stretch is, 0xFF none
    for n in (999, 16384, 50001):
        assert all(len(set(im.piece_map(im.stretch(u, n)))) in (3, 4) for u in im.MERGING) and len(set(im.piece_map(im.stretch(im.ROTATE, n)))) == 5


def test_the_stages_of_the_scan_give_the_walk_s_phase():
    """Scan.entry - carry, before, excl, own as inspect_scan composes them - is the walk's entry phase for every non-first block of a
    call of 8200 one-block streams around patterned streams across the lane, wavefront and tile edges; no stage dropped or reversed
    is the truth everywhere."""
    rng = np.random.default_rng(7300)
    fillers = [bytes([0xC0]), bytes([0xFE]), bytes([0xFF]), bytes([0x80]), bytes([0xFE, 0x00])]
    streams, maps = [], []
    for first, n_blocks in ((5, 4), (500, 30), (4090, 9), (8185, 12), (8700, 9)):
        while len(maps) < first:
            maps += im.block_maps(fillers[int(rng.integers(5))])
        body = im.patterned_body(rng, n_blocks * BLOCK - int(rng.integers(0, 9)), merges=2)
        streams.append((len(maps), body))
        maps += im.block_maps(body)
    scan = im.Scan(maps)
    differs = set()
    for first, body in streams:
        for k, e in enumerate(im.entries(body)):
            if k == 0:
                continue                                  # (a stream's first block takes phase 0 whatever the scan says)
            assert scan.entry(first + k) == e, (first, k)
            differs |= {name for name, phase in scan.wrong(first + k).items() if k and phase != e}
    assert differs >= {"without " + s for s in im.STAGES} | {"before reversed", "excl reversed", "own reversed"}
