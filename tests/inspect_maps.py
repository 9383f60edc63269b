"""The phase maps of qoi_inspect.hip restated in plain Python, for tests that must PROVE that their input carries state through the kernels'
scans: the map of a byte string as a tuple {0..4} -> {0..4} (entered e bytes behind its first byte - the chunk in front reaches e bytes in -
the walk leaves x bytes over), the composition of maps, the counts of the walk entered at e, and the four stages in which inspect_scan puts
the entry phase of a block together.  tests/test_inspect_maps.py holds all of it to streaminfo.inspect_stream."""
from functools import lru_cache

BLOCK = 16384                      # qoi_inspect.hip: kInsBlock
PER, WAVE, TILE = 8, 512, 8192     # inspect_scan: block maps per thread, per wavefront (64 lanes), per tile (16 wavefronts)
IDENTITY = (0, 1, 2, 3, 4)
HEADER, TRAILER = 14, 8


def chunk_len(b):
    return b - 0xFA if b >= 0xFE else (2 if b >> 6 == 2 else 1)


@lru_cache(maxsize=4096)
def piece_map(data):
    """The map of `data` (bytes): one backward sweep, exit(pos) = exit(pos + length of the chunk at pos), exit(n + j) = j."""
    n = len(data)
    ex = [0] * n + [0, 1, 2, 3, 4]
    for pos in range(n - 1, -1, -1):
        ex[pos] = ex[pos + chunk_len(data[pos])]
    return tuple(ex[:5])


def compose(first, then):
    """the map of two pieces in a row: then[first[e]] (qoi_inspect.hip: ins_compose)"""
    return tuple(then[first[e]] for e in range(5))


def compose_all(maps):
    r = IDENTITY
    for m in maps:
        r = compose(r, m)
    return r


def constant(x):
    return (x,) * 5


def is_constant(m):
    return len(set(m)) == 1


def blocks(body):
    return [bytes(body[at:at + BLOCK]) for at in range(0, len(body), BLOCK)]


def block_maps(body):
    """The maps of the 16 KiB blocks of a stream's body as inspect_maps publishes them: the first as the constant map of its exit at phase 0."""
    ms = [piece_map(b) for b in blocks(body)]
    if ms:
        ms[0] = constant(ms[0][0])
    return ms


def entries(body):
    """the true entry phase of every block of a body"""
    out, e = [], 0
    for b in blocks(body):
        out.append(e)
        e = piece_map(b)[e]
    return out


def counts(data, e):
    """The walk over `data` entered at phase e: (ops[6], run pixels, repeated INDEX pairs inside, first tag, last tag, exit); a tag is None
    where no chunk starts in `data`."""
    ops, run_px, rep, first, last = [0] * 6, 0, 0, None, None
    p, n = e, len(data)
    while p < n:
        b = data[p]
        if b >= 0xFE:
            ops[4 + (b & 1)] += 1
        else:
            ops[b >> 6] += 1
            if b >> 6 == 3:
                run_px += (b & 63) + 1
        if b < 64 and b == last:
            rep += 1
        first = b if first is None else first
        last = b
        p += chunk_len(b)
    return ops, run_px, rep, first, last, p - n


def info_from_blocks(body):
    """The walk's fields of streaminfo.inspect_stream put together as inspect_count and inspect_reduce do: per block at its true entry
    phase, the repeated INDEX across a block edge from the neighbours' last / first tags."""
    ops, run_px, rep, prev_last, e = [0] * 6, 0, 0, None, 0
    for b in blocks(body):
        o, r, q, first, last, e = counts(b, e)
        ops = [a + c for a, c in zip(ops, o)]
        run_px += r
        rep += q + (1 if first is not None and first < 64 and first == prev_last else 0)
        prev_last = last if last is not None else prev_last
    pixels = sum(ops) - ops[3] + run_px
    return {"pixels": pixels, "run_pixels": run_px, "ops": ops, "repeat_index": rep, "walk_end": HEADER + len(body) + e}


# ---------------------------------------------------------------------------------------------------------------------------------
# inspect_scan: the entry phase of block i of a call is own(excl(before(carry(0)))) - the maps of the tiles in front (carry), of the
# wavefronts in front within the tile (before), of the lanes in front within the wavefront (excl) and of the thread's own maps in front.
# ---------------------------------------------------------------------------------------------------------------------------------
STAGES = ("carry", "before", "excl", "own")


class Scan:
    """inspect_scan over the published block maps of one call"""

    def __init__(self, maps):
        self.maps = list(maps)
        self._totals = {}

    def total(self, k):
        """the map of tile k"""
        if k not in self._totals:
            self._totals[k] = compose_all(self.maps[k * TILE:(k + 1) * TILE])
        return self._totals[k]

    def stages(self, i):
        """the four stage maps of block i"""
        t0, w0, l0 = i // TILE * TILE, i // WAVE * WAVE, i // PER * PER
        m = self.maps
        return {"carry": compose_all(self.total(k) for k in range(i // TILE)), "before": compose_all(m[t0:w0]),
                "excl": compose_all(m[w0:l0]), "own": compose_all(m[l0:i])}

    def entry(self, i):
        return entry_phase(self.stages(i))

    def wrong(self, i):
        """What block i would be entered at if inspect_scan were wrong in one place: {name: phase}.  `without X`: stage X replaced by the
        identity.  `X reversed`: the composition that brings stage X in, taken in the wrong order.  `tiles reversed`: the tile totals composed
        as carry = compose(total, carry)."""
        st = self.stages(i)
        out = {"without " + s: entry_phase(dict(st, **{s: IDENTITY})) for s in STAGES}
        cb = compose(st["carry"], st["before"])
        cbe = compose(cb, st["excl"])
        out["before reversed"] = compose(compose(compose(st["before"], st["carry"]), st["excl"]), st["own"])[0]
        out["excl reversed"] = compose(compose(st["excl"], cb), st["own"])[0]
        out["own reversed"] = compose(st["own"], cbe)[0]
        rev = IDENTITY
        for k in range(i // TILE):
            rev = compose(self.total(k), rev)
        out["tiles reversed"] = entry_phase(dict(st, carry=rev))
        return out


def entry_phase(st):
    return compose_all(st[s] for s in STAGES)[0]


# ---------------------------------------------------------------------------------------------------------------------------------
# Bodies whose block maps are neither constant nor commuting: stretches of period 5.  Only 0xFF (5 bytes) keeps a walk in its residue,
# so a stretch of 0xFF rotates the phases, and a unit with one walk that hops through several residues (FE ... C5: 4 + 1 bytes) merges the
# phases of those residues into one and leaves the others apart - one live phase less per stretch, whatever its length.
# ---------------------------------------------------------------------------------------------------------------------------------
ROTATE = bytes([0xFF] * 5)
MERGING = [bytes(u) for u in ([0xFE, 0xFF, 0xFF, 0xFF, 0xC5], [0xC5, 0xFE, 0xFF, 0xFF, 0xFF], [0xFF, 0xFF, 0xFE, 0xFF, 0x15], [0xFF, 0xC5, 0xFE, 0xFF, 0xFF],
                                      [0xFE, 0xFF, 0xFF, 0xFF, 0x6A], [0xFF, 0xFF, 0xFF, 0xFE, 0xFF])]


def stretch(unit, n):
    return (unit * (n // len(unit) + 1))[:n]


def patterned_body(rng, n, merges=1):
    """n bytes: a stretch of 0xFF, then `merges` times a merging stretch and a stretch of 0xFF, every length drawn by `rng` (a numpy
    Generator) and no stretch of 0xFF a multiple of 5."""
    cuts = sorted(int(x) for x in rng.integers(1, max(2, n), size=2 * merges))
    parts, at = [], 0
    for k, c in enumerate(cuts + [n]):
        ln = max(0, min(c, n) - at)
        unit = ROTATE if k % 2 == 0 else MERGING[int(rng.integers(len(MERGING)))]
        if unit is ROTATE and ln % 5 == 0 and ln > 0 and c != n:
            ln -= 1
        parts.append(stretch(unit, ln))
        at += ln
    return b"".join(parts)
