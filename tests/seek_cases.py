"""What the -m gpu tests of the row seek index share: hand-made and encoded streams whose seek points fall where the kernels can go wrong,
their oracle decodes (computed once, never changed) and a pack of them on the device, back to back at odd offsets."""
import numpy as np

from qoi_amd import seekindex as si
from model_cases import END, header

STREAM_FILL = 0xEE


class Case:
    def __init__(self, name, stream, w, h, ch, K, oracle):
        self.name, self.stream, self.w, self.h, self.ch, self.K = name, bytes(stream), w, h, ch, K
        full4, d = oracle.decode(self.stream, 4)
        assert full4 is not None and (d.width, d.height, d.channels) == (w, h, ch), name
        full3, _ = oracle.decode(self.stream, 3)
        self.full = {4: full4.reshape(h, w, 4), 3: full3.reshape(h, w, 3)}
        self.points = si.points(self.stream, w, h, K, full4)

    def band(self, first_row, rows):
        return si.band_stream(self.stream, self.w, self.h, self.ch, 0, self.K, self.points, first_row, rows)


def cases(oracle):
    rng = np.random.default_rng(2026)
    out = []
    # a body of about 46 KB: points in different 16 KiB blocks, 4 KiB tiles and 64-byte pieces
    noise = oracle.encode(rng.integers(0, 256, size=96 * 96 * 4, dtype=np.uint8), 96, 96, 4)
    assert 40000 < len(noise) < 50000
    out.append(Case("noise96", noise, 96, 96, 4, 2, oracle))
    # runs of 62 that straddle the seek rows: 187 = 3 * 62 + 1, 185 = 2 * 62 + 61
    out.append(Case("skip1", header(187, 5, 4) + b"\xfd" * 30 + END, 187, 5, 4, 1, oracle))
    out.append(Case("skip61", header(185, 4, 3) + b"\xfd" * 20 + END, 185, 4, 3, 1, oracle))
    assert int(out[-2].points[0]["skip"]) == 1 and int(out[-1].points[0]["skip"]) == 61
    # ... and a block edge: row 5432 of 187 pixels begins at pixel 1 015 784 = 16 383 * 62 + 38, inside the run whose byte is the last of the
    # body's first 16 KiB block; with one INDEX chunk in front, inside the run whose byte is the first of the second block
    out.append(Case("edge_last", header(187, 5440, 4) + b"\xfd" * 16500 + END, 187, 5440, 4, 1, oracle))
    out.append(Case("edge_first", header(187, 5440, 3) + b"\x00" + b"\xfd" * 16500 + END, 187, 5440, 3, 1, oracle))
    assert (int(out[-2].points[5431]["byte_off"]), int(out[-2].points[5431]["skip"])) == (14 + 16383, 38)
    assert (int(out[-1].points[5431]["byte_off"]), int(out[-1].points[5431]["skip"])) == (14 + 16384, 37)
    # a body of 0xFF bytes keeps five phases alive for ever
    out.append(Case("all_ff", header(64, 125, 4) + b"\xff" * 40001 + END, 64, 125, 4, 2, oracle))
    # cut in the middle: points behind the end of the chunks
    out.append(Case("cut", noise[:len(noise) // 2], 96, 96, 4, 3, oracle))
    assert int(out[-1].points[-1]["byte_off"]) == len(out[-1].stream) - 8
    # a colour last seen many intervals back, slots never written
    px = np.zeros((60, 64, 3), dtype=np.uint8)
    px[0, :5] = (200, 10, 30)
    px[1:, ::2] = (1, 2, 3)
    px[1:, 1::2] = (9, 9, 9)
    out.append(Case("old_colour", oracle.encode(px, 64, 60, 3), 64, 60, 3, 2, oracle))
    old = int(out[-1].full[4][0, 0].view("<u4")[0])
    assert old in [int(v) for v in out[-1].points[-1]["table"]] and sum(int(v) == 0 for v in out[-1].points[-1]["table"]) > 50
    # widths 1 and 63 to 65
    out.append(Case("w1", oracle.encode(rng.integers(0, 4, size=400 * 4, dtype=np.uint8) * 60, 1, 400, 4), 1, 400, 4, 128, oracle))
    for w in (63, 64, 65):
        out.append(Case(f"w{w}", oracle.encode(rng.integers(0, 256, size=w * 20 * 3, dtype=np.uint8), w, 20, 3), w, 20, 3, 3, oracle))
    # an image without a point
    out.append(Case("no_point", oracle.encode(rng.integers(0, 256, size=40 * 4 * 4, dtype=np.uint8), 40, 4, 4), 40, 4, 4, 4, oracle))
    assert len(out[-1].points) == 0 and {c.ch for c in out} == {3, 4}
    return out


class DevicePack:
    """The cases' streams back to back on the device, every one at an odd offset, between fill bytes."""

    def __init__(self, api, the_cases):
        import torch
        self.cases = the_cases
        self.offsets, pos = [], 65
        for c in the_cases:
            self.offsets.append(pos)
            pos += len(c.stream) + (2 if (pos + len(c.stream)) % 2 else 1)
        assert all(o % 2 for o in self.offsets)
        host = np.full(pos + 64, STREAM_FILL, dtype=np.uint8)
        for o, c in zip(self.offsets, the_cases):
            host[o:o + len(c.stream)] = np.frombuffer(c.stream, dtype=np.uint8)
        self.host = host
        self.dev = torch.from_numpy(host).cuda()
        self.sizes = [len(c.stream) for c in the_cases]
        self.descs = [api.QoiDesc(c.w, c.h, c.ch, 0) for c in the_cases]
        self.intervals = [c.K for c in the_cases]
        self.point_firsts = [int(x) for x in np.cumsum([0] + [len(c.points) for c in the_cases[:-1]])]
        self.points = np.concatenate([c.points for c in the_cases])
