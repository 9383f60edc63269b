"""CPU-only: the ABI of qoimi_inspect_streams (declaration, export list, struct layout) and the Python model of its walk
(qoi_amd/streaminfo.py) against the reference encoder's streams, the reference decoder's leniency and hand-written streams."""
import ctypes
import os
import re

import numpy as np

import cases
from qoi_amd import api, streaminfo as si

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_of_inspect_streams():
    hdr = open(os.path.join(ROOT, "include", "qoi_mi355x.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+qoimi_inspect_streams\s*\(", hdr)
    assert "qoimi_inspect_streams" in api.EXPORTS
    assert ctypes.sizeof(api.StreamInfo) == 64 and si.INFO_DTYPE.itemsize == 64
    names = ("pixels", "run_pixels", "ops", "repeat_index", "walk_end", "flags", "reserved")
    want = (0, 8, 16, 40, 44, 48, 52)
    assert tuple(getattr(api.StreamInfo, n).offset for n in names) == want
    assert tuple(si.INFO_DTYPE.fields[n][1] for n in names) == want
    for name, value in (("QOIMI_OP_INDEX", 0), ("QOIMI_SI_TOO_SHORT", 1), ("QOIMI_SI_HEADER_BAD", 2), ("QOIMI_SI_PIXELS_SHORT", 4), ("QOIMI_SI_PIXELS_OVER", 8),
                        ("QOIMI_SI_LAST_CHUNK_CUT", 16), ("QOIMI_SI_NO_END_MARKER", 32), ("QOIMI_SI_REPEATED_INDEX", 64)):
        assert re.search(rf"\b{name}\s*=\s*{value}\b", hdr), name
    assert (si.SI_TOO_SHORT, si.SI_HEADER_BAD, si.SI_PIXELS_SHORT, si.SI_PIXELS_OVER, si.SI_LAST_CHUNK_CUT, si.SI_NO_END_MARKER,
            si.SI_REPEATED_INDEX) == (1, 2, 4, 8, 16, 32, 64)
    assert (si.OP_INDEX, si.OP_DIFF, si.OP_LUMA, si.OP_RUN, si.OP_RGB, si.OP_RGBA) == (0, 1, 2, 3, 4, 5)


def test_reference_encoder_streams_conform(ref, port):
    oracle = ref or port
    n = 0
    for case in cases.encode_cases():
        stream = oracle.encode(case["pixels"], case["w"], case["h"], case["ch"], case["cs"])
        info = si.inspect_stream(stream)
        assert info["flags"] == 0, (case["name"], si.flag_names(info["flags"]))
        assert info["pixels"] == case["w"] * case["h"], case["name"]
        assert info["walk_end"] == len(stream) - 8, case["name"]
        assert sum(info["ops"]) - info["ops"][si.OP_RUN] + info["run_pixels"] == info["pixels"], case["name"]
        assert info["repeat_index"] == 0, case["name"]
        n += 1
    assert n > 80


def test_leniency_of_the_reference_decoder(ref, port, encoded_streams):
    oracle = ref or port
    by_name = {c["name"]: c for c in cases.decode_cases(encoded_streams)}
    checked = 0
    for name, case in by_name.items():
        if not name.startswith("trunc_"):
            continue
        info = si.inspect_stream(case["stream"], case["size"])
        if not (info["flags"] & si.SI_PIXELS_SHORT and info["pixels"] > 0):
            continue
        px, desc = oracle.decode(case["stream"], 4, case["size"])
        assert px is not None, name
        px = np.asarray(px).reshape(-1, 4)
        assert info["pixels"] < desc.width * desc.height
        # a cut stream decodes into a tail of repeated pixels (qoi.h:544) - with status OK; the model says where it begins
        assert np.all(px[info["pixels"]:] == px[info["pixels"] - 1]), name
        checked += 1
    assert checked >= 30
    assert si.inspect_stream(by_name["garbage_trailer"]["stream"])["flags"] == si.SI_NO_END_MARKER
    for name in ("rgba_into_trailer", "luma_into_trailer"):
        assert si.inspect_stream(by_name[name]["stream"])["flags"] & si.SI_LAST_CHUNK_CUT, name


def test_hand_written_streams():
    size22 = cases.header(5, 3) + cases.END
    assert si.inspect_stream(size22) == {"pixels": 0, "run_pixels": 0, "ops": [0, 0, 0, 0, 0, 0], "repeat_index": 0, "walk_end": 14,
                                         "flags": si.SI_PIXELS_SHORT}
    # INDEX, DIFF, LUMA (2 bytes), RUN of 5, RGB (4 bytes), RGBA (5 bytes): 14 body bytes, 10 pixels
    each = cases.header(5, 2) + bytes([0x07, 0x6A, 0xA0, 0x88, 0xC4, 0xFE, 1, 2, 3, 0xFF, 4, 5, 6, 7]) + cases.END
    assert si.inspect_stream(each) == {"pixels": 10, "run_pixels": 5, "ops": [1, 1, 1, 1, 1, 1], "repeat_index": 0, "walk_end": 28, "flags": 0}
    triple = cases.header(3, 1) + bytes([0x15, 0x15, 0x15]) + cases.END
    assert si.inspect_stream(triple) == {"pixels": 3, "run_pixels": 0, "ops": [3, 0, 0, 0, 0, 0], "repeat_index": 2, "walk_end": 17,
                                         "flags": si.SI_REPEATED_INDEX}
    assert si.inspect_stream(size22[:21]) == {"pixels": 0, "run_pixels": 0, "ops": [0] * 6, "repeat_index": 0, "walk_end": 0, "flags": si.SI_TOO_SHORT}
    # the size override cuts the stream; a record holds what the dict holds
    cut = si.inspect_stream(each, len(each) - 6)
    assert cut["flags"] == si.SI_PIXELS_SHORT | si.SI_NO_END_MARKER | si.SI_LAST_CHUNK_CUT and cut["walk_end"] == 23 and cut["ops"] == [1, 1, 1, 1, 1, 0]
    rec = si.info_record(cut)
    assert rec.dtype == si.INFO_DTYPE and int(rec["pixels"]) == 9 and list(rec["ops"]) == [1, 1, 1, 1, 1, 0] and int(rec["flags"]) == cut["flags"]
