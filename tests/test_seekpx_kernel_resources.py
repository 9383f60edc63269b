"""The two kernels behind both builds of the seek index (qoimi_build_seek_index, qoimi_seek_index_from_pixels) in the built library, without a
GPU: they are the only pair of their kind, no scratch and no spills (the lane's dwords and pixels
stay in registers), the LDS of seekpx_last is the tile's 64 words, and few enough registers for eight wavefronts per SIMD (512 / 8 = 64):
the kernels wait for memory, not for arithmetic."""
import os
import re

import pytest

from tools import kernel_resources as KR

LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "qoi_amd", "lib", "libqoi_mi355x.so")


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    return KR.kernels(LIB)


@pytest.mark.parametrize("name", ["seekpx_last", "seekpx_carry"])
def test_no_scratch(kernels, name):
    hits = [k for k in kernels if name in k]
    assert len(hits) == 1, hits
    k = kernels[hits[0]]
    assert k["scratch"] == 0 and k["vgpr_spills"] == 0 and k["agpr"] == 0, k
    assert k["vgpr"] <= 64, k
    assert k["lds"] == (256 if name == "seekpx_last" else 0), k


def function_name(symbol):
    """the function's own name in an Itanium-mangled symbol of namespace qoimi (_ZN5qoimi<len><name>E...); anything else as it is"""
    m = re.match(r"_ZN5qoimi(\d+)", symbol)
    return symbol[m.end():m.end() + int(m.group(1))] if m else symbol


def test_one_pair_of_table_kernels(kernels):
    """prev and table of a seek point come from one kernel pair, whichever call builds the index"""
    names = sorted(n for n in map(function_name, kernels) if "seek" in n and n.endswith(("_last", "_carry")))
    assert names == ["seekpx_carry", "seekpx_last"], names
