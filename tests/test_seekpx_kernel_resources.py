"""The two kernels of qoimi_seek_index_from_pixels in the built library, without a GPU: no scratch and no spills (the lane's dwords and pixels
stay in registers), the LDS of seekpx_last is the tile's 64 words, and few enough registers for eight wavefronts per SIMD (512 / 8 = 64):
the kernels wait for memory, not for arithmetic."""
import os

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
