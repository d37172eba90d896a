"""Static facts about the Canny kernels (csrc/canny.hip), read from the code object's metadata (CPU, -m "not gpu"; pattern of
tests/test_codeobj_image_prep.py).  Skipped when the library has not been built."""
import os

import pytest

from tests import _codeobj

LIB = os.environ.get("OMG_CODEOBJ_LIB") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "omg_amd", "csrc", "libomg_hip.so")
pytestmark = pytest.mark.skipif(not _codeobj.available(LIB), reason="libomg_hip.so not built (python -c 'import __graft_entry__ as g; g.build()')")

NAMES = {"canny_nms_kernel": 2, "canny_label_tile_kernel": 1, "canny_border_union_kernel": 1, "canny_flatten_kernel": 1, "canny_edges_kernel": 4}


@pytest.fixture(scope="module")
def kernels():
    return {n: k for n, k in _codeobj.kernels(LIB).items() if "canny_" in n}


def test_the_kernels_are_all_there_use_no_scratch_and_spill_nothing(kernels):
    """Two NMS kernels (C = 1, 3), one each for the tile labels, the border unions and the flattening, four epilogues (uint8 HW, uint8
    HW3, planar 16-bit, planar fp32).  No per-lane array, no recursion: no private segment, no spills, no dynamic stack."""
    for stem, count in NAMES.items():
        assert sum(stem in n for n in kernels) == count, (stem, list(kernels))
    assert len(kernels) == sum(NAMES.values()), list(kernels)
    for n, k in kernels.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (n, k)
        assert not k.get("uses_dynamic_stack", False), n
        assert k["max_flat_workgroup_size"] == 256, (n, k)


def test_lds_is_what_the_design_says(kernels):
    """NMS: 20 staged source rows of ceil((68 C + 6) / 4) dwords, 16 x 64 packed (dx, dy) pairs, 18 rows of 68 16-bit
    magnitudes, 20 row offsets.  Tile labels: 18 x 66 32-bit labels, and up to 256 bytes the block-wide OR of the sweep keeps.  The
    other kernels use none."""
    for n, k in kernels.items():
        lds = k["group_segment_fixed_size"]
        if "canny_nms_kernel" in n:
            C = 3 if "ILi3E" in n else 1                            # the template argument in the mangled name
            assert C == 3 or "ILi1E" in n, n
            assert lds == 20 * ((68 * C + 6) // 4) * 4 + 16 * 64 * 4 + 18 * 68 * 2 + 20 * 4, (n, lds)
        elif "canny_label_tile_kernel" in n:
            assert 18 * 66 * 4 <= lds <= 18 * 66 * 4 + 256, (n, lds)
        else:
            assert lds == 0, (n, lds)
