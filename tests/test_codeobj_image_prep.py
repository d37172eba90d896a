"""Static facts about image_resize_h_kernel and image_resize_v_kernel (csrc/image_prep.hip), read from the code object's metadata (CPU,
-m "not gpu"; pattern of tests/test_codeobj_bert.py).  Skipped when the library has not been built."""
import os

import pytest

from tests import _codeobj

LIB = os.environ.get("OMG_CODEOBJ_LIB") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "omg_amd", "csrc", "libomg_hip.so")
pytestmark = pytest.mark.skipif(not _codeobj.available(LIB), reason="libomg_hip.so not built (python -c 'import __graft_entry__ as g; g.build()')")


@pytest.fixture(scope="module")
def kernels():
    return _codeobj.kernels(LIB)


def test_the_resize_kernels_use_no_scratch_and_spill_nothing(kernels):
    """One horizontal kernel; three vertical ones: uint8 HWC, planar 16-bit, planar fp32.  Tap loops have run-time bounds and no
    per-lane array: no private segment, no spills, no dynamic stack."""
    h = {n: k for n, k in kernels.items() if "image_resize_h_kernel" in n}
    v = {n: k for n, k in kernels.items() if "image_resize_v_kernel" in n}
    assert len(h) == 1 and len(v) == 3, (list(h), list(v))
    for n, k in {**h, **v}.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (n, k)
        assert not k.get("uses_dynamic_stack", False), n
        assert k["max_flat_workgroup_size"] == 256, (n, k)


def test_lds_is_the_staged_segment_and_the_lookup_table(kernels):
    """Four rows of 4 KiB in the horizontal pass; 768 table entries of the output's element in the vertical one."""
    for n, k in kernels.items():
        if "image_resize_h_kernel" in n:
            assert k["group_segment_fixed_size"] == 4 * 4096, (n, k["group_segment_fixed_size"])
        if "image_resize_v_kernel" in n:
            assert k["group_segment_fixed_size"] <= 768 * 4, (n, k["group_segment_fixed_size"])
