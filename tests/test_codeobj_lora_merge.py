"""Static facts about lora_merge_kernel and lora_rownorm_kernel (csrc/lora_merge.hip), read from the code object's metadata alone (CPU,
-m "not gpu"; pattern of tests/test_codeobj_bert.py).  Skipped when the library has not been built."""
import os

import pytest

from tests import _codeobj

LIB = os.environ.get("OMG_CODEOBJ_LIB") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "omg_amd", "csrc", "libomg_hip.so")
pytestmark = pytest.mark.skipif(not _codeobj.available(LIB), reason="libomg_hip.so not built (python -c 'import __graft_entry__ as g; g.build()')")


@pytest.fixture(scope="module")
def kernels():
    ks = _codeobj.kernels(LIB)
    return {n: k for n, k in ks.items() if "lora_merge_kernel" in n}, {n: k for n, k in ks.items() if "lora_rownorm_kernel" in n}


def test_both_kernels_exist_for_fp16_and_bf16_and_use_no_scratch(kernels):
    merge, norm = kernels
    assert len(merge) == 2 and len(norm) == 2, (list(merge), list(norm))
    for n, k in {**merge, **norm}.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (n, k)
        assert not k.get("uses_dynamic_stack", False), n
        assert k["max_flat_workgroup_size"] == 256, (n, k)


def test_three_workgroups_fit_a_compute_unit(kernels):
    """A workgroup is four waves, one a SIMD; a SIMD has 512 registers a lane (vector and accumulation together): at most 168 a wave keeps
    three waves a SIMD resident (the sum, a term's two products and the second LoHa product of a 32 x 64 tile are 128 registers by
    themselves; held to 128 in all the merge spills); their factor loads from L2 hide each other's latency.  LDS: the merge's four
    32 x 68 fp32 tiles and 4 x 32 row coefficients (35,328 bytes: four workgroups would fit the 160 KiB of a compute unit), the norm's
    4 x 32 partial sums."""
    merge, norm = kernels
    for n, k in {**merge, **norm}.items():
        assert k["vgpr_count"] <= 168, (n, k["vgpr_count"], k.get("agpr_count"))          # vgpr_count is the wave's whole allocation
    assert all(k["group_segment_fixed_size"] == 4 * 32 * 68 * 4 + 4 * 32 * 4 for k in merge.values())
    assert all(k["group_segment_fixed_size"] == 4 * 32 * 4 for k in norm.values())
