"""Static facts about conv_f32_wino_kernel (csrc/conv_f32_wino.hip), read from the code object (CPU, -m "not gpu"; pattern of
tests/test_codeobj.py).  Skipped when the library has not been built."""
import os

import pytest

from tests import _codeobj

LIB = os.environ.get("OMG_CODEOBJ_LIB") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "omg_amd", "csrc", "libomg_hip.so")
pytestmark = pytest.mark.skipif(not _codeobj.available(LIB), reason="libomg_hip.so not built (python -c 'import __graft_entry__ as g; g.build()')")


def test_the_winograd_convolution_keeps_its_256_accumulators_in_registers():
    """One wave per SIMD holding all 16 transform positions of its 32 x 32 sub-block: 256 accumulator registers, no scratch, no spills
    (a spill reload in the K loop would wait on vmcnt, i.e. on the LDS-DMA of the next stage); 64 MFMAs per stage, and no global
    load to registers among them (the input transform reads the shared raw patch from LDS)."""
    inst = {n: k for n, k in _codeobj.kernels(LIB).items() if "conv_f32_wino_kernel" in n}
    assert len(inst) == 1, list(inst)
    for n, k in inst.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (n, k)
        assert k["agpr_count"] == 256 and k["vgpr_count"] <= 512 and k["max_flat_workgroup_size"] == 256, (n, k)
    for n, ins in _codeobj.disassembly(LIB, "conv_f32_wino_kernel").items():
        assert not [x for x in ins if x.startswith("scratch_")], n
        mf = [i for i, x in enumerate(ins) if x.startswith("v_mfma_f32_32x32x2_f32")]
        assert len(mf) == 64, (n, len(mf))
        loads = [x for x in ins[mf[0]:mf[-1]] if x.startswith(("buffer_load", "global_load", "flat_load"))]
        assert all(" lds" in x for x in loads), (n, [x for x in loads if " lds" not in x][:3])
