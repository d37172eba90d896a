"""Static facts about gemm_skinny_kernel and bert_embed_ln_kernel (csrc/bert.hip), read from the code object (CPU, -m "not gpu"; pattern
of tests/test_codeobj_wino.py).  Skipped when the library has not been built."""
import os

import pytest

from tests import _codeobj

LIB = os.environ.get("OMG_CODEOBJ_LIB") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "omg_amd", "csrc", "libomg_hip.so")
pytestmark = pytest.mark.skipif(not _codeobj.available(LIB), reason="libomg_hip.so not built (python -c 'import __graft_entry__ as g; g.build()')")


@pytest.fixture(scope="module")
def kernels():
    return _codeobj.kernels(LIB)


def test_the_skinny_gemm_and_the_embedding_kernel_use_no_scratch_and_spill_nothing(kernels):
    """fp16 and bf16 of 1, 2 and 4 row blocks a workgroup; fp16 and bf16 of 1, 2, 4 and 8 vectors a lane."""
    sk = {n: k for n, k in kernels.items() if "gemm_skinny_kernel" in n}
    em = {n: k for n, k in kernels.items() if "bert_embed_ln_kernel" in n}
    assert len(sk) == 6 and len(em) == 8, (list(sk), list(em))
    for n, k in {**sk, **em}.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (n, k)
        assert not k.get("uses_dynamic_stack", False), n
    for needle in ("gemm_skinny_kernel", "bert_embed_ln_kernel"):
        for n, ins in _codeobj.disassembly(LIB, needle).items():
            assert not [x for x in ins if x.startswith("scratch_")], n


def test_the_skinny_gemm_admits_two_workgroups_a_compute_unit(kernels):
    """A workgroup is four waves, one a SIMD; a SIMD has 512 registers a lane (vector and accumulation together), a compute unit 160 KiB
    of LDS: two resident workgroups need at most 256 registers a wave and 80 KiB each.  The second workgroup's loads run under the
    first one's fold and epilogue."""
    sk = {n: k for n, k in kernels.items() if "gemm_skinny_kernel" in n}
    assert sk
    for n, k in sk.items():
        assert k["max_flat_workgroup_size"] == 256, (n, k)
        assert k["vgpr_count"] <= 256, (n, k["vgpr_count"], k["agpr_count"])          # vgpr_count is the wave's whole allocation
        assert k["group_segment_fixed_size"] <= 80 * 1024, (n, k["group_segment_fixed_size"])
    for n, ins in _codeobj.disassembly(LIB, "gemm_skinny_kernel").items():
        assert [x for x in ins if x.startswith("v_mfma_f32_16x16x32")], n
