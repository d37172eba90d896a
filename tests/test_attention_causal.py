"""`omg_attn_fwd_causal` against the built library, no GPU (-m "not gpu"): the entry point exists under ABI 6, the code object holds
an f16 and a bf16 causal instance of the resident-K/V kernel, and that instance meets the bounds tests/test_codeobj.py sets for the
attention kernels.

The causal kernel is `attn_fwd_causal_kernel6`, NOT a name that contains `attn_fwd_kernel6`: tests/test_codeobj.py selects by that
substring and asserts that it finds exactly two instances (f16, bf16), so two more under the same substring would fail it.  The bounds
it would have applied — two workgroups per CU, no scratch, no scratch access between the first and the last MFMA — are asserted here
under the kernel's own name."""
import os

from omg_amd import _lib
from tests import _codeobj

CAUSAL = "attn_fwd_causal_kernel6"


def test_the_causal_entry_is_exported_under_abi_6():
    lib = _lib.lib()
    assert "omg_attn_fwd_causal" in _lib.SYMBOLS and hasattr(lib, "omg_attn_fwd_causal")
    assert lib.omg_abi_version() == 6
    header = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "..", "..", "include", "omg_hip.h")).read()
    assert "int omg_attn_fwd_causal(const omg_attn_args* a, void* stream);" in header


def test_the_code_object_holds_an_f16_and_a_bf16_causal_instance_within_the_attention_bounds():
    ks = {n: k for n, k in _codeobj.kernels(_lib.LIB_PATH).items() if CAUSAL in n}
    assert len(ks) == 2 and any("IDF16_E" in n for n in ks) and any("IDF16bE" in n for n in ks), list(ks)
    for n, k in ks.items():
        assert k["wavefront_size"] == 64 and not k.get("uses_dynamic_stack", False), n
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, n
        assert k["vgpr_count"] + k.get("agpr_count", 0) <= 256, n      # 512 registers per SIMD lane: two waves
        assert k["group_segment_fixed_size"] <= 80 * 1024, n            # 160 KB of LDS: two workgroups
    dis = _codeobj.disassembly(_lib.LIB_PATH, CAUSAL)
    assert len(dis) == 2
    for n, ins in dis.items():
        mf = [i for i, x in enumerate(ins) if x.startswith("v_mfma")]
        assert mf, n
        assert not [ins[i] for i in range(mf[0], mf[-1]) if ins[i].startswith("scratch_")], n


def test_the_causal_entry_rejects_on_the_host_what_its_kernel_cannot_serve():
    """Validation happens before any launch, so it needs no device: more than 128 keys, and row-major V without a V^T image."""
    import ctypes as C
    lib = _lib.lib()
    a = _lib.AttnArgs()
    a.dtype, a.B, a.heads, a.Nq, a.Nkv = 0, 1, 1, 129, 129
    # Q, K, O stay NULL in both calls: were a check below missing, the null-operand check behind it would still return before a launch
    a.ldq = a.ldk = a.ldo = 64
    a.q_bstride = a.k_bstride = a.o_bstride = 129 * 64
    a.Nkv_pad, a.scale, a.out_scale = 192, 0.125, 1.0
    assert lib.omg_attn_fwd_causal(C.byref(a), None) == -1 and b"128" in lib.omg_last_error()
    a.Nq = a.Nkv = 80
    a.Nkv_pad = 128
    a.Vt, a.V, a.ldv, a.v_bstride = None, 4096, 64, 80 * 64
    assert lib.omg_attn_fwd_causal(C.byref(a), None) == -1 and b"Vt" in lib.omg_last_error()
