"""GroundingDINO's feature enhancer without a GPU: the plain-torch oracle (tests/gdino_torch.py) against the live library classes and
the fixture, the fixture's regeneration and sensitivity, the module's key / shape / prefix contract, its refusals, and the static
properties of the new kernels' code objects."""
import os
import sys

import numpy as np
import pytest
import torch

from omg_amd import _lib
from omg_amd import gdino as hip_gdino
from tests import _codeobj
from tests import gdino_torch as gt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "gdino_golden.npz")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_gdino as mg  # noqa: E402

CONFIGS = ["a", "b"]


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLD)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def regenerated():
    return mg.build()


def case(gold, name):
    cfg = gt.small_cfg(name)
    return cfg, gt.seed_state(cfg, int(gold[name + ".cfg_seed"])), gt.seeded_inputs(cfg, int(gold[name + ".cfg_input_seed"]))


@pytest.mark.parametrize("name", CONFIGS)
def test_oracle_equals_the_live_library_and_the_fixture(gold, name):
    """Per layer and for the neck, to fp32 rounding (1e-5 of the state's rms; the library and the oracle order a few sums differently)."""
    cfg, sd, inp = case(gold, name)
    vs, ts, maps = mg.library_run(cfg, sd, inp)
    o = mg.oracle(cfg, sd, inp)
    assert o["spatial"] == [tuple(m.shape[-2:]) for m in maps] and sum(h * w for h, w in o["spatial"]) == {"a": 343, "b": 319}[name]
    for l, (a, b) in enumerate(zip(o["neck_maps"], maps)):
        assert gt.rel_rms(a, b) < 1e-5, ("neck", l)
    iv, it = torch.from_numpy(gold[name + ".idx.vision"]), torch.from_numpy(gold[name + ".idx.text"])
    for i in range(cfg["encoder_layers"] + 1):
        assert gt.rel_rms(o["vision_states"][i], vs[i]) < 1e-5 and gt.rel_rms(o["text_states"][i], ts[i]) < 1e-5, i
        assert gt.rel_rms(o["vision_states"][i][:, iv], torch.from_numpy(gold[f"{name}.vision{i}"])) < 1e-5, i
        assert gt.rel_rms(o["text_states"][i][:, it], torch.from_numpy(gold[f"{name}.text{i}"])) < 1e-5, i
    if name == "a":
        assert float(o["valid_ratios"][1].min()) < 0.7 and float(o["valid_ratios"][0].min()) == 1.0


def test_the_fixture_regenerates_identically(gold, regenerated):
    """Seeds, keys, inputs, masks and positions bit for bit; the weights' float64 checksums to the order of a sum; the recorded states to
    fp32 rounding (1e-5 of their rms: the host's BLAS may order a sum differently); the twin and defect figures, which are statistics of
    rounding noise, to 5 %."""
    assert sorted(regenerated) == sorted(gold)
    for k, v in regenerated.items():
        name = k.split(".", 1)[1]
        if v.dtype.kind != "f":
            assert np.array_equal(v, gold[k]), k
        elif name.startswith("sum."):
            np.testing.assert_allclose(v, gold[k], rtol=1e-9, atol=1e-9, err_msg=k)
        elif name.startswith(("twin_err.", "defect.")):
            np.testing.assert_allclose(v, gold[k], rtol=5e-2, err_msg=k)
        else:
            assert gt.rel_rms(torch.from_numpy(v), torch.from_numpy(gold[k])) < 1e-5, k
    assert os.path.getsize(GOLD) < 1_000_000


def test_the_fixture_is_sensitive(gold):
    """Every defect moves the last vision or text state of a config that has the mask it needs by 10 x the fp16 twin's figure."""
    for d in gt.DEFECTS:
        seen = False
        for name in CONFIGS:
            dv, dt = float(gold[f"{name}.defect.{d}.vision"]), float(gold[f"{name}.defect.{d}.text"])
            tv, tt = float(gold[name + ".twin_err.vision"][0]), float(gold[name + ".twin_err.text"][0])
            seen = seen or dv >= mg.SENSITIVITY * tv or dt >= mg.SENSITIVITY * tt
        assert seen, d


def test_key_and_shape_contract_prefix_and_strict_loading(gold):
    cfg, sd, _ = case(gold, "a")
    h = hip_gdino.GroundingDinoEncoder(cfg)
    assert h.shapes() == gt.shapes(cfg)
    m, hc = mg.library_model(cfg)
    lib = m.state_dict()
    assert all(k in lib and tuple(lib[k].shape) == s for k, s in h.shapes().items())
    # a GroundingDinoForObjectDetection state dict: "model." in front, the detector's other keys ignored
    full = {"model." + k: v for k, v in lib.items()}
    full["bbox_embed.0.layers.0.weight"] = torch.zeros(4, 4)
    assert h.load_state_dict(full, strict=True, prefix="model.") == ([], [])
    assert torch.equal(h.state_dict()["level_embed"], lib["level_embed"].half())
    # the library's config object is accepted as it is
    h2 = hip_gdino.GroundingDinoEncoder(hc)
    assert h2.shapes() == h.shapes()
    short = dict(sd)
    del short["level_embed"]
    with pytest.raises(_lib.OmgHipError, match="level_embed"):
        h.load_state_dict(short, strict=True)
    assert h.load_state_dict(short, strict=False)[0] == ["level_embed"]
    with pytest.raises(_lib.OmgHipError, match="encoder.layers.7"):
        h.load_state_dict(dict(sd, **{"encoder.layers.7.fusion_layer.vision_param": torch.zeros(256)}), strict=True)
    with pytest.raises(_lib.OmgHipError, match="text_projection.weight"):
        h.load_state_dict(dict(sd, **{"text_projection.weight": torch.zeros(256, 64)}))


def test_packed_operands(gold):
    cfg, sd, _ = case(gold, "a")
    h = hip_gdino.GroundingDinoEncoder(cfg, dtype=torch.bfloat16)
    h.load_state_dict(sd)
    pk = h._pk()
    f = "encoder.layers.1.fusion_layer."
    assert torch.equal(pk[f + "attn.vis.weight"][1024:], sd[f + "attn.values_vision_proj.weight"].bfloat16())
    assert torch.equal(pk[f + "attn.txt.bias"][:1024], sd[f + "attn.text_proj.bias"].bfloat16())
    want = (sd[f + "vision_param"].bfloat16().float()[:, None] * sd[f + "attn.out_vision_proj.weight"].bfloat16().float()).bfloat16()
    assert torch.equal(pk[f + "attn.out_vision.weight"], want)
    m = "encoder.layers.0.deformable_layer.self_attn."
    assert pk[m + "ow.weight"].shape == (384, 256) and torch.equal(pk[m + "ow.weight"][256:], sd[m + "attention_weights.weight"].bfloat16())
    assert pk["input_proj_vision.3.0.weight"].shape == (256, 3, 3, 256) and pk["input_proj_vision.0.0.weight"].shape == (256, 64)
    h.load_state_dict(sd)
    assert h._packed is None


@pytest.mark.parametrize("key,value", [("d_model", 128), ("encoder_attention_heads", 4), ("encoder_ffn_dim", 1024), ("encoder_n_points", 8),
                                       ("num_feature_levels", 5), ("activation_function", "gelu"), ("position_embedding_type", "learned"),
                                       ("max_text_len", 512)])
def test_refusals_name_the_config_key(key, value):
    cfg = gt.small_cfg("a")
    cfg[key] = value
    with pytest.raises(_lib.OmgHipError, match=f"'{key}'"):
        hip_gdino.GroundingDinoEncoder(cfg)


def test_training_and_cpu_inputs_are_refused(gold):
    cfg, sd, inp = case(gold, "a")
    h = hip_gdino.GroundingDinoEncoder(cfg)
    with pytest.raises(_lib.OmgHipError, match="fusion_droppath"):
        h.train()
    with pytest.raises(_lib.OmgHipError, match="no CPU fallback"):
        h(**inp)
    with pytest.raises(_lib.OmgHipError, match="float16 or bfloat16"):
        hip_gdino.GroundingDinoEncoder(cfg, dtype=torch.float32)


def test_exported_and_declared():
    import omg_amd
    assert omg_amd.GroundingDinoEncoder is hip_gdino.GroundingDinoEncoder
    lib = _lib.lib()
    for n in ("omg_msdeform_attn", "omg_attn_bi_vision", "omg_attn_bi_text", "omg_attn_bi_text_chunk", "omg_attn_bi_text_ws_floats", "omg_attn_masked"):
        assert hasattr(lib, n)
    assert lib.omg_abi_version() == 6
    assert "gdino.hip" in open(os.path.join(ROOT, "omg_amd", "csrc", "Makefile")).read()
    # the chunk is a function of N alone; the workspace follows from it
    assert [lib.omg_attn_bi_text_chunk(n) for n in (1, 64, 4096, 4097, 19947)] == [64, 64, 64, 128, 320]
    assert lib.omg_attn_bi_text_ws_floats(2, 4, 11, 343) == 2 * 4 * 6 * 11 * 258


def test_new_kernels_use_no_scratch():
    """Static, from the code objects in the library: every instance without scratch or spills.  Recorded (vector registers incl.
    accumulation registers / LDS bytes): msdeform_kernel 75 .. 128 / 0 (four waves per SIMD); attn_tiled_kernel at head_dim 256: 248 /
    70 720 (two workgroups per CU), at head_dim 64: 96 / 18 432; attn_fold_kernel 34 / 0."""
    ks = _codeobj.kernels(_lib.LIB_PATH)
    msd = {n: k for n, k in ks.items() if "msdeform_kernel" in n}
    att = {n: k for n, k in ks.items() if "attn_tiled_kernel" in n}
    fold = {n: k for n, k in ks.items() if "attn_fold_kernel" in n}
    assert len(msd) == 16 and len(att) == 6 and len(fold) == 2, (list(msd), list(att), list(fold))     # f16 / bf16 x L 1..4 x mask; x 3 entries
    for n, k in {**msd, **att, **fold}.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, n
        assert k["wavefront_size"] == 64 and not k.get("uses_dynamic_stack", False), n
        print(n, k["vgpr_count"], k.get("agpr_count", 0), k["group_segment_fixed_size"])
    for n, k in msd.items():
        assert k["vgpr_count"] <= 128 and k["group_segment_fixed_size"] == 0, (n, k["vgpr_count"])
    for n, k in att.items():
        assert k["vgpr_count"] <= 256, (n, k["vgpr_count"])
        assert k["group_segment_fixed_size"] <= (80 * 1024 if "Li256E" in n else 20 * 1024), n


def test_host_side_argument_checks():
    """Refusals that need no device: they are decided before anything is launched."""
    lib = _lib.lib()
    a = _lib.MsdeformArgs()
    a.dtype, a.B, a.N, a.Nq, a.heads, a.head_dim, a.L, a.points = 0, 1, 8, 8, 8, 32, 5, 4
    assert lib.omg_msdeform_attn(a, None) == -1 and b"levels" in lib.omg_last_error()
    a.L, a.head_dim = 1, 64
    assert lib.omg_msdeform_attn(a, None) == -1 and b"head_dim 32" in lib.omg_last_error()
    a.head_dim, a.dtype = 32, 2
    assert lib.omg_msdeform_attn(a, None) == -1 and b"dtype" in lib.omg_last_error()
    assert lib.omg_attn_bi_vision(0, 1, 4, 8, 300, None, 2048, 0, None, 2048, 0, None, 1.0, None, 1024, 0, None) == -1
    assert b"T at most 256" in lib.omg_last_error()
    assert lib.omg_attn_masked(0, 1, 4, 300, 8, None, 256, 0, None, 256, 0, None, 256, 0, None, 1.0, None, 256, 0, None) == -1
    assert b"at most 256" in lib.omg_last_error()
    assert lib.omg_attn_masked(0, 0, 4, 8, 8, None, 256, 0, None, 256, 0, None, 256, 0, None, 1.0, None, 256, 0, None) == 0       # B == 0: nothing to do
