"""LoHa, LoKr and DoRA adapters, CPU side (-m "not gpu"): the file loader in the kohya / LyCORIS namespace (diffusers and SGM module names)
and PEFT's magnitude vector, the refusals by message, the round trip, the float64 oracle's self-check, the bank's refusals that need no
device, and the ABI of the two merge entries."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from omg_amd import loaders
from omg_amd.lora import LoraAdapter, LoraBank, LoraTerm
from omg_amd.unet import UNet2DConditionModel, UNetConfig
from tests import _lycoris_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (module path, kohya flat name, SGM flat name): a Linear, a 3x3 and a 1x1 convolution of the tiny UNet
LIN = ("down_blocks.1.attentions.0.transformer_blocks.0.attn1.to_q", "down_blocks_1_attentions_0_transformer_blocks_0_attn1_to_q",
       "input_blocks_4_1_transformer_blocks_0_attn1_to_q")
C3 = ("down_blocks.0.resnets.0.conv1", "down_blocks_0_resnets_0_conv1", "input_blocks_1_0_in_layers_2")
C1 = ("down_blocks.1.resnets.0.conv_shortcut", "down_blocks_1_resnets_0_conv_shortcut", "input_blocks_4_0_skip_connection")
TARGETS = {"linear": LIN, "conv3": C3, "conv1": C1}


@pytest.fixture(scope="module")
def tiny():
    return UNet2DConditionModel(UNetConfig.tiny(), device="meta")


def shape_of(unet, mod):
    m = unet.get_submodule(mod)
    return (m.out_features, m.in_features) if hasattr(m, "in_features") else (m.cout, m.cin, m.ksize, m.ksize)


def randn(g, *shape):
    return torch.randn(*shape, generator=g)


def make_entries(family, shape, g, r=4, kron=("full", "full"), split=(4, 8)):
    """File tensors {suffix: tensor} of one module and the oracle's (kind, factors) for them."""
    out, cin = shape[0], shape[1]
    kk = shape[2] * shape[3] if len(shape) == 4 else 1
    if family == "plain":
        down = randn(g, r, *shape[1:])
        up = randn(g, out, r, 1, 1) if len(shape) == 4 else randn(g, out, r)
        return {"lora_down.weight": down, "lora_up.weight": up}, ("plain", [down, up])
    if family == "hada":
        f = {"hada_w1_a": randn(g, out, r), "hada_w1_b": randn(g, r, cin * kk), "hada_w2_a": randn(g, out, r), "hada_w2_b": randn(g, r, cin * kk)}
        return f, ("hada", [f[n] for n in ("hada_w1_a", "hada_w1_b", "hada_w2_a", "hada_w2_b")])
    a, b = split
    c, d = out // a, cin // b
    f = {}
    if kron[0] == "full":
        f["lokr_w1"] = randn(g, a, b)
        w1 = O.kron_operand(f["lokr_w1"])
    else:
        f["lokr_w1_a"], f["lokr_w1_b"] = randn(g, a, r), randn(g, r, b)
        w1 = O.kron_operand(None, f["lokr_w1_a"], f["lokr_w1_b"])
    if kron[1] == "full":
        f["lokr_w2"] = randn(g, c, d, *shape[2:])
        w2 = O.kron_operand(f["lokr_w2"])
    else:
        f["lokr_w2_a"], f["lokr_w2_b"] = randn(g, c, r), randn(g, r, d * kk)
        w2 = O.kron_operand(None, f["lokr_w2_a"], f["lokr_w2_b"])
    return f, ("kron", [w1, w2])


def dense_from_kernel_term(kind, f):
    """What omg_lora_merge forms from the factors ``LoraTerm.kernel_term`` hands it (packed columns), in float64."""
    f = [t.double() for t in f]
    if kind == "plain":
        return f[0] @ f[1]
    if kind == "hada":
        return (f[0] @ f[1]) * (f[2] @ f[3])
    w1, w2 = f                                                     # [a, b], [c, taps, d]: column = tap * (b d) + ib * d + id
    a, b = w1.shape
    c, taps, d = w2.shape
    return torch.einsum("ab,ctd->actbd", w1, w2).reshape(a * c, taps * b * d)


def term_delta(unet, mod, term):
    shape = shape_of(unet, mod)
    k = shape[2] if len(shape) == 4 else 1
    return dense_from_kernel_term(*term.kernel_term(shape[0], shape[1], k, "cpu"))


# ------------------------------------------------------------------ loader: every family on every target, both namings
@pytest.mark.parametrize("naming", ["kohya", "sgm"])
@pytest.mark.parametrize("target", ["linear", "conv3", "conv1"])
@pytest.mark.parametrize("family", ["hada", "kron", "plain+dora", "hada+dora", "kron+dora"])
def test_each_family_loads_to_the_oracle_delta(tiny, family, target, naming):
    mod, kflat, sflat = TARGETS[target]
    shape = shape_of(tiny, mod)
    g = torch.Generator().manual_seed(len(family) * 100 + len(target) * 10 + len(naming))
    base, dora = family.split("+")[0], family.endswith("+dora")
    f, (kind, fo) = make_entries(base, shape, g)
    pre = "lora_unet_" + (kflat if naming == "kohya" else sflat)
    sd = {f"{pre}.{n}": t for n, t in f.items()}
    sd[f"{pre}.alpha"] = torch.tensor(2.0)
    m = torch.rand(shape[0], generator=g) + 0.5
    if dora:
        sd[f"{pre}.dora_scale"] = m.reshape(-1, *([1] * (len(shape) - 1)))
    ad = loaders.load_lora_adapter(tiny, sd, "x")
    assert set(ad.terms) == {mod} and not ad.weights and ad.rank == 0
    t = ad.terms[mod]
    assert t.kind == kind
    # hada: alpha / r = 2 / 4; kron of two full matrices: 1 whatever alpha holds; plain: 2 / 4
    assert t.factor == (1.0 if base == "kron" else 0.5) and t.alpha == 2.0
    want = O.pack(O.delta(kind, fo, shape))
    assert (term_delta(tiny, mod, t) - want).abs().max() <= 1e-6 * want.abs().max()
    if dora:
        assert torch.equal(t.magnitude, m)
    else:
        assert t.magnitude is None


@pytest.mark.parametrize("target", ["linear", "conv3"])
@pytest.mark.parametrize("w1", ["full", "factored"])
@pytest.mark.parametrize("w2", ["full", "factored"])
@pytest.mark.parametrize("alpha", [None, 3.0])
def test_lokr_in_all_four_combinations_with_and_without_alpha(tiny, target, w1, w2, alpha):
    mod, kflat, _ = TARGETS[target]
    shape = shape_of(tiny, mod)
    g = torch.Generator().manual_seed(7)
    f, (kind, fo) = make_entries("kron", shape, g, r=2, kron=(w1, w2))
    sd = {f"lora_unet_{kflat}.{n}": t for n, t in f.items()}
    if alpha is not None:
        sd[f"lora_unet_{kflat}.alpha"] = torch.tensor(alpha)
    t = loaders.load_lora_adapter(tiny, sd, "x").terms[mod]
    factored = "factored" in (w1, w2)
    assert t.rank == (2 if factored else None)
    assert t.factor == (alpha / 2 if alpha is not None and factored else 1.0)          # full x full ignores alpha
    want = O.pack(O.delta(kind, fo, shape))
    assert (term_delta(tiny, mod, t) - want).abs().max() <= 1e-5 * want.abs().max()


def test_hada_without_alpha_has_factor_one(tiny):
    f, _ = make_entries("hada", shape_of(tiny, LIN[0]), torch.Generator().manual_seed(1))
    t = loaders.load_lora_adapter(tiny, {f"lora_unet_{LIN[1]}.{n}": v for n, v in f.items()}, "x").terms[LIN[0]]
    assert t.alpha is None and t.factor == 1.0 and t.rank == 4


@pytest.mark.parametrize("suffix", ["", ".weight", ".default", ".default.weight"])
def test_peft_magnitude_vector_on_a_peft_pair(tiny, suffix):
    mod = C3[0]
    g = torch.Generator().manual_seed(3)
    a, b, m = randn(g, 4, 64, 3, 3), randn(g, 64, 4, 1, 1), torch.rand(64, generator=g) + 0.5
    sd = {f"unet.{mod}.lora_A.weight": a, f"unet.{mod}.lora_B.weight": b, f"unet.{mod}.lora_magnitude_vector{suffix}": m}
    ad = loaders.load_lora_adapter(tiny, sd, "x")
    t = ad.terms[mod]
    assert t.kind == "plain" and t.factor == 1.0 and torch.equal(t.magnitude, m) and not ad.weights
    assert torch.equal(t.factors["lora_down"], a) and torch.equal(t.factors["lora_up"], b.reshape(64, 4))


def test_round_trip_through_lora_state_dict(tiny):
    g = torch.Generator().manual_seed(11)
    sd = {}
    for (mod, kflat, _), fam, kw in ((LIN, "hada", {}), (C3, "kron", dict(kron=("factored", "full"))), (C1, "plain", {})):
        f, _ = make_entries(fam, shape_of(tiny, mod), g, **kw)
        sd.update({f"lora_unet_{kflat}.{n}": t for n, t in f.items()})
        sd[f"lora_unet_{kflat}.alpha"] = torch.tensor(2.0)
    sd[f"lora_unet_{C1[1]}.dora_scale"] = torch.rand(128, 1, 1, 1, generator=g) + 0.5
    sd[f"lora_unet_{LIN[1]}.dora_scale"] = torch.rand(128, 1, generator=g) + 0.5
    te = "lora_te1_text_model_encoder_layers_0_self_attn_q_proj"
    fte, _ = make_entries("hada", (32, 32), g)
    sd.update({f"{te}.{n}": t for n, t in fte.items()})
    ad = loaders.load_lora_adapter(tiny, sd, "x")
    assert isinstance(ad.text_encoder[1]["text_model.encoder.layers.0.self_attn.q_proj"], LoraTerm)
    back = loaders.lora_state_dict(ad, "kohya")
    assert set(back) == set(sd)
    for k, v in sd.items():
        assert torch.equal(back[k].reshape(v.shape).float(), v.float()), k
    again = loaders.load_lora_adapter(tiny, back, "x")
    assert set(again.terms) == set(ad.terms)
    for mod, t in ad.terms.items():
        u = again.terms[mod]
        assert (u.kind, u.alpha, set(u.factors)) == (t.kind, t.alpha, set(t.factors))
        assert all(torch.equal(u.factors[n], t.factors[n]) for n in t.factors) and torch.equal(u.magnitude, t.magnitude) if t.magnitude is not None else u.magnitude is None
    with pytest.raises(ValueError, match="kohya"):
        loaders.lora_state_dict(ad, "peft")


def test_text_encoder_entries_carry_the_fp32_delta(tiny):
    g = torch.Generator().manual_seed(5)
    f, (kind, fo) = make_entries("kron", (32, 32), g, r=2, kron=("full", "factored"), split=(4, 4))
    pre = "lora_te2_text_model_encoder_layers_1_mlp_fc1"
    sd = {f"{pre}.{n}": t for n, t in f.items()}
    sd[f"{pre}.alpha"] = torch.tensor(1.0)
    fl, _ = make_entries("plain", shape_of(tiny, LIN[0]), g)
    sd.update({f"lora_unet_{LIN[1]}.{n}": t for n, t in fl.items()})
    ad = loaders.load_lora_adapter(tiny, sd, "x")
    t = ad.text_encoder[2]["text_model.encoder.layers.1.mlp.fc1"]
    assert t.factor == 0.5 and t.dense().dtype == torch.float32
    want = O.delta(kind, fo, (32, 32))
    assert (t.dense().double() - want).abs().max() <= 1e-6 * want.abs().max()


# ------------------------------------------------------------------ refusals, each by its message
def _plain_sd(tiny, mod=C3[0]):
    cin, cout, k = loaders.conv_module_paths(tiny)[mod]
    return {f"unet.{mod}.lora_A.weight": torch.zeros(4, cin, k, k), f"unet.{mod}.lora_B.weight": torch.zeros(cout, 4, 1, 1)}


def _hada_sd(tiny, g=None):
    f, _ = make_entries("hada", shape_of(tiny, LIN[0]), g or torch.Generator().manual_seed(0))
    return {f"lora_unet_{LIN[1]}.{n}": t for n, t in f.items()}


@pytest.mark.parametrize("suffix,words", [("lora_mid.weight", "Tucker-decomposed"), ("hada_t1", "Tucker-decomposed"), ("hada_t2", "Tucker-decomposed"),
                                          ("lokr_t2", "Tucker-decomposed")])
def test_tucker_forms_are_refused(tiny, suffix, words):
    sd = _hada_sd(tiny)
    sd[f"lora_unet_{LIN[1]}.{suffix}"] = torch.zeros(4, 4, 3, 3)
    with pytest.raises(loaders.LoaderError, match=r"LoHa / LoKr / Tucker.*" + words + ".*" + re.escape(suffix.split(".")[0])):
        loaders.load_lora_adapter(tiny, sd, "x")


def test_the_other_refusals(tiny):
    pre = f"lora_unet_{LIN[1]}"
    ok = _hada_sd(tiny)
    loaders.load_lora_adapter(tiny, ok, "ok")

    def refused(sd, words):
        with pytest.raises(loaders.LoaderError, match=r"LoHa / LoKr / Tucker.*" + words):
            loaders.load_lora_adapter(tiny, sd, "x")

    # the over-input magnitude of LyCORIS
    refused({**ok, f"{pre}.dora_scale": torch.ones(1, 128)}, "over the input axis")
    # a magnitude of the wrong length / shape
    refused({**ok, f"{pre}.dora_scale": torch.ones(64, 1)}, r"magnitude of shape \(64, 1\)")
    refused({**ok, f"{pre}.dora_scale": torch.ones(128, 2)}, "magnitude of shape")
    # two algebras on one module
    refused({**ok, f"{pre}.lokr_w1": torch.ones(4, 8), f"{pre}.lokr_w2": torch.ones(32, 16)}, "LoHa and LoKr factors on one module")
    refused({**ok, f"{pre}.lora_down.weight": torch.ones(4, 128), f"{pre}.lora_up.weight": torch.ones(128, 4)}, "plain lora_down / lora_up pair and LoHa / LoKr")
    # incomplete factor sets
    bad = dict(ok); del bad[f"{pre}.hada_w2_b"]
    refused(bad, "incomplete LoHa factor set")
    refused({f"{pre}.lokr_w1": torch.ones(4, 8)}, "incomplete LoKr factor set")
    refused({f"{pre}.lokr_w1": torch.ones(4, 8), f"{pre}.lokr_w2_a": torch.ones(32, 2)}, "incomplete LoKr factor set")
    refused({f"{pre}.lokr_w1": torch.ones(4, 8), f"{pre}.lokr_w1_a": torch.ones(4, 2), f"{pre}.lokr_w1_b": torch.ones(2, 8), f"{pre}.lokr_w2": torch.ones(32, 16)},
            "incomplete LoKr factor set")
    refused({**_plain_sd(tiny), f"{pre}.dora_scale": torch.ones(128, 1)}, "magnitude without the factors")
    # mis-shaped factors
    refused({**ok, f"{pre}.hada_w2_b": torch.ones(4, 64)}, "LoHa factor shapes")
    c3 = f"lora_unet_{C3[1]}"
    refused({f"{c3}.lokr_w1": torch.ones(4, 8), f"{c3}.lokr_w2": torch.ones(16, 8)}, "LoKr factor shapes")            # a 3x3 layer needs [c, d, 3, 3]
    refused({f"{c3}.lokr_w1": torch.ones(4, 8), f"{c3}.lokr_w2": torch.ones(16, 4, 3, 3)}, "LoKr factor shapes")
    # a DoRA magnitude on a text-encoder module, in both namespaces
    te = "lora_te1_text_model_encoder_layers_0_self_attn_q_proj"
    refused({**ok, f"{te}.lora_down.weight": torch.ones(4, 32), f"{te}.lora_up.weight": torch.ones(32, 4), f"{te}.dora_scale": torch.ones(32, 1)},
            "text-encoder module")
    refused({**ok, "text_encoder.text_model.encoder.layers.0.self_attn.q_proj.lora_magnitude_vector": torch.ones(32)}, "text-encoder module")
    # these families outside the kohya / LyCORIS namespace
    refused({**ok, f"unet.{LIN[0]}.hada_w1_a": torch.ones(128, 4)}, "not a key of the kohya / LyCORIS namespace")
    # conv_in / conv_out stay refused
    with pytest.raises(loaders.LoaderError, match="conv_in / conv_out"):
        loaders.load_lora_adapter(tiny, {**ok, "lora_unet_conv_in.hada_w1_a": torch.ones(64, 4)}, "x")
    with pytest.raises(loaders.LoaderError, match="conv_in / conv_out"):
        loaders.load_lora_adapter(tiny, {**ok, "unet.conv_out.lora_magnitude_vector": torch.ones(4)}, "x")


# ------------------------------------------------------------------ plain files are what they were; mixed files
def test_a_plain_only_file_gives_todays_adapter(tiny):
    g = torch.Generator().manual_seed(9)
    sd, want = {}, {}
    for (mod, kflat, sflat), alpha in ((LIN, 2.0), (C3, None), (C1, 8.0)):
        f, _ = make_entries("plain", shape_of(tiny, mod), g)
        sd.update({f"lora_unet_{sflat}.{n}": t for n, t in f.items()})
        if alpha is not None:
            sd[f"lora_unet_{sflat}.alpha"] = torch.tensor(alpha)
        b = f["lora_up.weight"].reshape(f["lora_up.weight"].shape[0], 4)
        want[mod] = (f["lora_down.weight"], b * (alpha / 4) if alpha is not None else b)        # alpha / r folded into the up matrix
    ad = loaders.load_lora_adapter(tiny, sd, "p")
    assert ad.terms == {} and ad.rank == 4 and set(ad.weights) == set(want) and ad.text_encoder == {}
    for mod, (a, b) in want.items():
        assert torch.equal(ad.weights[mod][0], a) and torch.equal(ad.weights[mod][1], b) and ad.scaling(mod) == 1.0
    assert LoraAdapter("q", dict(ad.weights)).terms == {}                                          # the constructor as it was


def test_a_mixed_file(tiny):
    g = torch.Generator().manual_seed(13)
    sd = {}
    for (mod, kflat, _), fam in ((LIN, "plain"), (C3, "hada"), (C1, "kron")):
        f, _ = make_entries(fam, shape_of(tiny, mod), g)
        sd.update({f"lora_unet_{kflat}.{n}": t for n, t in f.items()})
    ad = loaders.load_lora_adapter(tiny, sd, "m")
    assert set(ad.weights) == {LIN[0]} and ad.rank == 4
    assert {m: t.kind for m, t in ad.terms.items()} == {C3[0]: "hada", C1[0]: "kron"}
    with pytest.raises(ValueError, match="both a plain pair and a term"):
        LoraAdapter("bad", dict(ad.weights), terms={LIN[0]: ad.terms[C3[0]]})


# ------------------------------------------------------------------ the bank's refusals that need no device
def test_segment_mode_and_the_torch_merge_refuse_non_plain_terms(tiny):
    f, _ = make_entries("hada", shape_of(tiny, LIN[0]), torch.Generator().manual_seed(0))
    ad = loaders.load_lora_adapter(tiny, {f"lora_unet_{LIN[1]}.{n}": t for n, t in f.items()}, "loha")
    bank = LoraBank(tiny, [ad])
    from omg_amd._lib import OmgHipError
    with pytest.raises(OmgHipError, match=r"adapter 'loha', module " + re.escape(LIN[0]) + ".*mode='merged'"):
        bank.build([(("loha", 1.0),)], mode="segment")
    with pytest.raises(OmgHipError, match=re.escape(LIN[0]) + ".*merge='torch'"):
        bank.build([(("loha", 1.0),)], mode="merged", merge="torch")
    with pytest.raises(ValueError):
        bank.build([(("loha", 1.0),)], merge="fast")


# ------------------------------------------------------------------ the oracle's self-check
def _self_check_case(conv):
    g = torch.Generator().manual_seed(21 + conv)
    shape = (16, 8, 3, 3) if conv else (16, 24)
    W = randn(g, *shape) * 0.2
    fk, (_, ko) = make_entries("kron", shape, g, split=(4, 2))
    fp, (_, po) = make_entries("plain", shape, g, r=4)
    terms = []
    for kind, fo, r, scale in (("kron", ko, 1, 0.8), ("plain", po, 4, 0.56)):
        fo = [t * 0.3 for t in fo]
        d = O.delta(kind, fo, shape)
        n = (W.double() + scale * 0.25 * d).pow(2).sum(tuple(range(1, len(shape)))).sqrt()
        m = (n * (torch.rand(shape[0], generator=g).double() + 0.5)).float()
        terms.append({"kind": kind, "f": fo, "scale": scale, "factor": 0.25, "m": m, "r": r})
    return W, terms


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("fault", O.FAULTS)
def test_every_deliberate_defect_moves_the_result_by_more_than_100_bounds(fault, dtype):
    """The oracle with one defect against itself without, on seeded inputs: a Linear for every defect, the convolution where the defect is
    about the column order.  ``|defective - exact| > 100 x bound`` somewhere — a kernel or a build with that defect cannot pass."""
    W, terms = _self_check_case(conv=fault == "conv_cin_order")
    exact, S, r = O.slot_weight(W, terms)
    wrong, _, _ = O.slot_weight(W, terms, fault=fault)
    ratio = ((wrong - exact).abs() / O.bound(wrong, exact, S, r, dtype)).max().item()
    print(f"{fault} {dtype}: max |defective - exact| / bound = {ratio:.1f}")
    assert ratio > 100.0
    assert (O.slot_weight(W, terms)[0] - exact).abs().max() == 0


def test_the_oracle_reduces_to_the_plain_merge_and_to_torch_kron():
    g = torch.Generator().manual_seed(2)
    W, down, up = randn(g, 6, 8), randn(g, 3, 8), randn(g, 6, 3)
    exact, S, r = O.slot_weight(W, [{"kind": "plain", "f": [down, up], "scale": 0.8, "factor": 0.5, "m": None, "r": 3}])
    assert (exact - (W.double() + 0.4 * up.double() @ down.double())).abs().max() < 1e-14 and r == 3
    assert bool((S >= exact.abs() - 1e-12).all())
    w1, w2 = randn(g, 2, 4), randn(g, 3, 2, 3, 3)
    d = O.delta("kron", [w1, w2], (6, 8, 3, 3))
    assert d[1 * 3 + 2, 3 * 2 + 1, 0, 2] == w1[1, 3].double() * w2[2, 1, 0, 2].double()
    # a magnitude equal to the norm is no magnitude
    t = {"kind": "plain", "f": [down, up], "scale": 1.0, "factor": 1.0, "m": None, "r": 3}
    n = (W.double() + up.double() @ down.double()).norm(dim=1)
    with_m, _, _ = O.slot_weight(W, [dict(t, m=n)])
    assert (with_m - O.slot_weight(W, [t])[0]).abs().max() < 1e-14
    # the 16-bit spacing
    assert O.ulp16(torch.tensor([1.0, 1.5, 2.0, 2.0 ** -20], dtype=torch.float64), torch.float16).tolist() == [2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -24]
    assert O.ulp16(torch.tensor([1.0], dtype=torch.float64), torch.bfloat16).item() == 2.0 ** -7


# ------------------------------------------------------------------ ABI
def test_header_and_ctypes_prototypes_agree_and_the_abi_version_stays():
    from omg_amd import _lib
    header = open(os.path.join(ROOT, "include", "omg_hip.h")).read()
    assert re.search(r"#define\s+OMG_ABI_VERSION\s+6\b", header)
    for name, nargs in (("omg_lora_rownorm", 7), ("omg_lora_merge", 2)):
        m = re.search(r"^int " + name + r"\(([^;]*)\);", header, re.M)
        assert m is not None, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.SYMBOLS[name][1]), name
    code = ('#include <stdio.h>\n#include <stddef.h>\n#include "omg_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu %d %d\\n",sizeof(omg_lora_term),'
            'sizeof(omg_lora_merge_args),offsetof(omg_lora_term,f0),offsetof(omg_lora_term,gain),offsetof(omg_lora_merge_args,terms),'
            'OMG_LORA_MAX_TERMS,OMG_LORA_KRON);return 0;}')
    exe = os.path.join(ROOT, "tests", "_sizes_lora_merge.out")
    subprocess.run(["gcc", "-x", "c", "-I", os.path.join(ROOT, "include"), "-o", exe, "-"], input=code.encode(), check=True)
    try:
        out = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    finally:
        os.remove(exe)
    assert out == [ctypes.sizeof(_lib.LoraTermDesc), ctypes.sizeof(_lib.LoraMergeArgs), _lib.LoraTermDesc.f0.offset, _lib.LoraTermDesc.gain.offset,
                   _lib.LoraMergeArgs.terms.offset, _lib.LORA_MAX_TERMS, _lib.LORA_KRON]
    lib = _lib.lib()
    assert lib.omg_abi_version() == 6
    assert hasattr(lib, "omg_lora_merge") and hasattr(lib, "omg_lora_rownorm")
    # appended: the two entries follow everything the header declared before
    assert header.index("int omg_lora_rownorm(") > header.index("int omg_image_resize_v(")
