"""LoHa, LoKr and DoRA adapters through the bank and the callers' surfaces (-m gpu): a tiny UNet whose two adapters mix plain pairs, LoHa,
LoKr and DoRA magnitudes on Linear and convolution targets — two adapters in one slot — against oracle/unet.py on weights merged in float64 by
tests/_lycoris_oracle.py; every layer's slots against the derived bound; the torch and the kernel merge of plain adapters; the text encoder;
``compat``'s ``load_lora_weights``."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from omg_amd import _lib as L
from omg_amd import loaders, ops
from omg_amd.lora import LoraAdapter, LoraBank, LoraTerm
from omg_amd.modules import Conv2d, LoraState
from omg_amd.unet import UNet2DConditionModel, UNetConfig
from oracle import unet as ou
from tests import _conv_lora_oracle as co
from tests import _lycoris_oracle as O

DTYPES = [torch.float16, torch.bfloat16]
UNET_TOL = {torch.float16: 3e-2, torch.bfloat16: 2e-1}      # the UNet tolerance of tests/test_conv_lora_gpu.py (the module tolerance of tests/test_unet_gpu.py)
SCALE = 0.8
SLOTS = [(("a", 1.0),), (("a", 0.7), ("b", 0.5))]


def make_term(kind, shape, g, r, dora, W, alpha):
    """One module's term in the file layout: ``(LoraTerm for the engine, the oracle's dict without its slot scale)``."""
    out, cin = shape[0], shape[1]
    kk = shape[2] * shape[3] if len(shape) == 4 else 1
    fan = cin * kk
    rn = lambda *s: torch.randn(*s, generator=g)
    if kind == "plain":
        f = {"lora_down": rn(r, *shape[1:]) * fan ** -0.5, "lora_up": rn(out, r) * 0.1}
        fo, rank = [f["lora_down"], f["lora_up"]], r
    elif kind == "hada":
        f = {"hada_w1_a": rn(out, r) * 0.15, "hada_w1_b": rn(r, fan) * fan ** -0.25, "hada_w2_a": rn(out, r) * 0.15, "hada_w2_b": rn(r, fan) * fan ** -0.25}
        fo, rank = [f[n] for n in ("hada_w1_a", "hada_w1_b", "hada_w2_a", "hada_w2_b")], r
    else:
        a, b = 4, 8
        c, d = out // a, cin // b
        f = {"lokr_w1": rn(a, b) * 0.25, "lokr_w2_a": rn(c, r) * 0.3, "lokr_w2_b": rn(r, d * kk) * fan ** -0.5 * 2}
        fo, rank = [f["lokr_w1"], f["lokr_w2_a"].double() @ f["lokr_w2_b"].double()], r
    factor = alpha / rank
    m = None
    if dora:
        n = (W.double() + SCALE * factor * O.delta(kind, fo, shape)).pow(2).sum(tuple(range(1, len(shape)))).sqrt()
        m = (n * (0.8 + 0.4 * torch.rand(out, generator=g).double())).float()
    return LoraTerm(kind, f, alpha, m), {"kind": kind, "f": fo, "factor": factor, "m": m, "r": rank}


def make_adapters(ocfg, sd, dtype):
    """Adapters "a" and "b" over every Linear and conv target, kinds and magnitudes in rotation and shifted between the two, so that the
    layers of the two-adapter slot see every pairing; a third of a's Linear targets stay plain pairs in ``weights``."""
    shapes = ou.param_shapes(ocfg)
    targets = ou.lora_target_names(ocfg) + co.conv_targets(ocfg)
    kinds = ("plain", "hada", "kron")
    engine, oracle = {}, {}
    for ai, name in enumerate(("a", "b")):
        g = torch.Generator().manual_seed(500 + ai)
        weights, terms, oterms = {}, {}, {}
        for i, key in enumerate(targets):
            shape = tuple(shapes[key + ".weight"])
            kind, dora = kinds[(i + ai) % 3], (i // 3 + ai) % 2 == 1
            W = sd[key + ".weight"]
            if kind == "plain" and not dora:
                t, o = make_term("plain", shape, g, 8, False, W, 8.0)
                weights[key] = (t.factors["lora_down"], t.factors["lora_up"])
            else:
                t, o = make_term(kind, shape, g, 4 if kind != "plain" else 8, dora, W, 2.0)
                terms[key] = t
            oterms[key] = o
        engine[name] = LoraAdapter(name, weights, terms=terms)
        oracle[name] = oterms
    return engine, oracle


def oracle_terms(oracle, key, combo):
    return [dict(oracle[n][key], scale=SCALE * w) for n, w in combo if key in oracle[n]]


@pytest.fixture(scope="module")
def case(dev):
    out = {}

    def get(dtype):
        if dtype not in out:
            cfg, ocfg = UNetConfig.tiny(), ou.UNetConfig.tiny()
            sd = ou.init_state_dict(ocfg, seed=0, dtype=dtype)
            unet = UNet2DConditionModel(cfg, dtype=dtype, device=dev)
            unet.load_state_dict({k: v.to(dtype) for k, v in sd.items()})
            engine, oracle = make_adapters(ocfg, sd, dtype)
            keys = sorted(set(oracle["a"]) | set(oracle["b"]))
            merged = []                                     # per slot: the state dict with every target merged in float64
            for combo in SLOTS:
                sdn = dict(sd)
                for key in keys:
                    sdn[key + ".weight"] = O.slot_weight(sd[key + ".weight"], oracle_terms(oracle, key, combo), packed=False)[0].float()
                merged.append(sdn)
            g = torch.Generator().manual_seed(3)
            L_ = cfg.sample_size
            x = torch.randn(4, 4, L_, L_, generator=g)
            ctx = torch.randn(4, 77, cfg.cross_attention_dim, generator=g).to(dtype).float()
            te = torch.randn(4, 64, generator=g).to(dtype).float()
            tid = torch.tensor([[L_ * 8.0, L_ * 8.0, 0, 0, L_ * 8.0, L_ * 8.0]] * 4)
            refs = [ou.unet_forward(sd if s == 0 else merged[s - 1], ocfg, x[b:b + 1], 981, ctx[b:b + 1], te[b:b + 1], tid[b:b + 1])
                    for b, s in enumerate([0, 1, 2, 1])]
            out[dtype] = dict(unet=unet, bank=LoraBank(unet, list(engine.values())), sd=sd, oracle=oracle, keys=keys, x=x, ctx=ctx, te=te, tid=tid,
                              ref=torch.cat(refs), engine=engine)
        return out[dtype]

    return get


def run_unet(c, dev, dtype, rows=slice(None), state=None):
    unet = c["unet"]
    unet.set_lora_state(state)
    try:
        return unet(c["x"][rows].to(dev), 981, encoder_hidden_states=c["ctx"][rows].to(dev).to(dtype),
                    added_cond_kwargs={"text_embeds": c["te"][rows].to(dev).to(dtype), "time_ids": c["tid"][rows].to(dev)})[0].float().cpu()
    finally:
        unet.set_lora_state(None)


@pytest.mark.parametrize("dtype", DTYPES)
def test_unet_with_mixed_adapters_matches_the_float64_merge(dev, dtype, case):
    c = case(dtype)
    bank = c["bank"]
    bank.build(SLOTS, scale=SCALE, mode="merged")
    try:
        # ---- every layer's slots against the derived bound (the gains come from the norm kernel: its own bound joins, gain_slack)
        worst = 0.0
        kinds = set()
        for key in c["keys"]:
            mod = c["unet"].get_submodule(key)
            W = c["sd"][key + ".weight"]
            assert torch.equal(mod.w_slots[0], ops.pack_conv_weight(mod.weight.data) if isinstance(mod, Conv2d) else mod.weight.data)
            for s, combo in enumerate(SLOTS):
                terms = oracle_terms(c["oracle"], key, combo)
                kinds.add(tuple(sorted((t["kind"], t["m"] is not None) for t in terms)))
                exact, S, r = O.slot_weight(W, terms)
                got = mod.w_slots[1 + s].double().cpu()
                ratio = ((got - exact).abs() / (O.bound(got, exact, S, r, dtype) + O.gain_slack(W, terms)[:, None] * S)).max().item()
                worst = max(worst, ratio)
                assert ratio <= 1.0, f"{key} slot {s}: |error| / bound = {ratio:.3f}"
        assert len(kinds) >= 8, kinds                       # single terms of every kind, with and without magnitude, and mixed pairs
        # ---- the forward
        slots = [0, 1, 2, 1]
        mk = lambda s: LoraState(torch.tensor(s, dtype=torch.int32, device=dev), len(s), merged=True)
        got = run_unet(c, dev, dtype, state=mk(slots))
        err = (got - c["ref"]).abs().max().item()
        print(f"unet lycoris {dtype}: max|d| = {err:.3e}; slots: largest |error| / bound = {worst:.3f}")
        assert err < UNET_TOL[dtype]
        plain = run_unet(c, dev, dtype)
        assert torch.equal(got[0], plain[0]) and (got[1] - plain[1]).abs().max() > 1e-3 and (got[2] - got[1]).abs().max() > 1e-3
        # ---- batched equals single, bitwise
        for b in range(4):
            one = run_unet(c, dev, dtype, rows=slice(b, b + 1), state=mk(slots[b:b + 1]))
            assert torch.equal(one[0], got[b]), f"sample {b}"
        # ---- the un-merged stacks carry plain pairs only, and none is of zero width
        for m in c["unet"].modules():
            if getattr(m, "lora_down", None) is not None:
                assert m.lora_down.shape[1] == 16 and m.lora_up.shape[2] == 16
    finally:
        bank.clear()


@pytest.mark.parametrize("dtype", DTYPES)
def test_kernel_and_torch_merge_of_plain_adapters_agree_within_the_bound(dev, dtype, case):
    """``merge="auto"`` on plain adapters is ``merge="torch"`` bit for bit; ``merge="hip"`` gives slots within the bound of the same float64
    merge that the torch expression is within."""
    c = case(dtype)
    ocfg = ou.UNetConfig.tiny()
    lin, _ = ou.make_lora(ocfg, ou.lora_target_names(ocfg), 8, 100, SCALE, dtype)
    conv = co.make_conv_lora(ocfg, co.conv_targets(ocfg), 5, 150, dtype)
    lin2, _ = ou.make_lora(ocfg, ou.lora_target_names(ocfg)[::2], 4, 101, SCALE, dtype)
    ads = [LoraAdapter("p", {k: (a.to(dev), b.to(dev)) for k, (a, b) in {**lin, **conv}.items()}), LoraAdapter("q", dict(lin2))]
    bank = LoraBank(c["unet"], ads)
    slots = [(("p", 1.0),), (("p", 0.7), ("q", 0.5))]
    try:
        stacks = {}
        for merge in ("torch", "auto", "hip"):
            bank.build(slots, scale=SCALE, mode="merged", merge=merge)
            stacks[merge] = {k: c["unet"].get_submodule(k).w_slots.clone() for k in ads[0].weights}
        worst = {"torch": 0.0, "hip": 0.0}
        for key, w_t in stacks["torch"].items():
            assert torch.equal(stacks["auto"][key], w_t), key
            W = c["sd"][key + ".weight"]
            for s, combo in enumerate(slots):
                terms = [{"kind": "plain", "f": list(ad.weights[key]), "scale": SCALE * w, "factor": 1.0, "m": None, "r": ad.weights[key][0].shape[0]}
                         for ad, w in ((bank.adapters[n], w) for n, w in combo) if key in ad.weights]
                terms = [dict(t, f=[x.cpu() for x in t["f"]]) for t in terms]
                exact, S, r = O.slot_weight(W, terms)
                for merge in ("torch", "hip"):
                    ok, ratio = O.held(stacks[merge][key][1 + s], exact, S, r)
                    worst[merge] = max(worst[merge], ratio)
                    assert ok, f"{merge} {key} slot {s}: {ratio:.3f}"
        print(f"plain adapters {dtype}: largest |error| / bound torch {worst['torch']:.3f}, kernel {worst['hip']:.3f}")
    finally:
        bank.clear()


def test_more_than_four_terms_in_a_slot_are_refused_by_name(dev, case):
    c = case(torch.float16)
    key = "down_blocks.1.attentions.0.transformer_blocks.0.attn1.to_q"
    g = torch.Generator().manual_seed(1)
    ads = [LoraAdapter(f"h{i}", {}, terms={key: make_term("hada", (128, 128), g, 2, False, None, 2.0)[0]}) for i in range(5)]
    bank = LoraBank(c["unet"], ads)
    try:
        bank.build([tuple((a.name, 1.0) for a in ads[:4])])
        assert c["unet"].get_submodule(key).w_slots is not None and c["unet"].get_submodule(key).lora_down is None        # rank 0: no zero-width stack
        with pytest.raises(L.OmgHipError, match=r"down_blocks\.1.*slot 0: 5 adapter terms, at most 4"):
            bank.build([tuple((a.name, 1.0) for a in ads)])
    finally:
        bank.clear()


# ------------------------------------------------------------------ the text encoder
@pytest.mark.parametrize("dtype", DTYPES)
def test_text_encoder_loha_entry_equals_the_full_rank_pair(dev, dtype):
    """A LoHa (and a LoKr) entry on the text encoder gives the packed weights of the same delta handed over as the plain pair (delta, I):
    ``W + mult * delta`` with delta formed in fp32, one rounding."""
    from omg_amd.text_encoder import ClipTextConfig, ClipTextEncoder
    cfg = ClipTextConfig(vocab_size=300, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, hidden_act="quick_gelu",
                         projection_dim=64, eos_token_id=299, with_projection=False)
    enc = ClipTextEncoder(cfg, dtype=dtype, device=dev)
    g = torch.Generator().manual_seed(2)
    with torch.no_grad():
        for p in enc.parameters():
            p.copy_((torch.randn(p.shape, generator=g) * 0.05).to(dtype))
    q, fc1 = "text_model.encoder.layers.0.self_attn.q_proj", "text_model.encoder.layers.1.mlp.fc1"
    rn = lambda *s: torch.randn(*s, generator=g) * 0.3
    sd = {"lora_te1_text_model_encoder_layers_0_self_attn_q_proj." + n: rn(*s) for n, s in
          (("hada_w1_a", (128, 4)), ("hada_w1_b", (4, 128)), ("hada_w2_a", (128, 4)), ("hada_w2_b", (4, 128)))}
    sd.update({"lora_te1_text_model_encoder_layers_1_mlp_fc1." + n: rn(*s) for n, s in (("lokr_w1", (4, 8)), ("lokr_w2_a", (64, 2)), ("lokr_w2_b", (2, 16)))})
    sd["lora_te1_text_model_encoder_layers_0_self_attn_q_proj.alpha"] = torch.tensor(2.0)
    sd["lora_unet_down_blocks_1_attentions_0_transformer_blocks_0_attn1_to_q.lora_down.weight"] = rn(4, 128)
    sd["lora_unet_down_blocks_1_attentions_0_transformer_blocks_0_attn1_to_q.lora_up.weight"] = rn(128, 4)
    ad = loaders.load_lora_adapter(UNet2DConditionModel(UNetConfig.tiny(), device="meta"), sd, "x")
    te = ad.text_encoder[1]
    assert isinstance(te[q], LoraTerm) and te[q].factor == 0.5 and te[fc1].factor == 1.0
    pairs = {k: (torch.eye(t.dense().shape[1]), t.dense() * t.factor) for k, t in te.items()}
    ids = torch.randint(0, 298, (2, 77), generator=g)
    ids[:, -1] = 299
    ids = ids.to(dev)
    base = enc(ids)[0].clone()
    enc.set_lora([(te, 0.7)])
    enc.forward(ids)
    got_w = [enc._packed["layers"][0]["wqkv"].clone(), enc._packed["layers"][1]["w1"].clone()]
    got = enc(ids)[0].clone()
    enc.set_lora([(pairs, 0.7)])
    want = enc(ids)[0].clone()
    want_w = [enc._packed["layers"][0]["wqkv"], enc._packed["layers"][1]["w1"]]
    enc.set_lora(None)
    for a, b in zip(got_w, want_w):
        assert (a.float() - b.float()).abs().max() <= 2 * float(torch.finfo(dtype).eps) * b.float().abs().max()        # (0.7 * 0.5) * d vs 0.7 * (0.5 * d): an fp32 rounding apart
    assert (got.float() - want.float()).abs().max() <= 1e-2 * want.float().abs().max()
    assert (got.float() - base.float()).abs().max() > 10 * (got.float() - want.float()).abs().max()
    # the merged weight is W + mult * factor * delta with delta from the float64 oracle, to one 16-bit rounding
    wq = enc.text_model.encoder.layers[0].self_attn.q_proj.weight.data.double().cpu()
    f = [sd["lora_te1_text_model_encoder_layers_0_self_attn_q_proj." + n] for n in ("hada_w1_a", "hada_w1_b", "hada_w2_a", "hada_w2_b")]
    exact = wq + 0.7 * 0.5 * O.delta("hada", f, (128, 128))
    gq = got_w[0][:128].double().cpu()
    assert bool(((gq - exact).abs() <= 0.5 * O.ulp16(torch.maximum(gq.abs(), exact.abs()), dtype) + 1e-5 * exact.abs().max()).all())


# ------------------------------------------------------------------ the script surface
def test_compat_load_lora_weights_accepts_a_loha_file(dev, tmp_path):
    from safetensors.torch import save_file
    from omg_amd import compat
    from tests import _fake_hub as hub
    model = hub.write_sdxl_dir(str(tmp_path / "sdxl"))
    compat.clear_component_cache()
    try:
        pipe = compat.StableDiffusionXLPipeline.from_pretrained(model, torch_dtype=torch.float16, variant="fp16").to(dev)
        unet = pipe._comp.unet
        g = torch.Generator().manual_seed(0)
        sd, want = {}, {}
        convs = loaders.conv_module_paths(unet)
        lin = [n for n in loaders.linear_module_paths(unet) if n.endswith(("attn1.to_q", "attn2.to_v", "ff.net.2"))][:6]
        for mod in lin + list(convs)[:3]:
            m = unet.get_submodule(mod)
            out, fan = (m.out_features, m.in_features) if mod in lin else (m.cout, m.cin * m.ksize * m.ksize)
            flat = "lora_unet_" + mod.replace(".", "_")
            for n, shp in (("hada_w1_a", (out, 4)), ("hada_w1_b", (4, fan)), ("hada_w2_a", (out, 4)), ("hada_w2_b", (4, fan))):
                sd[f"{flat}.{n}"] = torch.randn(*shp, generator=g) * 0.2
            sd[f"{flat}.alpha"] = torch.tensor(2.0)
            want[mod] = sd[f"{flat}.hada_w1_a"]
        path = str(tmp_path / "loha" / "loha-concept.safetensors")
        os.makedirs(os.path.dirname(path))
        save_file(sd, path)
        pipe.load_lora_weights(path, weight_name="pytorch_lora_weights.safetensors", adapter_name="loha-concept")
        bank = pipe.bank
        ad = bank.adapters["loha-concept"]
        assert set(ad.terms) == set(want) and not ad.weights and ad.rank == 0
        assert all(t.kind == "hada" and t.factor == 0.5 and torch.equal(t.factors["hada_w1_a"], want[m]) for m, t in ad.terms.items())
        bank.build([(("loha-concept", 1.0),)], scale=0.8)
        for mod in want:
            ws = unet.get_submodule(mod).w_slots
            assert ws is not None and ws.shape[0] == 2 and not torch.equal(ws[0], ws[1]), mod
        bank.clear()
    finally:
        compat.clear_component_cache()
