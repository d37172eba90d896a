"""Conv LoRA through the callers' surfaces (-m gpu):
  * the script path: ``omg_amd.compat``'s ``load_lora_weights`` on fake hub files with conv entries (tests/_fake_hub_conv.py: kohya / SGM
    names for the concepts, PEFT keys for the style adapter, loaded into the main AND the concept pipe as inference_lora.py does), then a
    short stage-2 call with ``styleL=True``;
  * one InstantID call whose default-active style adapter carries conv entries — main rows at scale 0.8, concept rows at 1.0 — against
    the oracle's literal loop on state dicts with the conv half merged in fp32 (tests/_conv_lora_oracle.py)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from omg_amd import controller as pc
from omg_amd.controlnet import ControlNetModel
from omg_amd.ip_adapter import IPAdapter
from omg_amd.lora import LoraAdapter, LoraBank
from omg_amd.pipeline import ConceptModels, LoraMultiConceptPipeline, revise_regionally_controlnet_forward
from omg_amd.schedulers import make_scheduler
from omg_amd.unet import UNet2DConditionModel, UNetConfig
from oracle import controller as oc
from oracle import controlnet as ocn
from oracle import ip_adapter as oip
from oracle import pipeline as opipe
from oracle import schedulers as osched
from oracle import unet as ou
from tests import _conv_lora_oracle as co
from tests import _fake_hub as hub
from tests import _fake_hub_conv as hubc

P = "a man and a woman walking on the street"
dtype = torch.float16


# ------------------------------------------------------------------ the transcribed script path
@pytest.fixture(scope="module")
def hub_dirs(tmp_path_factory):
    from omg_amd import compat
    root = tmp_path_factory.mktemp("hub_conv")
    model, cn = hub.write_sdxl_dir(str(root / "sdxl")), hub.write_controlnet_dir(str(root / "controlnet"))
    compat.clear_component_cache()
    comp = compat._components(model, torch.float16, "fp16")
    tes = [comp.text_encoder, comp.text_encoder_2]
    out = {}
    for kind, write in (("conv", lambda *a, **k: hubc.write_conv_lora_file(*a, **k)[0]), ("plain", hub.write_lora_file)):
        loras = [write(str(root / kind / "loras" / f"{n}.safetensors"), comp.unet, 20 + i, text_encoders=tes)
                 for i, n in enumerate(("chris-evans", "TaylorSwiftSDXL"))]
        style = os.path.dirname(write(str(root / kind / "style" / "pytorch_lora_weights.safetensors"), comp.unet, 30, style="peft", text_encoders=tes))
        out[kind] = ("|".join(loras), style)
    written = hubc.write_conv_lora_file(str(root / "probe" / "probe.safetensors"), comp.unet, 20, text_encoders=tes)[1]
    compat.clear_component_cache()
    return model, cn, out, written


def run_script(dev, model, cn, lora_paths, style, S=18):
    """What inference_lora.py does with its pipes (:152-171, :37-73), on the compat objects: two pipes over one directory, the style LoRA
    loaded into both, every concept LoRA into the concept pipe, then the stage-2 call."""
    from omg_amd import compat
    compat.clear_component_cache()
    width = height = 128
    prompts = [P] * 2
    controlnet = compat.ControlNetModel.from_pretrained(cn, torch_dtype=torch.float16).to(dev)
    pipe = compat.LoraMultiConceptPipeline.from_pretrained(model, controlnet=controlnet, torch_dtype=torch.float16, variant="fp16").to(dev)
    controller = pc.AttentionReplace(prompts, 50, cross_replace_steps={"default_": 1.}, self_replace_steps=0.4, tokenizer=pipe.tokenizer, device=dev,
                                     dtype=torch.float16, width=width // 32, height=height // 32)
    revise_regionally_controlnet_forward(pipe.unet, controller)
    pipe_concept = compat.StableDiffusionXLPipeline.from_pretrained(model, torch_dtype=torch.float16, variant="fp16").to(dev)
    pipe.load_lora_weights(style, weight_name="pytorch_lora_weights.safetensors", adapter_name="style")
    pipe_concept.load_lora_weights(style, weight_name="pytorch_lora_weights.safetensors", adapter_name="style")
    names = []
    for path in lora_paths.split("|"):
        name = path.split("/")[-1].split(".")[0]
        pipe_concept.load_lora_weights(path, weight_name="pytorch_lora_weights.safetensors", adapter_name=name)
        names.append(name)
    mask1 = torch.zeros(height, width, dtype=torch.bool); mask1[32:, 8:60] = True
    mask2 = torch.zeros(height, width, dtype=torch.bool); mask2[32:, 56:120] = True
    region = [("a man in the park", "painting"), ("a woman in the park", "painting")]
    images = pipe(prompt=[prompts, region], concept_models=pipe_concept, negative_prompt=["painting"] * 2, generator=torch.Generator(dev).manual_seed(7),
                  guidance_scale=7.5, num_inference_steps=S, cross_attention_kwargs={"scale": 0.8}, controller=controller, stage=2,
                  region_masks=[mask1, mask2], lora_list=names, styleL=True, image=None, height=height, width=width).images
    return pipe_concept, names, [np.array(im).astype(int) for im in images]


def test_script_path_loads_files_with_conv_entries_and_runs_stage_2(dev, hub_dirs):
    model, cn, files, written = hub_dirs
    concept, names, img_conv = run_script(dev, model, cn, *files["conv"])
    bank = concept.bank
    assert set(bank.adapters) == {"style", *names}
    ad = bank.adapters[names[0]]
    assert set(written) <= set(ad.weights) and len(written) == 49                 # every conv entry of the file arrived, under its diffusers path
    for mod, (a, b) in written.items():
        assert torch.equal(ad.weights[mod][0], a) and torch.equal(ad.weights[mod][1], b), mod
    assert any(a.dim() == 4 for a, _ in bank.adapters["style"].weights.values())   # the PEFT-keyed style file too
    carried = [m for m in concept._comp.unet.modules() if getattr(m, "w_slots", None) is not None and hasattr(m, "ksize")]
    assert len(carried) == 49                                                      # the stage-2 call built and used the conv slot stacks
    assert len(img_conv) == 2 and img_conv[0].shape == (128, 128, 3)
    _, _, img_plain = run_script(dev, model, cn, *files["plain"])                   # the same files without their conv entries
    assert np.abs(img_conv[1] - img_plain[1]).max() > 3, "the conv entries of the concept adapters must show in the edited sample"
    assert np.abs(img_conv[0] - img_plain[0]).max() > 3, "the conv entries of the style adapter must show on the main pass"


# ------------------------------------------------------------------ InstantID
def emb(cfg, n, seed, tokens=77):
    g = torch.Generator().manual_seed(seed)
    e = torch.randn(n, tokens, cfg.cross_attention_dim, generator=g).to(dtype).float()
    p = torch.randn(n, cfg.projection_class_embeddings_input_dim - 6 * cfg.addition_time_embed_dim, generator=g).to(dtype).float()
    return e, p


@pytest.mark.parametrize("use_graph", [False, True])
def test_instantid_call_with_conv_entries_in_the_style_adapter(dev, use_graph):
    """The call of tests/test_instantid_gpu.py (style = True) with a style adapter on Linear AND conv targets: the adapter reaches the convs
    through the main pass's slot (scale 0.8) and the concept rows' slot (scale 1.0); the IdentityNet never receives a LoRA state."""
    cfg, ocfg = UNetConfig.tiny(), ou.UNetConfig.tiny()
    sd = ou.init_state_dict(ocfg, seed=0, dtype=dtype)
    unet = UNet2DConditionModel(cfg, dtype=dtype, device=dev)
    unet.load_state_dict({k: v.to(dtype) for k, v in sd.items()})
    csd = ocn.init_state_dict(ocfg, seed=5, dtype=dtype)
    idn = ControlNetModel(cfg, dtype=dtype, device=dev)
    idn.load_state_dict({k: v.to(dtype) for k, v in csd.items()})
    L = cfg.sample_size
    S, gs, fstart, ip_scale, idn_scale, ntok = 7, 3.0, 2, 0.8, 0.8, 16
    H = W = L * 8
    pos_e, pos_p = emb(cfg, 1, 2); neg_e, neg_p = emb(cfg, 1, 1)
    pe, ne, pp, npp = pos_e.repeat(2, 1, 1), neg_e.repeat(2, 1, 1), pos_p.repeat(2, 1), neg_p.repeat(2, 1)
    regions, faces = [], []
    g = torch.Generator().manual_seed(77)
    for c in range(2):
        re_, rp_ = emb(cfg, 2, 10 + c)
        regions.append((re_[0:1], re_[1:2], rp_[0:1], rp_[1:2]))
        idtok = torch.randn(1, ntok, cfg.cross_attention_dim, generator=g).to(dtype).float()
        faces.append(torch.cat([torch.randn(1, ntok, cfg.cross_attention_dim, generator=g).to(dtype).float() * 0.1, idtok], dim=0))
    m1 = torch.zeros(H, W); m1[H // 4:, W // 16: W // 2] = 1
    m2 = torch.zeros(H, W); m2[H // 4:, W // 2 - 16:] = 1
    kps = torch.rand(1, 3, H, W, generator=g).to(dtype).float()
    lat0 = torch.randn(1, 4, L, L, generator=torch.Generator().manual_seed(14))
    tid = torch.tensor([[H, W, 0, 0, H, W]], dtype=torch.float32)
    ipw = {}
    gi = torch.Generator().manual_seed(9)
    for name, shp in ou.param_shapes(ocfg).items():
        if name.endswith(".attn2.to_k.weight"):
            c_, cx = shp
            ipw[name[: -len(".to_k.weight")]] = ((torch.randn(c_, cx, generator=gi) * cx ** -0.5).to(dtype).float(),
                                                 (torch.randn(c_, cx, generator=gi) * cx ** -0.5).to(dtype).float())
    IPAdapter(unet, num_tokens=ntok, scale=ip_scale).load_named(ipw)
    args = ([P, P], S, {"default_": 1.0}, 0.4, L // 4, L // 4)
    pctl = pc.AttentionReplace(*args, device=dev)
    revise_regionally_controlnet_forward(unet, pctl)
    pipe = LoraMultiConceptPipeline(unet, make_scheduler("euler"))
    names = ou.lora_target_names(ocfg)
    w_lin, lora_main = ou.make_lora(ocfg, names, rank=8, seed=300, scale=0.8, dtype=dtype)
    _, lora_conc = ou.make_lora(ocfg, names, rank=8, seed=300, scale=1.0, dtype=dtype)
    w_conv = co.make_conv_lora(ocfg, co.conv_targets(ocfg), 8, 350, dtype)
    bank = LoraBank(unet, [LoraAdapter("style", {k: (a.to(dev), b.to(dev)) for k, (a, b) in {**w_lin, **w_conv}.items()})])
    concept = ConceptModels(unet, bank)
    req = dict(prompt_embeds=pe, negative_prompt_embeds=ne, pooled_prompt_embeds=pp, negative_pooled_prompt_embeds=npp,
               region_prompt_embeds=regions, region_masks=[m1, m2], latents=lat0, region_image_embeds=faces, kps_image=kps)
    kw = dict(height=H, width=W, num_inference_steps=S, guidance_scale=gs, controller=pctl, concept_models=concept, stage=2, lora_list=["id0", "id1"],
              styleL=False, fusion_start=fstart, identitynet=idn, identitynet_conditioning_scale=idn_scale, main_adapters=[("style", 1.0)],
              concept_adapters=[("style", 1.0)], concept_adapter_scale=1.0, cross_attention_kwargs={"scale": 0.8}, concept_lora=False)
    try:
        pctl.reset()
        traj = []
        pipe.generate_many([req], trajectory=traj, use_graph=use_graph, **kw)
        assert all(getattr(m, "lora_state", None) is None for m in idn.modules())
        # ---- the oracle twin: conv half merged in fp32 at the row's scale, Linear half through lora=
        sd_main, sd_conc = co.merged_state_dict(sd, w_conv, 0.8), co.merged_state_dict(sd, w_conv, 1.0)
        osch = osched.make("euler", S)
        octl = oc.AttentionReplaceOracle(*args)
        octl.num_att_layers = pctl.num_att_layers
        attn_main = oc.reference_attn_fn(octl)
        ip_fn = oip.make_ip_attn_fn(ipw, ip_scale, ntok)
        ctx4, te4 = torch.cat([ne, pe]), torch.cat([npp, pp])

        def main(x, i):
            return ou.unet_forward(sd_main, ocfg, x, float(osch.timesteps[i]), ctx4, te4, tid.repeat(4, 1), attn_fn=attn_main, lora=lora_main)

        def conc(c):
            ctx2 = torch.cat([regions[c][0], regions[c][1]]); te2 = torch.cat([regions[c][2], regions[c][3]])

            def f(x, i):
                t = float(osch.timesteps[i])
                down, mid = ocn.controlnet_forward(csd, ocfg, x, t, faces[c], kps.repeat(2, 1, 1, 1), idn_scale, te2, tid.repeat(2, 1))
                return ou.unet_forward(sd_conc, ocfg, x, t, torch.cat([ctx2, faces[c]], dim=1), te2, tid.repeat(2, 1), attn_fn=ip_fn,
                                       down_block_additional_residuals=down, mid_block_additional_residual=mid, lora=lora_conc)
            return f

        rec = []
        ref = opipe.denoise(main, [conc(0), conc(1)], osch, lat0 * osch.init_noise_sigma, S, gs, 2, masks=[m1, m2], fusion_start=fstart, record=rec)
        errs = [(a[0].float().cpu() - b).abs().max().item() for a, b in zip(traj, rec)]
        rel = errs[-1] / ref.pow(2).mean().sqrt().item()
        print(f"instantid conv style (graph={use_graph}): per-step max|d| = " + " ".join(f"{e:.2e}" for e in errs), f" rel {rel:.2e}")
        assert rel < 2e-2, errs                                  # the loop tolerance of tests/test_instantid_gpu.py
        # the conv half must matter: the Linear-only oracle lands elsewhere
        octl.reset()
        lin_only = opipe.denoise(lambda x, i: ou.unet_forward(sd, ocfg, x, float(osch.timesteps[i]), ctx4, te4, tid.repeat(4, 1), attn_fn=attn_main, lora=lora_main),
                                 [conc(0), conc(1)], osch, lat0 * osch.init_noise_sigma, S, gs, 2, masks=[m1, m2], fusion_start=fstart)
        assert (lin_only - ref).abs().max() > 10 * errs[-1]
    finally:
        bank.clear()
