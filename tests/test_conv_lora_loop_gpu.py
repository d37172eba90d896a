"""Loop parity with conv LoRA (-m gpu): the 8-step two-stage call of tests/test_pipeline_gpu.py's kind with two concept adapters that
target Linear AND conv layers, against oracle/pipeline.denoise whose concept UNets close over state dicts with the conv halves merged in
fp32 (tests/_conv_lora_oracle.py); hipGraph == eager; an adapter whose conv B is zero == the adapter without conv entries."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from omg_amd import controller as pc
from omg_amd.lora import LoraAdapter, LoraBank
from omg_amd.pipeline import ConceptModels, LoraMultiConceptPipeline, revise_regionally_controlnet_forward
from omg_amd.schedulers import make_scheduler
from oracle import controller as oc
from oracle import pipeline as opipe
from oracle import schedulers as osched
from oracle import unet as ou
from omg_amd.unet import UNet2DConditionModel, UNetConfig
from tests import _conv_lora_oracle as co

conv_targets, make_conv_lora = co.conv_targets, co.make_conv_lora
P = "a man and a woman walking on the street"


def embeds(cfg, n, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    e = torch.randn(n, 77, cfg.cross_attention_dim, generator=g).to(dtype).float()
    p = torch.randn(n, cfg.projection_class_embeddings_input_dim - 6 * cfg.addition_time_embed_dim, generator=g).to(dtype).float()
    return e, p


def build_unet(dev, dtype, seed=0):
    cfg, ocfg = UNetConfig.tiny(), ou.UNetConfig.tiny()
    sd = ou.init_state_dict(ocfg, seed=seed, dtype=dtype)
    unet = UNet2DConditionModel(cfg, dtype=dtype, device=dev)
    unet.load_state_dict({k: v.to(dtype) for k, v in sd.items()})
    return cfg, ocfg, sd, unet

S, GS, FSTART = 8, 7.5, 3


def make_inputs(cfg, dtype, lh=16, lw=16):
    H, W = lh * 8, lw * 8
    neg_e, neg_p = embeds(cfg, 1, 1, dtype)
    pos_e, pos_p = embeds(cfg, 1, 2, dtype)
    regions = []
    for c in range(2):
        re_, rp_ = embeds(cfg, 2, 10 + c, dtype)
        regions.append((re_[0:1], re_[1:2], rp_[0:1], rp_[1:2]))
    m1 = torch.zeros(H, W); m1[H // 4:, W // 16: W // 2 - 8] = 1
    m2 = torch.zeros(H, W); m2[H // 4:, W // 2 - 24: W - 8] = 1
    return dict(H=H, W=W, pe=pos_e.repeat(2, 1, 1), ne=neg_e.repeat(2, 1, 1), pp=pos_p.repeat(2, 1), npp=neg_p.repeat(2, 1), regions=regions,
                masks=[m1, m2], lat0=torch.randn(1, 4, lh, lw, generator=torch.Generator().manual_seed(14)),
                tid=torch.tensor([[H, W, 0, 0, H, W]], dtype=torch.float32))


def call(pipe, inp, pctl, concept, stage, **kw):
    pctl.reset()
    return pipe(output_type="latent", prompt_embeds=inp["pe"], negative_prompt_embeds=inp["ne"], pooled_prompt_embeds=inp["pp"],
                negative_pooled_prompt_embeds=inp["npp"], height=inp["H"], width=inp["W"], num_inference_steps=S, guidance_scale=GS,
                latents=inp["lat0"], cross_attention_kwargs={"scale": 0.8}, controller=pctl, concept_models=concept, stage=stage,
                region_masks=inp["masks"], lora_list=["c0", "c1"], styleL=False, region_prompt_embeds=inp["regions"], fusion_start=FSTART, **kw).images


@pytest.fixture(scope="module")
def loop(dev):
    dtype = torch.float16
    cfg, ocfg, sd, unet = build_unet(dev, dtype)
    lin, fns, conv = [], [], []
    for c in range(2):
        w, fn = ou.make_lora(ocfg, ou.lora_target_names(ocfg), rank=8, seed=100 + c, scale=0.8, dtype=dtype)
        lin.append(w); fns.append(fn)
        conv.append(make_conv_lora(ocfg, conv_targets(ocfg), 8, 150 + c, dtype))
    todev = lambda w: {k: (a.to(dev), b.to(dev)) for k, (a, b) in w.items()}
    pctl = pc.AttentionReplace([P, P], S, {"default_": 1.0}, 0.4, 4, 4, device=dev)
    revise_regionally_controlnet_forward(unet, pctl)
    pipe = LoraMultiConceptPipeline(unet, make_scheduler("ddim"))
    return dict(cfg=cfg, ocfg=ocfg, sd=sd, unet=unet, lin=lin, fns=fns, conv=conv, todev=todev, pctl=pctl, pipe=pipe, inp=make_inputs(cfg, dtype), dtype=dtype, ref={})


def oracle_run(lp, stage):
    if stage in lp["ref"]:
        return lp["ref"][stage]
    inp, ocfg, sd = lp["inp"], lp["ocfg"], lp["sd"]
    osch = osched.make("ddim", S)
    octl = oc.AttentionReplaceOracle([P, P], S, {"default_": 1.0}, 0.4, 4, 4)
    octl.num_att_layers = lp["pctl"].num_att_layers
    attn = oc.reference_attn_fn(octl)
    ctx4 = torch.cat([inp["ne"], inp["pe"]]); te4 = torch.cat([inp["npp"], inp["pp"]])
    tid = inp["tid"]

    def main(x, i):
        return ou.unet_forward(sd, ocfg, x, float(osch.timesteps[i]), ctx4, te4, tid.repeat(4, 1), attn_fn=attn)

    def conc(c):
        r = inp["regions"][c]
        ctx2 = torch.cat([r[0], r[1]]); te2 = torch.cat([r[2], r[3]])
        sdc = co.merged_state_dict(sd, lp["conv"][c], 0.8)             # the conv half merged in fp32; the Linear half through lora=
        return lambda x, i: ou.unet_forward(sdc, ocfg, x, float(osch.timesteps[i]), ctx2, te2, tid.repeat(2, 1), lora=lp["fns"][c])

    rec = []
    out = opipe.denoise(main, [conc(c) for c in range(2)], osch, inp["lat0"] * osch.init_noise_sigma, S, GS, stage, masks=inp["masks"],
                        fusion_start=FSTART, record=rec)
    lp["ref"][stage] = (out, rec)
    return out, rec


@pytest.mark.parametrize("lora_mode", ["merged", "segment"])
def test_two_stage_loop_with_conv_adapters_matches_oracle(dev, loop, lora_mode):
    lp = loop
    bank = LoraBank(lp["unet"], [LoraAdapter(f"c{c}", lp["todev"]({**lp["lin"][c], **lp["conv"][c]})) for c in range(2)])
    concept = ConceptModels(lp["unet"], bank)
    try:
        for stage in (1, 2):
            traj = []
            call(lp["pipe"], lp["inp"], lp["pctl"], concept, stage, trajectory=traj, lora_mode=lora_mode)
            ref, rec = oracle_run(lp, stage)
            errs = [(a.float().cpu() - b).abs().max().item() for a, b in zip(traj, rec)]
            print(f"conv lora {lora_mode} stage {stage}: per-step max|d| = " + " ".join(f"{e:.2e}" for e in errs))
            rel = errs[-1] / ref.pow(2).mean().sqrt().item()
            assert rel < 2e-2, (rel, errs)                             # the loop tolerance of tests/test_pipeline_gpu.py
    finally:
        bank.clear()


def test_graph_replay_with_conv_slots_is_bitwise_eager(dev, loop):
    lp = loop
    bank = LoraBank(lp["unet"], [LoraAdapter(f"c{c}", lp["todev"]({**lp["lin"][c], **lp["conv"][c]})) for c in range(2)])
    concept = ConceptModels(lp["unet"], bank)
    try:
        for mode in ("merged",):                                       # the engine captures graphs in merged mode only (segment mode is refused)
            runs = []
            for use_graph in (False, True, True):                      # capture, then pure replay
                traj = []
                call(lp["pipe"], lp["inp"], lp["pctl"], concept, 2, trajectory=traj, lora_mode=mode, use_graph=use_graph)
                runs.append([t.cpu() for t in traj])
            for other in runs[1:]:
                for i, (x, y) in enumerate(zip(runs[0], other)):
                    assert torch.equal(x, y), f"{mode} step {i}: graph replay differs from eager by {(x - y).abs().max().item()}"
    finally:
        bank.clear()


def test_zero_conv_up_matrix_equals_the_adapter_without_conv_entries(dev, loop):
    """Merged mode: W + s * 0 . A rounds to W, so the conv slots hold the base weight and the latents are bitwise those of the Linear-only adapter."""
    lp = loop
    outs = []
    for with_conv in (True, False):
        ws = []
        for c in range(2):
            w = dict(lp["lin"][c])
            if with_conv:
                w.update({k: (a, torch.zeros_like(b)) for k, (a, b) in lp["conv"][c].items()})
            ws.append(w)
        bank = LoraBank(lp["unet"], [LoraAdapter(f"c{c}", lp["todev"](ws[c])) for c in range(2)])
        try:
            outs.append(call(lp["pipe"], lp["inp"], lp["pctl"], ConceptModels(lp["unet"], bank), 2, lora_mode="merged").float().cpu())
        finally:
            bank.clear()
    assert torch.equal(outs[0], outs[1])
