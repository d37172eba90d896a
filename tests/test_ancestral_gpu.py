"""Stochastic steps on the GPU (-m gpu): the noise step kernel (omg_fuse_cfg_step_noise) against a float64 recomputation, against
omg_fuse_cfg_step when the noise coefficient is 0, and through a captured hipGraph; the denoising loop with Euler-ancestral and with DDIM
eta = 1 against oracle.pipeline.denoise driven by the literal restatements in tests/_ancestral_oracle.py (LoRA flow and InstantID flow), the
noise drawn by the oracle side from a fresh generator of the same seed; and the engine's bitwise invariances under noise (graph == eager,
batched == single, dedup, StageCache resume with and without drop_unc0, seeds, switching eta on one pipe, concept_shard refused)."""
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

from omg_amd import _lib as L
from omg_amd import controller as pc
from omg_amd import ops
from omg_amd.lora import LoraAdapter, LoraBank
from omg_amd.parallel import ConceptShard
from omg_amd.pipeline import ConceptModels, LoraMultiConceptPipeline, StageCache, revise_regionally_controlnet_forward
from omg_amd.schedulers import DDIMScheduler, EulerAncestralDiscreteScheduler, make_scheduler
from omg_amd.unet import UNetConfig
from oracle import controller as oc
from oracle import pipeline as opipe
from oracle import schedulers as osched
from oracle import unet as ou
from tests import _ancestral_oracle as ao
from tests import test_instantid_gpu as tig
from tests import test_pipeline_gpu as tpg
from tests.test_dpm_gpu import C_, H_, W_, _mask_lr, kernel_inputs

GS = 7.5
P = tpg.P


def ref_step(noise, lat, row, z, fuse, regs, masks):
    """float64 restatement of one omg_fuse_cfg_step_noise launch: fusion, CFG, x' = cx x + ce eps + cz z"""
    unc0, unc1, cnd0, cnd1 = noise.clone()
    if fuse:
        any_ = torch.zeros(H_, W_, dtype=torch.bool)
        add_u, add_c = torch.zeros_like(unc1), torch.zeros_like(cnd1)
        for r, m in zip(regs, masks):
            if m is None:
                continue
            on = _mask_lr(m, H_, W_)
            any_ |= on
            if r is not None:
                add_u = add_u + on * r[0]
                add_c = add_c + on * r[1]
        unc1 = torch.where(any_, 0.0, unc1) + add_u
        cnd1 = torch.where(any_, 0.0, cnd1) + add_c
    e = torch.stack([unc0 + GS * (cnd0 - unc0), unc1 + GS * (cnd1 - unc1)])
    return row[0] * lat + row[1] * e + row[3] * z


def random_table(S, seed):
    """(S, 4) rows {cx, ce, cin_next, cz} with random values; the last row has cz = 0 (like the last ancestral step)"""
    g = torch.Generator().manual_seed(seed)
    tab = torch.stack([1 + 0.2 * torch.rand(S, generator=g), -torch.rand(S, generator=g), 0.5 + torch.rand(S, generator=g),
                       torch.rand(S, generator=g)], dim=1)
    tab[-1, 3] = 0.0
    return tab.float().contiguous()


def noise_buffer(S, dev, seed):
    """(S, 2, C, H, W) noise as a strided view of a wider (S, 4, C, H, W) buffer, like the engine's eng.z[:, 2j: 2j + 2]"""
    g = torch.Generator().manual_seed(seed)
    wide = torch.randn(S, 4, C_, H_, W_, generator=g).to(dev)
    return wide[:, 1:3]


def test_noise_step_kernel_matches_float64(dev):
    S = 6
    tab = random_table(S, 3).to(dev)
    rows = tab.double().cpu()
    z = noise_buffer(S, dev, 4)
    assert not z.is_contiguous() and z.stride(0) == 4 * C_ * H_ * W_
    zc = z.double().cpu()
    noise, regs, masks, lat0 = kernel_inputs(dev, S, seed=2)
    lat = lat0.to(dev)
    step_idx = torch.zeros(1, dtype=torch.int32, device=dev)
    dmasks = [m.to(dev) if m is not None else None for m in masks]
    ref = lat0.double()
    for i, dt in enumerate([torch.float16, torch.bfloat16, torch.float32] * 2):
        fuse = i % 2 == 1                                   # on and off
        mi = torch.empty(4, C_, H_, W_, dtype=dt, device=dev)
        ops.fuse_cfg_step_noise(noise[i].to(dev), lat, tab, z, step_idx, guidance_scale=GS, fuse=fuse,
                                region_preds=[r.to(dev) for r in regs[i]] if fuse else [None] * 3, masks=dmasks if fuse else [None] * 3,
                                model_input_next=mi)
        ref = ref_step(noise[i].double(), ref, rows[i], zc[i], fuse, [r.double() for r in regs[i]], masks)
        torch.cuda.synchronize()
        got = lat.double().cpu()
        err = (got - ref).abs().max() / ref.pow(2).mean().sqrt()
        assert err < 1e-5, (i, err.item())
        assert torch.equal(mi, (torch.cat([lat, lat]) * tab[i, 2]).to(dt)), f"step {i}: model input"
    assert step_idx.item() == S


def test_noise_step_with_zero_coefficient_equals_the_plain_step(dev):
    """cz = 0 in every row: bit for bit omg_fuse_cfg_step (latents, next model input, fused-noise tap), whatever z holds"""
    S = 5
    tab = random_table(S, 5)
    tab[:, 3] = 0.0
    tab = tab.to(dev)
    z = noise_buffer(S, dev, 6)
    noise, regs, masks, lat0 = kernel_inputs(dev, S, seed=7)
    dmasks = [m.to(dev) if m is not None else None for m in masks]
    la, lb = lat0.to(dev), lat0.to(dev)
    ia, ib = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    for i in range(S):
        fuse = i >= 2
        kw = dict(guidance_scale=GS, fuse=fuse, region_preds=[r.to(dev) for r in regs[i]] if fuse else [None] * 3,
                  masks=dmasks if fuse else [None] * 3)
        ma, mb = torch.empty(4, C_, H_, W_, dtype=torch.float16, device=dev), torch.empty(4, C_, H_, W_, dtype=torch.float16, device=dev)
        fa, fb = torch.empty(2, C_, H_, W_, device=dev), torch.empty(2, C_, H_, W_, device=dev)
        ops.fuse_cfg_step(noise[i].to(dev), la, tab, ia, model_input_next=ma, fused_noise_out=fa, **kw)
        ops.fuse_cfg_step_noise(noise[i].to(dev), lb, tab, z, ib, model_input_next=mb, fused_noise_out=fb, **kw)
        assert torch.equal(la, lb) and torch.equal(ma, mb), f"step {i}"
        if fuse:
            assert torch.equal(fa, fb)
    assert ia.item() == ib.item() == S


def test_noise_step_graph_replay_equals_eager(dev):
    S = 6
    tab = random_table(S, 8).to(dev)
    z = noise_buffer(S, dev, 9)
    noise, regs, masks, lat0 = kernel_inputs(dev, S, seed=10)
    noise = [x.to(dev) for x in noise]
    regs = [[r.to(dev) for r in rs] for rs in regs]
    dmasks = [m.to(dev) if m is not None else None for m in masks]
    lat = torch.empty(2, C_, H_, W_, device=dev)
    step_idx = torch.zeros(1, dtype=torch.int32, device=dev)
    mis = [torch.empty(4, C_, H_, W_, dtype=dt, device=dev) for dt in (torch.float16, torch.bfloat16, torch.float32) * 2]

    def reset():
        lat.copy_(lat0.to(dev)); step_idx.zero_()

    def body():
        for i in range(S):
            fuse = i >= 2
            ops.fuse_cfg_step_noise(noise[i], lat, tab, z, step_idx, guidance_scale=GS, fuse=fuse,
                                    region_preds=regs[i] if fuse else [None] * 3, masks=dmasks if fuse else [None] * 3, model_input_next=mis[i])

    reset()
    body()
    torch.cuda.synchronize()
    eager = (lat.clone(), [m.clone() for m in mis])
    reset()
    for m in mis:
        m.zero_()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        body()
    for _ in range(2):                                  # replay twice from the same start
        reset()
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(lat, eager[0]) and all(torch.equal(a, b) for a, b in zip(mis, eager[1]))
    z.mul_(2.0)                                         # the graph reads the noise buffer in place: new noise, new result
    reset()
    gr.replay()
    torch.cuda.synchronize()
    assert not torch.equal(lat, eager[0])


# ------------------------------------------------------------------------------------------------ the loop against the oracle
def _scheduler(kind):
    return (EulerAncestralDiscreteScheduler(), 0.0) if kind == "euler_a" else (DDIMScheduler(), 1.0)


def _oracle(kind, S, zs):
    return ao.EulerAncestral(S, zs) if kind == "euler_a" else ao.DDIMEta(S, 1.0, zs)


@pytest.mark.parametrize("kind", ["euler_a", "ddim_eta1"])
def test_two_stage_loop_matches_oracle_stochastic(dev, kind):
    """S = 8, fusion_start = 3, 3 concepts with LoRA (overlapping masks + a None mask), the p2p controller, generator=torch.Generator(dev):
    stage 1 and stage 2 against the oracle loop stepping the literal restatement with the same draws; rel < 2e-2 of the latent rms"""
    dtype = torch.float16
    cfg, ocfg, sd, unet = tpg.setup(dev, dtype)
    lh = lw = cfg.sample_size
    S, gs, fstart, seed = 8, 7.5, 3, 21
    H, W = lh * 8, lw * 8
    neg_e, neg_p = tpg.embeds(cfg, 1, 1, dtype)
    pos_e, pos_p = tpg.embeds(cfg, 1, 2, dtype)
    pe, ne, pp, npp = pos_e.repeat(2, 1, 1), neg_e.repeat(2, 1, 1), pos_p.repeat(2, 1), neg_p.repeat(2, 1)
    regions = []
    for c in range(3):
        re_, rp_ = tpg.embeds(cfg, 2, 10 + c, dtype)
        regions.append((re_[0:1], re_[1:2], rp_[0:1], rp_[1:2]))
    m1 = torch.zeros(H, W); m1[H // 4:, W // 16: W // 2 - 8] = 1
    m2 = torch.zeros(H, W); m2[H // 4:, W // 2 - 24: W - 8] = 1
    masks = [m1, None, m2]
    tid = torch.tensor([[H, W, 0, 0, H, W]], dtype=torch.float32)
    names = ou.lora_target_names(ocfg)
    ow, olora = [], []
    for c in range(3):
        w, fn = ou.make_lora(ocfg, names, rank=8, seed=100 + c, scale=0.8, dtype=dtype)
        ow.append(w); olora.append(fn)
    bank = LoraBank(unet, [LoraAdapter(f"c{c}", {k: (a.to(dev), b.to(dev)) for k, (a, b) in ow[c].items()}) for c in range(3)])
    concept = ConceptModels(unet, bank)
    args = ([P, P], S, {"default_": 1.0}, 0.4, lw // 4, lh // 4)
    pctl = pc.AttentionReplace(*args, device=dev)
    revise_regionally_controlnet_forward(unet, pctl)
    sch, eta = _scheduler(kind)
    pipe = LoraMultiConceptPipeline(unet, sch)
    lat0, zs = ao.draws(seed, dev, (1, 4, lh, lw), S)
    osch = _oracle(kind, S, zs)

    def oracle_run(stage):
        octl = oc.AttentionReplaceOracle(*args)
        octl.num_att_layers = pctl.num_att_layers
        attn = oc.reference_attn_fn(octl)
        ctx4 = torch.cat([ne, pe]); te4 = torch.cat([npp, pp])
        def main(x, i):
            return ou.unet_forward(sd, ocfg, x, float(osch.timesteps[i]), ctx4, te4, tid.repeat(4, 1), attn_fn=attn)
        def conc(c):
            ctx2 = torch.cat([regions[c][0], regions[c][1]]); te2 = torch.cat([regions[c][2], regions[c][3]])
            return lambda x, i: ou.unet_forward(sd, ocfg, x, float(osch.timesteps[i]), ctx2, te2, tid.repeat(2, 1), lora=olora[c])
        rec = []
        out = opipe.denoise(main, [conc(c) for c in range(3)], osch, lat0 * osch.init_noise_sigma, S, gs, stage,
                            masks=masks, fusion_start=fstart, record=rec)
        return out, rec

    for stage in (1, 2):
        pctl.reset()
        traj = []
        out = pipe(output_type="latent", prompt_embeds=pe, negative_prompt_embeds=ne, pooled_prompt_embeds=pp, negative_pooled_prompt_embeds=npp,
                   height=H, width=W, num_inference_steps=S, guidance_scale=gs, generator=torch.Generator(dev).manual_seed(seed), eta=eta,
                   cross_attention_kwargs={"scale": 0.8}, controller=pctl, concept_models=concept, stage=stage,
                   region_masks=masks, lora_list=["c0", "c1", "c2"], styleL=False, region_prompt_embeds=regions,
                   trajectory=traj, fusion_start=fstart).images
        ref, rec = oracle_run(stage)
        errs = [(a.float().cpu() - b).abs().max().item() for a, b in zip(traj, rec)]
        print(f"{kind} stage {stage}: per-step max|d| = " + " ".join(f"{e:.2e}" for e in errs), " latent rms", ref.pow(2).mean().sqrt().item())
        rel = errs[-1] / ref.pow(2).mean().sqrt().item()
        assert rel < 2e-2, (rel, errs)
        assert (pctl.cur_step, pctl.cur_att_layer) == (S, 0)
        if stage == 1:
            assert (out[0] - out[1]).abs().max() > 0.1, "stage 1: the two samples get different noise"
            stage1 = ref
        else:
            assert (ref[1] - stage1[1]).abs().max() > 0.1, "fusion must change the edited sample"
            assert torch.allclose(ref[0], stage1[0], atol=1e-5), "the base sample never depends on the edit"


def test_instantid_loop_matches_oracle_with_euler_ancestral(dev, monkeypatch):
    """the InstantID loop test with Euler-ancestral in place of Euler: its call passes latents=, so the request's generator (injected, seeded)
    draws the S noise tensors only, and the oracle draws them from a fresh generator of the same seed"""
    seed = 33
    L_ = UNetConfig.tiny().sample_size
    orig_many, orig_make = LoraMultiConceptPipeline.generate_many, osched.make

    def with_generator(self, requests, **kw):
        return orig_many(self, [dict(r, generator=torch.Generator(dev).manual_seed(seed)) for r in requests], **kw)

    def oracle_make(name, S):
        return ao.EulerAncestral(S, ao.draws(seed, dev, (1, 4, L_, L_), S, latents=False)[1]) if name == "euler" else orig_make(name, S)

    monkeypatch.setattr(LoraMultiConceptPipeline, "generate_many", with_generator)
    monkeypatch.setattr(tig, "make_scheduler", lambda name: EulerAncestralDiscreteScheduler() if name == "euler" else make_scheduler(name))
    monkeypatch.setattr(osched, "make", oracle_make)
    tig.test_instantid_loop_matches_oracle(dev, False, False)


# ------------------------------------------------------------------------------------------------ bitwise invariances of the engine
def _env(dev, S, fstart):
    dtype = torch.float16
    cfg, ocfg, sd, unet = tpg.setup(dev, dtype)
    L_ = cfg.sample_size
    H = W = L_ * 8
    names = ou.lora_target_names(ocfg)
    bank = LoraBank(unet, [LoraAdapter(nm, {k: (a.to(dev), b.to(dev)) for k, (a, b) in ou.make_lora(ocfg, names, 8, 100 + c, 0.8, dtype)[0].items()})
                           for c, nm in enumerate(["c0", "c1"])])
    concept = ConceptModels(unet, bank)
    pctl = pc.AttentionReplace([P, P], S, {"default_": 1.0}, 0.5, L_ // 4, L_ // 4, device=dev)
    revise_regionally_controlnet_forward(unet, pctl)
    m1 = torch.zeros(H, W); m1[H // 4:, : W // 2] = 1
    m2 = torch.zeros(H, W); m2[H // 4:, W // 2 - 16:] = 1

    def request(seed, gseed=None):
        """embeddings from ``seed``, a FRESH generator seeded ``gseed`` (default: seed) drawing the latents and the noise"""
        pe1, pp1 = tpg.embeds(cfg, 1, seed, dtype); ne1, np1 = tpg.embeds(cfg, 1, seed + 50, dtype)
        regions = []
        for c in range(2):
            re_, rp_ = tpg.embeds(cfg, 2, seed + 10 + c, dtype)
            regions.append((re_[0:1], re_[1:2], rp_[0:1], rp_[1:2]))
        return dict(prompt_embeds=pe1.repeat(2, 1, 1), negative_prompt_embeds=ne1.repeat(2, 1, 1), pooled_prompt_embeds=pp1.repeat(2, 1),
                    negative_pooled_prompt_embeds=np1.repeat(2, 1), region_prompt_embeds=regions, region_masks=[m1, m2],
                    generator=torch.Generator(dev).manual_seed(seed if gseed is None else gseed))

    kw = dict(height=H, width=W, num_inference_steps=S, guidance_scale=7.5, cross_attention_kwargs={"scale": 0.8}, controller=pctl,
              concept_models=concept, lora_list=["c0", "c1"], styleL=False, fusion_start=fstart)

    def run(pipe, reqs, stage, **extra):
        pctl.reset()
        traj = []
        out = pipe.generate_many(reqs, stage=stage, trajectory=traj, **kw, **extra)
        assert (pctl.cur_step, pctl.cur_att_layer) == (S, 0)
        return out.cpu(), torch.stack([t.cpu() for t in traj])

    return SimpleNamespace(unet=unet, request=request, run=run, kw=kw)


@pytest.mark.parametrize("kind", ["euler_a", "ddim_eta1"])
def test_stochastic_engine_invariances(dev, kind):
    """same seed twice == itself; graph (capture, replay) == eager; two requests in lock-step == the single calls; dedup=True == the
    full batch (it falls back: the samples differ from step 0); the two samples of a request differ in stage 1; another seed differs"""
    S, fstart = 8, 3
    env = _env(dev, S, fstart)
    sch, eta = _scheduler(kind)
    pipe = LoraMultiConceptPipeline(env.unet, sch)
    r = env.request
    full, traj = env.run(pipe, [r(1)], 2, eta=eta)
    assert torch.equal(env.run(pipe, [r(1)], 2, eta=eta)[1], traj), "the same seed twice"
    for _ in range(2):
        assert torch.equal(env.run(pipe, [r(1)], 2, eta=eta, use_graph=True)[1], traj), "graph replay != eager"
    single2, _ = env.run(pipe, [r(2)], 2, eta=eta)
    for use_graph in (False, True):
        many, _ = env.run(pipe, [r(1), r(2)], 2, eta=eta, use_graph=use_graph)
        assert torch.equal(many[0], full[0]) and torch.equal(many[1], single2[0]), f"batched != single (graph={use_graph})"
    for stage in (2, 1):
        want = env.run(pipe, [r(1), r(2)], stage, eta=eta)[1]
        assert torch.equal(env.run(pipe, [r(1), r(2)], stage, eta=eta, dedup=True)[1], want), f"stage {stage}: dedup"
        assert torch.equal(env.run(pipe, [r(1), r(2)], stage, eta=eta, dedup=True, use_graph=True)[1], want), f"stage {stage}: dedup, graph"
    s1 = env.run(pipe, [r(1)], 1, eta=eta)[1]
    assert not torch.equal(s1[0, 0, 0], s1[0, 0, 1]) and not torch.equal(s1[-1, 0, 0], s1[-1, 0, 1]), "stage 1: the samples differ"
    other, _ = env.run(pipe, [r(1, gseed=5)], 2, eta=eta)
    assert (other - full).abs().max() > 0.1, "another seed, other noise"


@pytest.mark.parametrize("use_graph", [False, True])
def test_stage_two_resume_stochastic(dev, use_graph):
    """Euler-ancestral: a StageCache entry holds the noise identity (the generator's state in front of the noise draws); the stage-2 call
    resumed from the stage-1 call of the same seed equals the uncached call bit for bit, plain and with drop_unc0; another seed misses
    and gives another result"""
    S, fstart = 9, 3
    env = _env(dev, S, fstart)
    pipe = LoraMultiConceptPipeline(env.unet, make_scheduler("euler_a"))
    r = env.request
    two = lambda: [r(1), r(2)]                                 # fresh generators every call
    full, full_traj = env.run(pipe, two(), 2, use_graph=use_graph)
    cache = StageCache()
    s1, s1_traj = env.run(pipe, two(), 1, stage_cache=cache, dedup=True, use_graph=use_graph)
    assert len(cache.entries) == 2 and cache.misses == 2 and cache.hits == 0
    assert torch.equal(s1_traj[fstart], full_traj[fstart]), "steps 0..fusion_start of the two stages coincide"
    resumed, r_traj = env.run(pipe, two(), 2, stage_cache=cache, use_graph=use_graph)
    assert cache.hits == 2 and len(r_traj) == S - (fstart + 1)
    assert torch.equal(resumed, full) and torch.equal(r_traj, full_traj[fstart + 1:])
    assert torch.equal(resumed[:, 0], s1[:, 0]), "the base sample of stage 2 is the stage-1 image"
    h0 = cache.hits
    dropped, d_traj = env.run(pipe, two(), 2, stage_cache=cache, drop_unc0=True, use_graph=use_graph)
    assert cache.hits == h0 + 2 and torch.equal(dropped, full) and torch.equal(d_traj, full_traj[fstart + 1:])
    # another seed of the noise (same embeddings, same latents) misses and runs in full
    lat = torch.randn(1, 4, full.shape[-2], full.shape[-1], generator=torch.Generator().manual_seed(8))
    env.run(pipe, [dict(r(1), latents=lat)], 1, stage_cache=cache, use_graph=use_graph)
    h0 = cache.hits
    got, t_ = env.run(pipe, [dict(r(1, gseed=6), latents=lat)], 2, stage_cache=cache, use_graph=use_graph)
    assert cache.hits == h0 and len(t_) == S
    want, _ = env.run(pipe, [dict(r(1, gseed=6), latents=lat)], 2, use_graph=use_graph)
    assert torch.equal(got, want)
    hit, _ = env.run(pipe, [dict(r(1), latents=lat)], 2, stage_cache=cache, use_graph=use_graph)
    assert cache.hits == h0 + 1 and (hit - got).abs().max() > 0.1


def test_ddim_eta_switch_on_one_pipe_equals_fresh_pipes(dev):
    """DDIM eta 0 -> 1 -> 0 through one pipe (engines, graphs, tables) == each on a fresh pipe; eta = 0 draws nothing (a call without a
    generator for the noise is the same); Euler-discrete ignores eta; a stage-1 entry of eta = 0 is not resumed by eta = 1"""
    S, fstart = 6, 2
    env = _env(dev, S, fstart)
    r = env.request
    etas = [0.0, 1.0, 0.0]
    fresh = [env.run(LoraMultiConceptPipeline(env.unet, DDIMScheduler()), [r(1)], 2, eta=e, use_graph=True)[0] for e in etas]
    assert not torch.equal(fresh[0], fresh[1]) and torch.equal(fresh[0], fresh[2])
    one = LoraMultiConceptPipeline(env.unet, DDIMScheduler())
    for e, want in zip(etas, fresh):
        for _ in range(2):                              # capture, then replay
            assert torch.equal(env.run(one, [r(1)], 2, eta=e, use_graph=True)[0], want), e
    lat = torch.randn(1, 4, fresh[0].shape[-2], fresh[0].shape[-1], generator=torch.Generator(dev).manual_seed(1), device=dev)
    no_gen = dict(r(1), generator=None, latents=lat)
    assert torch.equal(env.run(one, [no_gen], 2, eta=0.0)[0], fresh[0]), "eta = 0 draws no noise"
    eu = LoraMultiConceptPipeline(env.unet, make_scheduler("euler"))
    assert torch.equal(env.run(eu, [r(1)], 2, eta=1.0)[0], env.run(eu, [r(1)], 2, eta=0.0)[0]), "Euler-discrete ignores eta"
    cache = StageCache()
    env.run(one, [r(1)], 1, eta=0.0, stage_cache=cache)
    h0 = cache.hits
    assert torch.equal(env.run(one, [r(1)], 2, eta=1.0, stage_cache=cache)[0], fresh[1]) and cache.hits == h0
    assert torch.equal(env.run(one, [r(1)], 2, eta=0.0, stage_cache=cache)[0], fresh[0]) and cache.hits == h0 + 1


def test_concept_shard_with_a_stochastic_step_is_refused(dev):
    S, fstart = 4, 1
    env = _env(dev, S, fstart)
    pipe = LoraMultiConceptPipeline(env.unet, make_scheduler("euler_a"))
    with pytest.raises(L.OmgHipError, match="concept_shard"):
        pipe.generate_many([env.request(1)], stage=2, concept_shard=ConceptShard(rank=0, world=2), **env.kw)
    pipe.scheduler = DDIMScheduler()
    with pytest.raises(L.OmgHipError, match="concept_shard"):
        pipe.generate_many([env.request(1)], stage=2, eta=0.5, concept_shard=ConceptShard(rank=0, world=2), **env.kw)
