"""DPM-Solver++ multistep on the GPU (-m gpu): the multistep step kernel (omg_fuse_cfg_step_ms) against a float64 recomputation and
through a captured hipGraph; the denoising loop with DPMSolverMultistepScheduler against oracle.pipeline.denoise driven by the literal
restatement in tests/_dpm_oracle.py (LoRA flow and InstantID flow); and the engine's bitwise invariances (graph == eager, batched ==
single, dedup, StageCache resume with and without drop_unc0, switching schedulers on one pipe) with the multistep history buffer.

The loop and invariance cases run the bodies of the existing DDIM / Euler tests with the scheduler swapped in (monkeypatched factory),
so both schedulers are held to the same checks."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from omg_amd import ops
from omg_amd.lora import LoraAdapter, LoraBank
from omg_amd.pipeline import ConceptModels, LoraMultiConceptPipeline
from omg_amd.schedulers import MS_A, MS_B, MS_CM, MS_CP, MS_CX, DPMSolverMultistepScheduler, make_scheduler
from oracle import schedulers as osched
from oracle import unet as ou
from tests import _dpm_oracle as dpo
from tests import test_instantid_gpu as tig
from tests import test_pipeline_gpu as tpg

C_, H_, W_ = 4, 24, 20
GS = 7.5


def _mask_lr(m, H, W):
    Hm, Wm = m.shape
    ys = (torch.arange(H) * Hm) // H
    xs = (torch.arange(W) * Wm) // W
    return m[ys][:, xs] == 1.0


def ref_step(noise, lat, hist, row, fuse, regs, masks):
    """float64 restatement of one omg_fuse_cfg_step_ms launch (noise (4,C,H,W), lat / hist (2,C,H,W), all float64 on the host)"""
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
    m = row[MS_A] * lat + row[MS_B] * e
    out = row[MS_CX] * lat + row[MS_CM] * m
    if row[MS_CP] != 0.0:
        out = out + row[MS_CP] * hist
    return out, m


def kernel_inputs(dev, n_steps, seed=0):
    g = torch.Generator().manual_seed(seed)
    noise = [torch.randn(4, C_, H_, W_, generator=g) for _ in range(n_steps)]
    regs = [[torch.randn(2, C_, H_, W_, generator=g) for _ in range(3)] for _ in range(n_steps)]
    m1 = torch.zeros(2 * H_, 2 * W_); m1[H_ // 2:, : W_] = 1
    m2 = torch.zeros(2 * H_, 2 * W_); m2[H_ // 3:, W_ - 8:] = 1          # overlaps m1 (sum rule)
    masks = [m1, None, m2]                                              # concept 1: a region prediction without a mask is ignored
    lat = torch.randn(2, C_, H_, W_, generator=g)
    return noise, regs, masks, lat


@pytest.mark.parametrize("stype", ["midpoint", "heun"])
def test_multistep_step_kernel_matches_float64(dev, stype):
    """6 launches = order 1, four order-2 steps, order 1 (lower_order_final): fused masks with overlap and a None mask from step 2 on,
    next model input in fp16 / bf16 / fp32; the history buffer starts NaN-filled (order-1 rows must not read it)."""
    S = 6
    sch = DPMSolverMultistepScheduler(solver_type=stype)
    sch.set_timesteps(S)
    assert sch.orders == [1, 2, 2, 2, 2, 1]
    tab = sch.coef_table(dev)
    rows = tab.double().cpu()
    noise, regs, masks, lat0 = kernel_inputs(dev, S)
    lat = lat0.to(dev)
    hist = torch.full((2, C_, H_, W_), float("nan"), device=dev)
    step_idx = torch.zeros(1, dtype=torch.int32, device=dev)
    dmasks = [m.to(dev) if m is not None else None for m in masks]
    ref_lat, ref_hist = lat0.double(), torch.full((2, C_, H_, W_), float("nan"), dtype=torch.float64)
    for i, dt in enumerate([torch.float16, torch.bfloat16, torch.float32] * 2):
        fuse = i >= 2
        mi = torch.empty(4, C_, H_, W_, dtype=dt, device=dev)
        ops.fuse_cfg_step_ms(noise[i].to(dev), lat, tab, hist, step_idx, guidance_scale=GS, fuse=fuse,
                             region_preds=[r.to(dev) for r in regs[i]] if fuse else [None] * 3, masks=dmasks if fuse else [None] * 3,
                             model_input_next=mi, advance=True)
        ref_lat, ref_hist = ref_step(noise[i].double(), ref_lat, ref_hist, rows[i], fuse, [r.double() for r in regs[i]], masks)
        torch.cuda.synchronize()
        got_l, got_h = lat.double().cpu(), hist.double().cpu()
        assert not torch.isnan(got_l).any() and not torch.isnan(got_h).any(), f"step {i}"
        el = (got_l - ref_lat).abs().max() / ref_lat.pow(2).mean().sqrt()
        eh = (got_h - ref_hist).abs().max() / ref_hist.pow(2).mean().sqrt()
        assert el < 1e-5 and eh < 1e-5, (i, el.item(), eh.item())
        want_mi = torch.cat([lat, lat]).to(dt)                       # cin_next = 1
        assert torch.equal(mi, want_mi), f"step {i}: model input"
    assert step_idx.item() == S
    assert (rows[1:5, MS_CP] != 0).all() and (rows[[0, 5], MS_CP] == 0).all()


def test_multistep_keeps_coinciding_samples_bitwise_equal(dev):
    """stage 1: both samples see the same inputs, so latents AND histories stay bit-identical"""
    S = 6
    sch = DPMSolverMultistepScheduler(use_karras_sigmas=True, solver_type="heun")
    sch.set_timesteps(S)
    tab = sch.coef_table(dev)
    g = torch.Generator().manual_seed(5)
    lat = torch.randn(1, C_, H_, W_, generator=g).repeat(2, 1, 1, 1).to(dev)
    hist = torch.empty(2, C_, H_, W_, device=dev)
    step_idx = torch.zeros(1, dtype=torch.int32, device=dev)
    for i in range(S):
        u, c = torch.randn(1, C_, H_, W_, generator=g), torch.randn(1, C_, H_, W_, generator=g)
        ops.fuse_cfg_step_ms(torch.cat([u, u, c, c]).to(dev), lat, tab, hist, step_idx, guidance_scale=GS)
        assert torch.equal(lat[0], lat[1]) and torch.equal(hist[0], hist[1]), f"step {i}"


def test_multistep_step_graph_replay_equals_eager(dev):
    S = 6
    sch = DPMSolverMultistepScheduler()
    sch.set_timesteps(S)
    tab = sch.coef_table(dev)
    noise, regs, masks, lat0 = kernel_inputs(dev, S, seed=1)
    noise = [x.to(dev) for x in noise]
    regs = [[r.to(dev) for r in rs] for rs in regs]
    dmasks = [m.to(dev) if m is not None else None for m in masks]
    lat = torch.empty(2, C_, H_, W_, device=dev)
    hist = torch.empty(2, C_, H_, W_, device=dev)
    step_idx = torch.zeros(1, dtype=torch.int32, device=dev)
    mis = [torch.empty(4, C_, H_, W_, dtype=dt, device=dev) for dt in (torch.float16, torch.bfloat16, torch.float32) * 2]

    def reset():
        lat.copy_(lat0.to(dev)); hist.fill_(float("nan")); step_idx.zero_()

    def body():
        for i in range(S):
            fuse = i >= 2
            ops.fuse_cfg_step_ms(noise[i], lat, tab, hist, step_idx, guidance_scale=GS, fuse=fuse,
                                 region_preds=regs[i] if fuse else [None] * 3, masks=dmasks if fuse else [None] * 3, model_input_next=mis[i])

    reset()
    body()
    torch.cuda.synchronize()
    eager = (lat.clone(), hist.clone(), [m.clone() for m in mis])
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
        assert torch.equal(lat, eager[0]) and torch.equal(hist, eager[1])
        assert all(torch.equal(a, b) for a, b in zip(mis, eager[2]))


# ------------------------------------------------------------------------------------------------ the loop: the existing tests' bodies with DPM
def _dpm_factory(stype="midpoint", karras=False, names=("ddim", "dpm")):
    """make_scheduler with DPM-Solver++ in place of the schedulers called ``names`` (the others stay what they are)"""
    def make(name):
        return DPMSolverMultistepScheduler(solver_type=stype, use_karras_sigmas=karras) if name in names else make_scheduler(name)
    return make


def _oracle_factory(stype="midpoint", karras=False, names=("dpm",)):
    """oracle.schedulers.make with the literal DPM-Solver++ restatement in place of ``names``"""
    orig = osched.make

    def make(name, S):
        return dpo.DPMSolverPP(S, 2, stype, True, False, karras) if name in names else orig(name, S)
    return make


@pytest.mark.parametrize("stype,karras,lora_mode,lh,lw", [("midpoint", False, "merged", 16, 16), ("heun", True, "segment", 12, 20)])
def test_two_stage_loop_matches_oracle_with_dpm(dev, monkeypatch, stype, karras, lora_mode, lh, lw):
    """S = 8, fusion_start = 3, 3 concepts with LoRA (overlapping masks + a None mask), the p2p controller: stage 1 and stage 2 against the
    oracle loop stepping the literal DPM-Solver++ restatement; rel < 2e-2 of the latent rms, stage-1 samples equal, base sample unaffected"""
    monkeypatch.setattr(tpg, "make_scheduler", _dpm_factory(stype, karras))
    monkeypatch.setattr(osched, "make", _oracle_factory(stype, karras))
    tpg.test_two_stage_loop_matches_oracle(dev, "dpm", lora_mode, lh, lw)


def test_instantid_loop_matches_oracle_with_dpm(dev, monkeypatch):
    monkeypatch.setattr(tig, "make_scheduler", _dpm_factory(names=("euler",)))
    monkeypatch.setattr(osched, "make", _oracle_factory(names=("euler",)))
    tig.test_instantid_loop_matches_oracle(dev, False, False)


def test_graph_replay_is_bitwise_equal_to_eager_with_dpm(dev, monkeypatch):
    monkeypatch.setattr(tpg, "make_scheduler", _dpm_factory())
    tpg.test_graph_replay_is_bitwise_equal_to_eager(dev)


def test_generate_many_equals_single_requests_with_dpm(dev, monkeypatch):
    monkeypatch.setattr(tpg, "make_scheduler", _dpm_factory("heun", True))
    tpg.test_generate_many_equals_single_requests(dev)


def test_dedup_is_bitwise_equal_to_the_full_batch_with_dpm(dev, monkeypatch):
    monkeypatch.setattr(tpg, "make_scheduler", _dpm_factory())
    tpg.test_dedup_of_identical_samples_is_bitwise_equal_to_the_full_batch(dev, False)


@pytest.mark.parametrize("use_graph", [False, True])
def test_stage_two_resume_with_dpm(dev, monkeypatch, use_graph):
    """the cached entry carries each request's data prediction of step fusion_start: the resumed call (plain and drop_unc0) equals the
    uncached call bit for bit"""
    monkeypatch.setattr(tpg, "make_scheduler", _dpm_factory())
    tpg.test_stage_two_resumes_from_the_stage_one_call_of_the_same_image(dev, use_graph)


def test_scheduler_swaps_on_one_pipe_equal_fresh_pipes(dev):
    """DDIM -> DPM -> DPM (Karras) -> DDIM through one pipe (engines, graphs, tables) == each scheduler on a fresh pipe; a StageCache entry
    of one DPM configuration is not resumed by another"""
    from omg_amd.pipeline import StageCache
    dtype = torch.float16
    cfg, ocfg, sd, unet = tpg.setup(dev, dtype)
    L = cfg.sample_size
    S, fstart = 6, 2
    H = W = L * 8
    names = ou.lora_target_names(ocfg)
    bank = LoraBank(unet, [LoraAdapter(nm, {k: (a.to(dev), b.to(dev)) for k, (a, b) in ou.make_lora(ocfg, names, 8, 100 + c, 0.8, dtype)[0].items()})
                           for c, nm in enumerate(["c0", "c1"])])
    concept = ConceptModels(unet, bank)
    pe1, pp1 = tpg.embeds(cfg, 1, 1, dtype); ne1, np1 = tpg.embeds(cfg, 1, 51, dtype)
    regions = []
    for c in range(2):
        re_, rp_ = tpg.embeds(cfg, 2, 11 + c, dtype)
        regions.append((re_[0:1], re_[1:2], rp_[0:1], rp_[1:2]))
    m1 = torch.zeros(H, W); m1[H // 4:, : W // 2] = 1
    m2 = torch.zeros(H, W); m2[H // 4:, W // 2 - 16:] = 1
    req = dict(prompt_embeds=pe1.repeat(2, 1, 1), negative_prompt_embeds=ne1.repeat(2, 1, 1), pooled_prompt_embeds=pp1.repeat(2, 1),
               negative_pooled_prompt_embeds=np1.repeat(2, 1), region_prompt_embeds=regions, region_masks=[m1, m2],
               latents=torch.randn(1, 4, L, L, generator=torch.Generator().manual_seed(1)))
    kw = dict(height=H, width=W, num_inference_steps=S, guidance_scale=7.5, cross_attention_kwargs={"scale": 0.8}, concept_models=concept,
              stage=2, lora_list=["c0", "c1"], styleL=False, fusion_start=fstart, use_graph=True)
    scheds = [lambda: make_scheduler("ddim"), lambda: make_scheduler("dpm"), lambda: DPMSolverMultistepScheduler(use_karras_sigmas=True),
              lambda: make_scheduler("ddim")]
    fresh = [LoraMultiConceptPipeline(unet, mk()).generate_many([req], **kw).cpu() for mk in scheds]
    one = LoraMultiConceptPipeline(unet, scheds[0]())
    for mk, want in zip(scheds, fresh):
        one.scheduler = mk()
        for _ in range(2):                              # capture, then replay
            assert torch.equal(one.generate_many([req], **kw).cpu(), want), type(one.scheduler).__name__
    assert not torch.equal(fresh[0], fresh[1]) and not torch.equal(fresh[1], fresh[2])
    # the cache keys hold the table bytes: a Karras entry is not resumed by the plain configuration, and vice versa
    cache = StageCache()
    one.scheduler = DPMSolverMultistepScheduler(use_karras_sigmas=True)
    one.generate_many([req], **dict(kw, stage=1, stage_cache=cache))
    assert len(cache.entries) == 1 and len(cache.history) == 1
    one.scheduler = make_scheduler("dpm")
    h0 = cache.hits
    assert torch.equal(one.generate_many([req], **dict(kw, stage_cache=cache)).cpu(), fresh[1]) and cache.hits == h0
    one.scheduler = DPMSolverMultistepScheduler(use_karras_sigmas=True)
    assert torch.equal(one.generate_many([req], **dict(kw, stage_cache=cache)).cpu(), fresh[2]) and cache.hits == h0 + 1
