"""Word-swap / windowed prompt-to-prompt edits through the whole denoising loop (-m gpu): the tiny (32, 64, 128) topology, an 8-step
two-stage DDIM call with two masked concepts, "a man on the road" -> "a woman on the road" with per-word cross-replace windows and
self_replace_steps = (0.0, 0.5).  Against the oracle's literal loop at the existing loop tolerance (2e-2 of the latent rms at the last
step); captured graphs bitwise equal to eager (alpha is read through the device step counter: a graph recorded at one step and replayed
at another must follow it); three requests in lock-step bitwise equal to each alone; and the pure-replacement controller's launches
are the ones it made before the general path existed."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from omg_amd import _lib as L
from omg_amd import controller as pc
from omg_amd.lora import LoraAdapter, LoraBank
from omg_amd.pipeline import ConceptModels, LoraMultiConceptPipeline, revise_regionally_controlnet_forward
from omg_amd.schedulers import make_scheduler
from omg_amd.unet import UNet2DConditionModel, UNetConfig
from oracle import controller as oc
from oracle import pipeline as opipe
from oracle import schedulers as osched
from oracle import unet as ou

SWAP = ["a man on the road", "a woman on the road"]
WINDOWS = {"default_": 0.6, "road": (0.2, 0.9)}
S, GS, FSTART = 8, 7.5, 3
DT = torch.float16


def embeds(cfg, n, seed):
    g = torch.Generator().manual_seed(seed)
    e = torch.randn(n, 77, cfg.cross_attention_dim, generator=g).to(DT).float()
    p = torch.randn(n, cfg.projection_class_embeddings_input_dim - 6 * cfg.addition_time_embed_dim, generator=g).to(DT).float()
    return e, p


class World:
    """One UNet with its LoRA bank and pipeline, shared by the tests of this file; the installed controller is swapped per test."""

    def __init__(self, dev):
        self.dev = dev
        self.cfg, self.ocfg = UNetConfig.tiny(), ou.UNetConfig.tiny()
        self.sd = ou.init_state_dict(self.ocfg, seed=0, dtype=DT)
        self.unet = UNet2DConditionModel(self.cfg, dtype=DT, device=dev)
        self.unet.load_state_dict({k: v.to(DT) for k, v in self.sd.items()})
        self.Lat = self.cfg.sample_size
        self.H = self.W = self.Lat * 8
        names = ou.lora_target_names(self.ocfg)
        self.ow, self.olora = [], []
        for c in range(2):
            w, fn = ou.make_lora(self.ocfg, names, rank=8, seed=100 + c, scale=0.8, dtype=DT)
            self.ow.append(w); self.olora.append(fn)
        bank = LoraBank(self.unet, [LoraAdapter(f"c{c}", {k: (a.to(dev), b.to(dev)) for k, (a, b) in self.ow[c].items()}) for c in range(2)])
        self.concept = ConceptModels(self.unet, bank)
        self.pipe = LoraMultiConceptPipeline(self.unet, make_scheduler("ddim"))
        self.tid = torch.tensor([[self.H, self.W, 0, 0, self.H, self.W]], dtype=torch.float32)

    def args(self, prompts, cross):
        return (prompts, S, dict(cross) if isinstance(cross, dict) else cross, (0.0, 0.5), self.Lat // 4, self.Lat // 4)

    def controller(self, prompts, cross):
        ctl = pc.AttentionReplace(*self.args(prompts, cross), tokenizer=oc.PieceTokenizer(), device=self.dev, dtype=DT)
        revise_regionally_controlnet_forward(self.unet, ctl)
        return ctl

    def request(self, seed):
        """The two samples of a request have different prompt embeddings (base prompt / swapped prompt)."""
        H, W = self.H, self.W
        pe, pp = embeds(self.cfg, 2, seed)
        ne1, np1 = embeds(self.cfg, 1, seed + 50)
        regions = []
        for c in range(2):
            re_, rp_ = embeds(self.cfg, 2, seed + 10 + c)
            regions.append((re_[0:1], re_[1:2], rp_[0:1], rp_[1:2]))
        m1 = torch.zeros(H, W); m1[H // 4:, : W // 2 + 8 * (seed % 3)] = 1
        m2 = torch.zeros(H, W); m2[H // 8:, W // 2 - 16:] = 1
        return dict(prompt_embeds=pe, negative_prompt_embeds=ne1.repeat(2, 1, 1), pooled_prompt_embeds=pp,
                    negative_pooled_prompt_embeds=np1.repeat(2, 1), region_prompt_embeds=regions, region_masks=[m1, m2],
                    latents=torch.randn(1, 4, self.Lat, self.Lat, generator=torch.Generator().manual_seed(seed)))

    def run(self, ctl, reqs, stage=2, use_graph=False, trajectory=None):
        ctl.reset()
        out = self.pipe.generate_many(reqs, height=self.H, width=self.W, num_inference_steps=S, guidance_scale=GS,
                                      cross_attention_kwargs={"scale": 0.8}, controller=ctl, concept_models=self.concept, stage=stage,
                                      lora_list=["c0", "c1"], styleL=False, fusion_start=FSTART, use_graph=use_graph, trajectory=trajectory)
        assert (ctl.cur_step, ctl.cur_att_layer) == (S, 0)
        return out.cpu()

    def oracle(self, ctl, prompts, cross, r, stage):
        octl = oc.AttentionReplaceOracle(*self.args(prompts, cross), tokenizer=oc.PieceTokenizer())
        octl.num_att_layers = ctl.num_att_layers
        attn = oc.reference_attn_fn(octl)
        osch = osched.make("ddim", S)
        ctx4 = torch.cat([r["negative_prompt_embeds"], r["prompt_embeds"]])
        te4 = torch.cat([r["negative_pooled_prompt_embeds"], r["pooled_prompt_embeds"]])
        sd, ocfg, tid = self.sd, self.ocfg, self.tid

        def main(x, i):
            return ou.unet_forward(sd, ocfg, x, float(osch.timesteps[i]), ctx4, te4, tid.repeat(4, 1), attn_fn=attn)

        def conc(c):
            reg = r["region_prompt_embeds"][c]
            ctx2, te2 = torch.cat([reg[0], reg[1]]), torch.cat([reg[2], reg[3]])
            return lambda x, i: ou.unet_forward(sd, ocfg, x, float(osch.timesteps[i]), ctx2, te2, tid.repeat(2, 1), lora=self.olora[c])
        return opipe.denoise(main, [conc(c) for c in range(2)], osch, r["latents"] * osch.init_noise_sigma, S, GS, stage,
                             masks=r["region_masks"], fusion_start=FSTART)


@pytest.fixture(scope="module")
def world(dev):
    return World(dev)


def rel_err(got, ref):
    return (got.float() - ref).abs().max().item() / ref.pow(2).mean().sqrt().item()


@pytest.mark.parametrize("stage", [1, 2])
def test_word_swap_loop_matches_the_oracle(world, stage):
    ctl = world.controller(SWAP, WINDOWS)
    assert not ctl.is_pure_replacement and [ctl.cross_kind(s) for s in range(S)] == ["mixed"] * S
    r = world.request(1)
    got = world.run(ctl, [r], stage=stage)[0]
    ref = world.oracle(ctl, SWAP, WINDOWS, r, stage)
    rel = rel_err(got, ref)
    print(f"word swap, stage {stage}: max|d| / latent rms = {rel:.3e}")
    assert rel < 2e-2, rel
    assert (ref[1] - ref[0]).abs().max() > 0.1, "the swapped prompt must give another image"


def test_equal_prompts_with_a_cross_window_match_the_oracle(world):
    prompts = [SWAP[0]] * 2
    ctl = world.controller(prompts, 0.5)
    kinds = [ctl.cross_kind(s) for s in range(S)]
    assert kinds == ["borrow"] * 4 + ["own"] * 4 and not ctl.is_pure_replacement
    r = world.request(2)
    got = world.run(ctl, [r], stage=2)[0]
    rel = rel_err(got, world.oracle(ctl, prompts, 0.5, r, 2))
    print(f"equal prompts, cross_replace_steps 0.5: max|d| / latent rms = {rel:.3e}")
    assert rel < 2e-2, rel


def test_graph_replay_is_bitwise_equal_to_eager(world):
    """The first graph call captures each regime at its SECOND step and replays it at the later ones; the second call replays every step,
    including the ones in front of the step a graph was recorded at, whose alpha rows differ ("road" joins at step 1, the default window
    closes at step 5): an alpha baked in at capture time cannot pass."""
    ctl = world.controller(SWAP, WINDOWS)
    def steps(seed, use_graph):
        traj = []
        world.run(ctl, [world.request(seed)], use_graph=use_graph, trajectory=traj)
        return [x.cpu() for x in traj]

    eager = [steps(seed, False) for seed in (1, 2)]
    graph = [steps(seed, True) for seed in (1, 2, 1)]
    for a, b in ((eager[0], graph[0]), (eager[1], graph[1]), (eager[0], graph[2])):
        assert len(a) == len(b) == S
        for i, (x, y) in enumerate(zip(a, b)):
            assert torch.equal(x, y), f"step {i}: graph replay differs from eager by {(x - y).abs().max().item()}"
    assert not torch.equal(eager[0][-1], eager[1][-1])


def test_three_word_swap_requests_in_lock_step_equal_each_alone(world):
    ctl = world.controller(SWAP, WINDOWS)
    singles = [world.run(ctl, [world.request(seed)])[0] for seed in (1, 2, 3)]
    for use_graph in (False, True):
        many = world.run(ctl, [world.request(seed) for seed in (1, 2, 3)], use_graph=use_graph)
        for j in range(3):
            assert torch.equal(many[j], singles[j]), f"request {j} (graph={use_graph}): max diff {(many[j] - singles[j]).abs().max().item()}"


class _Recorder:
    """Stands in for the ctypes library object: the names of the `omg_*` calls, in order."""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("omg_") or name == "omg_last_error":
            return fn

        def recorded(*a):
            self.names.append(name)
            return fn(*a)
        return recorded


def test_a_pure_replacement_step_launches_what_it_always_did(world, monkeypatch):
    """The default controller (identity mapper, alpha = 1) must not move: its forward goes through ``fused_qk_src`` only — never through
    ``fused_edit`` — and its launch sequence is the one of a UNet without the general path: one omg_attn_fwd per attention layer, no
    mapped transpose, no materialised probabilities."""
    dev, cfg = world.dev, world.cfg
    ctl = pc.AttentionReplace([SWAP[0]] * 2, S, {"default_": 1.0}, (0.0, 0.5), world.Lat // 4, world.Lat // 4, device=dev, dtype=DT)
    revise_regionally_controlnet_forward(world.unet, ctl)
    assert ctl.is_pure_replacement
    monkeypatch.setattr(ctl, "fused_edit", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the pure path must not call fused_edit")))
    g = torch.Generator().manual_seed(0)
    x = torch.randn(4, 4, world.Lat, world.Lat, generator=g).to(dev)
    ctx = torch.randn(4, 77, cfg.cross_attention_dim, generator=g).to(DT).to(dev)
    te = torch.randn(4, 64, generator=g).to(DT).to(dev)
    tid = world.tid.repeat(4, 1).to(dev)
    fwd = lambda: world.unet(x, 981, encoder_hidden_states=ctx, added_cond_kwargs={"text_embeds": te, "time_ids": tid})[0]
    fwd()
    ctl.reset()
    rec = _Recorder(L.lib())
    monkeypatch.setattr(L, "_lib", rec)
    try:
        y = fwd()
    finally:
        monkeypatch.setattr(L, "_lib", rec._lib)
    assert rec.names.count("omg_attn_fwd") == ctl.num_att_layers
    assert not {"omg_transpose_v_mapped", "omg_attn_probs", "omg_attn_apply_probs"} & set(rec.names)
    assert (ctl.cur_step, ctl.cur_att_layer) == (1, 0)
    ctl.reset()
    fwd2 = fwd()
    assert torch.equal(y, fwd2)
