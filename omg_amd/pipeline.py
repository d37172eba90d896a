"""OMG's two-stage denoising loop on the MI355X — boundary B3 of SURVEY.md §8b.

Mirrors ``LoraMultiConceptPipeline.__call__`` (/root/reference src/pipelines/lora_pipeline.py:212-669):
same keyword names and meaning for everything on the hot path (``num_inference_steps``,
``guidance_scale``, ``generator``/``latents``, ``cross_attention_kwargs={"scale": 0.8}``, ``controller``,
``concept_models``, ``stage`` in {1, 2}, ``region_masks``, ``lora_list``, ``styleL``), and the same batch
layout: latents duplicated x2 (:409), model input ``[unc0, unc1, cond0, cond1]`` (:467-474, :491), concept
pass on ``latent_model_input[3:4]`` duplicated (:583-585), fusion for ``i > 15 and stage == 2`` (:568).

Text encoders and the VAE are separate modules (rows N4 / N1 of SURVEY §8f).  Without them the call takes ``prompt_embeds`` /
pooled embeddings (the reference computes them at :315-347 and passes them on) and returns latents
(``output_type="latent"``), or decoded images (``"pil"``, the reference's default, / ``"pt"`` / ``"np"``) when the pipeline was built with
``vae_decode=omg_amd.vae.AutoencoderKLDecoder(...).decode_latents`` (row N1; the reference's tail at :635-661);
``prompt=`` works when the pipeline was built with ``encode_prompt=omg_amd.text_encoder.make_encode_prompt(...)``.

MI355X-first differences from the reference's loop, all value-preserving:
  * the K per-concept UNet passes of a step run as ONE batched forward with a per-sample LoRA slot;
  * time/text-conditioning embeddings of all steps are computed once before the loop;
  * fusion + CFG + scheduler step + next model input are one kernel, masks stay on the device
    (the reference copies each mask to the host every step and boolean-indexes, :572-602, :675-679);
  * each step regime (plain / fused, self-replace on / off) can be captured as a hipGraph.
"""
from __future__ import annotations

import warnings
from collections import namedtuple
from types import SimpleNamespace
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib as L
from . import ops, parallel
from .attention import Attention, RegionControlNet_AttnProcessor
from .lora import LoraBank
from .modules import LoraState, pointer_epoch
from .schedulers import DDIMScheduler, DPMSolverMultistepScheduler, draw_noise, is_stochastic

FUSION_START = 15   # `if i > 15 and stage == 2` (lora_pipeline.py:568) — absolute, not relative
CONCEPT_LORA_SCALE = 0.8   # `cross_attention_kwargs={'scale': 0.8}` of every concept UNet call (lora_pipeline.py:596), whatever the caller passes


def controlnet_keep(n_steps: int, start, end, n_nets: int = 1) -> List[List[float]]:
    """``controlnet_keep`` of the reference (lora_pipeline.py:275-286 broadcast + :421-428): for step i and net k the factor on the conditioning scale is
    1.0 while  start_k <= i / S  and  (i + 1) / S <= end_k,  else 0.0.  ``start`` / ``end``: scalars (every net) or one entry per net."""
    def per_net(v, other):
        if isinstance(v, (list, tuple)):
            return [float(x) for x in v]
        return [float(v)] * (len(other) if isinstance(other, (list, tuple)) else n_nets)
    starts, ends = per_net(start, end), per_net(end, start)
    if len(starts) != len(ends):
        raise ValueError(f"control_guidance_start has {len(starts)} entries, control_guidance_end {len(ends)}")
    return [[0.0 if (i / n_steps < s_ or (i + 1) / n_steps > e_) else 1.0 for s_, e_ in zip(starts, ends)] for i in range(n_steps)]


def revise_regionally_controlnet_forward(unet, controller) -> None:
    """Install the region/controller attention processor on every ``Attention`` of the UNet and set
    ``controller.num_att_layers`` — same name, traversal order and place labels (including the
    mid/up label swap, harmless because the label is unused) as lora_pipeline.py:136-152."""

    def change_forward(module, count, place_in_unet):
        for name, layer in module.named_children():
            if layer.__class__.__name__ == "Attention":
                layer.set_processor(RegionControlNet_AttnProcessor(controller=controller, place_in_unet=place_in_unet))
                if "attn2" in name:
                    count += 1
            else:
                count = change_forward(layer, count, place_in_unet)
        return count

    n = change_forward(unet.down_blocks, 0, "down")
    n = change_forward(unet.mid_block, n, "up")
    n = change_forward(unet.up_blocks, n, "mid")
    print(f"Number of attention layer registered {n}")
    controller.num_att_layers = n * 2


class ConceptModels:
    """What the reference's loop needs from ``concept_models`` (a second SDXL pipeline with the concept
    LoRAs loaded; inference_lora.py:159-170): ``unet(...)``, ``set_adapters(...)``, ``_execution_device``.
    Here the concept UNet shares the base weights of the main UNet; adapters live in a :class:`LoraBank`."""

    def __init__(self, unet, bank: Optional[LoraBank] = None):
        self._unet = unet
        self.bank = bank
        self._active: Tuple[Tuple[str, float], ...] = ()
        self._state_cache: Dict[Tuple, LoraState] = {}

    @property
    def _execution_device(self):
        return self._unet.device

    def set_adapters(self, adapter_names, adapter_weights=None) -> None:
        if isinstance(adapter_names, str):
            adapter_names = [adapter_names]
        if adapter_weights is None:
            adapter_weights = [1.0] * len(adapter_names)
        self._active = tuple((n, float(w)) for n, w in zip(adapter_names, adapter_weights))

    def lora_state(self, slots: Sequence[int], merged: bool = False) -> Optional[LoraState]:
        """``slots[b]`` = LoRA slot of sample b.  segment mode: -1 = no adapter; merged mode: 0 = base weights,
        s+1 = bank slot s."""
        if self.bank is None:
            return None
        key = (tuple(slots), merged)
        st = self._state_cache.get(key)
        if st is None:
            st = LoraState(torch.tensor(list(slots), dtype=torch.int32, device=self._unet.device), len(slots), merged)
            self._state_cache[key] = st
        return st

    def unet_batched(self, sample, timestep, encoder_hidden_states, slots: Sequence[int], **kw):
        """Concept forward where sample b uses LoRA slot ``slots[b]``; bypasses the p2p controller."""
        cak = dict(kw.pop("cross_attention_kwargs", None) or {})
        cak["omg_bypass_controller"] = True
        merged = self.bank is not None and self.bank.mode == "merged"
        if merged:
            slots = [s + 1 for s in slots]            # slot 0 of the merged stacks is the base weight
        self._unet.set_lora_state(self.lora_state(slots, merged))
        try:
            return self._unet(sample, timestep, encoder_hidden_states=encoder_hidden_states, cross_attention_kwargs=cak, **kw)
        finally:
            self._unet.set_lora_state(None)

    def unet(self, sample, timestep, encoder_hidden_states=None, cross_attention_kwargs=None, added_cond_kwargs=None,
             return_dict=False, **kw):
        """Reference call shape (lora_pipeline.py:592-599): whole batch uses the adapters chosen by ``set_adapters``."""
        slot = self.bank.slot_of(self._active) if self.bank is not None and self._active else -1
        return self.unet_batched(sample, timestep, encoder_hidden_states, [slot] * sample.shape[0],
                                 cross_attention_kwargs=cross_attention_kwargs, added_cond_kwargs=added_cond_kwargs,
                                 return_dict=return_dict, **kw)


class StageCache:
    """Exact redundancy BETWEEN the two calls of one image (OFF unless a cache object is passed; "flag when used").

    The reference's flow is stage 1 -> segment -> stage 2 with the SAME seed, prompts and kwargs (inference_lora.py:262-297), and the
    fusion branch only fires for ``i > 15`` (lora_pipeline.py:568): steps 0..15 of the stage-2 call repeat steps 0..15 of the stage-1
    call operation for operation.  A call with ``stage_cache=cache`` that runs those steps stores, per request, the latents ENTERING
    the first fused step under a key made of everything that determines them (initial latents, all main-pass embeddings, step count,
    guidance, scheduler table, size, adapters, ControlNet + image, UNet identity and weight version); a later stage-2 call that finds
    every request's key starts at step 16 from the stored latents — 16 x 4 sample-forwards per image fewer, bitwise the same result
    with this package's batch-invariant deterministic kernels (tests/test_pipeline_gpu.py).  Nothing is assumed: a miss runs the full call."""

    def __init__(self, max_entries: int = 64):
        self.entries: Dict[str, torch.Tensor] = {}
        self.base: Dict[str, Dict[int, Tuple[torch.Tensor, torch.Tensor]]] = {}
        self.history: Dict[str, torch.Tensor] = {}
        self.max_entries = max_entries
        self.hits = 0
        self.misses = 0

    @staticmethod
    def digest(*parts) -> str:
        import hashlib
        h = hashlib.sha1()
        for p in parts:
            if torch.is_tensor(p):
                h.update(str((tuple(p.shape), str(p.dtype))).encode())
                h.update(p.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes())
            else:
                h.update(repr(p).encode())
        return h.hexdigest()

    def put(self, key: str, latents: torch.Tensor) -> None:
        if key not in self.entries and len(self.entries) >= self.max_entries:
            old = next(iter(self.entries))
            self.entries.pop(old)
            self.base.pop(old, None)
        self.entries[key] = latents.detach().clone()

    def get(self, key: str) -> Optional[torch.Tensor]:
        return self.entries.get(key)

    # ---- the BASE sample's trajectory behind the first fused step (last item): sample 0 of a call is never fused
    # (lora_pipeline.py:605-607 write samples 1 and 3 only), so its latents at every step are those of the stage-1 call.  With them
    # cached the stage-2 call need not compute `unc0` at all (its prediction only feeds sample 0's update); `cond0` stays — `cond1`
    # borrows its attention probabilities — and is fed the cached latents.
    def put_base(self, key: str, k: int, latents0: torch.Tensor, model_input0: torch.Tensor) -> None:
        """sample 0 ENTERING step k: its latents (fp32) and the scaled model input the step kernel wrote for it"""
        self.base.setdefault(key, {})[k] = (latents0.detach().clone(), model_input0.detach().clone())

    def get_base(self, key: str, first: int, n_steps: int):
        """{k: (latents0, model_input0)} for k = first + 1 .. n_steps if every step is there, else None"""
        b = self.base.get(key)
        if b is None or any(k not in b for k in range(first + 1, n_steps + 1)):
            return None
        return b

    # ---- a multistep scheduler's state (DPMSolverMultistepScheduler): the step after the stored latents also reads the data prediction
    # of the step before them, so an entry of such a call holds both; an entry without it is not resumed from
    def put_history(self, key: str, x0_hist: torch.Tensor) -> None:
        """the (2, C, H, W) data predictions of the step that produced the latents stored under ``key``"""
        self.history[key] = x0_hist.detach().clone()
        for k in [k for k in self.history if k not in self.entries]:      # put() evicted its entry
            del self.history[k]

    def get_history(self, key: str) -> Optional[torch.Tensor]:
        return self.history.get(key) if key in self.entries else None

    # ---- one call's use of the cache: its keys (stage_cache_keys below), what it resumes from, what it stores after a step
    # per request: latents (+ multistep history); drop_unc0: per step k the (n, C, H, W) latents / model inputs of the base samples
    Resume = namedtuple("Resume", "first latents history base_traj", defaults=(0, None, None, None))

    def lookup(self, keys: Sequence[str], plan: "CallPlan", device, dtype) -> "StageCache.Resume":
        """A stage-2 call resumes at the first fused step when EVERY request's key is there (with a multistep scheduler: and its history);
        ``plan.drop_unc0``: with the base samples' trajectory when every request has all of it."""
        hit = [self.get(k) for k in keys]
        hist = None
        if plan.multistep:      # the first resumed step also reads the data prediction of the step in front of it
            hist = [self.get_history(k) for k in keys]
            hit = [h if m is not None else None for h, m in zip(hit, hist)]
        if not (plan.fuse_possible and all(h is not None for h in hit)):
            self.misses += len(keys)
            return self.Resume()
        first, base_traj = plan.fusion_start + 1, None                   # every request resumes: the plain steps are not run at all
        self.hits += len(keys)
        if plan.drop_unc0:
            bases = [self.get_base(k, first, plan.S) for k in keys]
            if all(b is not None for b in bases):
                base_traj = {k: (torch.cat([b[k][0] for b in bases]).to(device), torch.cat([b[k][1] for b in bases]).to(device=device, dtype=dtype))
                             for k in range(first + 1, plan.S + 1)}
        return self.Resume(first, hit, hist, base_traj)

    def store(self, keys: Sequence[str], i: int, fusion_start: int, lat: torch.Tensor, xin: torch.Tensor, x0_hist: Optional[torch.Tensor]) -> None:
        """After step i of a call that started at step 0: ``lat`` (2n, ...) latents, ``xin`` next model inputs, ``x0_hist`` of a multistep scheduler."""
        if i == fusion_start:                                           # the latents entering the first fused step of a stage-2 call
            for j, k in enumerate(keys):
                self.put(k, lat[2 * j: 2 * j + 2])
                if x0_hist is not None:                                 # ... and the data prediction that step reads besides them
                    self.put_history(k, x0_hist[2 * j: 2 * j + 2])
        if i >= fusion_start:                                           # ... and the base sample's way from there on (drop_unc0)
            for j, k in enumerate(keys):
                self.put_base(k, i + 1, lat[2 * j: 2 * j + 1], xin[4 * j + 2: 4 * j + 3])


def stage_cache_keys(p: "CallPlan", sizes: tuple, unet, bank, controller, controlnet, t) -> List[str]:
    """Per request, the digest of everything that determines the latents entering step ``fusion_start + 1`` (see :class:`StageCache`);
    ``p``: the call's plan; ``sizes``: height, width, original size, the negative micro-conditioning or None, crop, target size, dtype."""
    common = (p.S, p.guidance_scale, p.scheduler_name, p.fusion_start) + sizes + (
              tuple(p.main_adapters), p.main_scale, p.lora_mode if p.main_adapters else None,
              id(unet), getattr(unet, "weights_version", 0), getattr(bank, "version", None) if p.main_adapters else None,
              None if controller is None else (type(controller).__name__, p.pure_controller, getattr(controller, "num_self_replace", None)),
              None if not p.use_cn else (id(controlnet), getattr(controlnet, "weights_version", 0), p.cn_scale,
                                         tuple(k[0] for k in p.cn_keep[: p.fusion_start + 1])))
    keys = []
    for j in range(p.n):
        cn_img = None if not p.use_cn else (t.cn_image if t.cn_image.shape[0] == 1 else t.cn_image[j: j + 1])
        z_key = (t.zid_l[j],) if p.stochastic else ()        # a trajectory is valid for the same noise only
        keys.append(StageCache.digest(common, t.coef, t.lats[j], t.ehs_l[j], t.text_l[j], cn_img, *z_key))
    return keys


# Parameters of the reference's ``__call__`` (lora_pipeline.py:212-255, instantid_pipeline.py:215-259) that change ITS output when they leave their
# default and that this engine does not implement: name -> (the default, where the reference uses it).  A non-default value is REFUSED — ignoring
# it would return an image the reference would not have produced, without a word.
_UNIMPLEMENTED = {
    "num_images_per_prompt": (1, "lora_pipeline.py:223"), "ip_adapter_image": (None, "lora_pipeline.py:231"),
}
# Implemented in round 6 and therefore no longer here: guess_mode, control_guidance_start / _end, a list of ControlNets (generate_many), prompt_2 /
# negative_prompt_2 / clip_skip (omg_amd.text_encoder.make_encode_prompt), negative_original_size / _crops_coords_top_left / _target_size, callback /
# callback_steps / callback_on_step_end (+ _tensor_inputs).
# names the reference's own ``**kwargs`` swallows without reading (the shipped scripts pass them: inference_lora.py:241-245), or reads only
# together with a callback
_REFERENCE_IGNORES = ("spatial_condition", "indices_to_alter")
_CALLBACK_TENSORS = ("latents", "prompt_embeds", "negative_prompt_embeds")      # _callback_tensor_inputs (lora_pipeline.py:165)


def refuse_unimplemented(given: dict, leftovers: dict, who: str) -> None:
    """``given``: the reference-signature parameters this engine does not implement, as the caller passed them; ``leftovers``: what is
    still in ``**kwargs`` after the engine took its own.  Raises OmgHipError for a non-default reference parameter and for a name nobody knows."""
    for name, value in given.items():
        default, where = _UNIMPLEMENTED[name]
        v = value[0] if isinstance(value, (list, tuple)) and len(value) == 1 and not isinstance(default, tuple) else value
        v = tuple(v) if isinstance(default, tuple) and isinstance(v, (list, tuple)) else v
        if not (v is default or v == default):
            raise L.OmgHipError(f"{who}: {name}={value!r} is not implemented (the reference uses it at {where}); only the default {default!r} is")
    unknown = [k for k in leftovers if k not in _REFERENCE_IGNORES]
    if unknown:
        raise L.OmgHipError(f"{who}: unknown keyword argument(s) {sorted(unknown)} — neither a parameter of the reference's __call__ nor one of this engine's")


class StableDiffusionXLPipelineOutput(SimpleNamespace):
    pass


class CallPlan(SimpleNamespace):
    """Every decision ``generate_many`` makes before it touches a device buffer, made by the constructor from plain values: which rows a
    step runs, which LoRA slot each row gets, which mode falls back to the full batch, what is refused, what keys the engine.  Two
    fields are settled on the device afterwards: ``twin`` survives only if the two samples' embeddings compare equal, and
    :meth:`with_drop0` follows the stage cache's answer."""

    def __init__(self, *, n: int, lora_list: Sequence[str], S: int, stage, fusion_start: int = FUSION_START, active: Sequence[int] = (),
                 scheduler_cls=DDIMScheduler, stochastic: bool = False, guidance_scale: float = 5.0, use_graph: bool = False,
                 n_nets: Optional[int] = None, cn_image_shapes=(), controlnet_conditioning_scale=1.0, guess_mode: bool = False,
                 control_guidance_start=0.0, control_guidance_end=1.0, has_identitynet: bool = False, identitynet_conditioning_scale: float = 1.0,
                 dedup: bool = False, stage_cache: bool = False, drop_unc0: bool = False, concept_shard=None, has_controller: bool = False,
                 pure_controller: bool = False, callback: bool = False, callback_steps=None, callback_on_step_end: bool = False,
                 callback_on_step_end_tensor_inputs=("latents",), has_concept_models: bool = True, shared: bool = True, bank_adapters=None,
                 bank_mode: Optional[str] = None, lora_mode: str = "merged", concept_lora: bool = True, styleL=None, main_adapters=None,
                 concept_adapters=None, concept_adapter_scale: float = 1.0, main_scale: float = 1.0):
        """``n_nets`` / ``cn_image_shapes``: how many ControlNets were passed (None: none) and the shape of each conditioning image (None: missing);
        ``bank_adapters`` / ``bank_mode``: of ``concept_models.bank`` (None: no bank); ``shared``: the concept UNet is the pipeline's own;
        the ``has_*`` / callback flags: whether the object was passed.  Everything else as ``generate_many`` takes it."""
        self.n, self.S, self.fusion_start, self.lora_list, self.active = n, S, fusion_start, tuple(lora_list), tuple(active)
        self.K, self.Ka = K, Ka = len(self.lora_list), len(self.active)
        self.cn_image_shapes, self.lora_mode, self.shared = tuple(cn_image_shapes), lora_mode, shared
        self.guidance_scale, self.idn_scale, self.styleL = float(guidance_scale), float(identitynet_conditioning_scale), bool(styleL)
        self.scheduler_name, self.stochastic = scheduler_cls.__name__, stochastic      # stochastic: omg_fuse_cfg_step_noise + the per-step noise eng.z
        self.multistep = issubclass(scheduler_cls, DPMSolverMultistepScheduler)         # omg_fuse_cfg_step_ms + the history buffer eng.x0_hist
        self.pure_controller, self.drop0 = pure_controller, False
        # ---- ControlNet plan: one net without guess_mode runs on the engine's original single-net path (twin / shard / stage-cache aware); a list of
        # nets or guess_mode on the general path `cn_multi` (full batch only)
        n_cn = n_nets or 0
        scs = list(controlnet_conditioning_scale) if isinstance(controlnet_conditioning_scale, (list, tuple)) else [controlnet_conditioning_scale] * n_cn
        if n_nets is not None and (not n_nets or len(cn_image_shapes) != n_nets or len(scs) < n_nets or any(s is None for s in cn_image_shapes)):
            raise ValueError(f"{n_nets} ControlNet(s) need as many conditioning images and scales (got {len(cn_image_shapes)} image(s), {len(scs)} scale(s))")
        self.use_cn, self.cn_guess = n_cn == 1 and not guess_mode, bool(guess_mode)
        self.cn_multi = n_cn > 0 and not self.use_cn
        self.cn_scale = 1.0 if self.cn_multi else float(scs[0] if self.use_cn else controlnet_conditioning_scale)
        self.cn_scales = tuple(float(x) for x in scs[:n_cn]) if self.cn_multi else ()
        # controlnet_keep (lora_pipeline.py:421-428): per step, per net, 0.0 or 1.0
        self.cn_keep = controlnet_keep(S, control_guidance_start, control_guidance_end, max(1, n_cn))
        if len(self.cn_keep[0]) != max(1, n_cn):
            raise ValueError(f"control_guidance_start / _end must be scalars or hold one entry per ControlNet ({max(1, n_cn)})")
        self.shard = shard = concept_shard if (concept_shard is not None and concept_shard.world > 1) else None
        if shard is not None and stochastic:
            raise L.OmgHipError("concept_shard with a stochastic step (Euler-ancestral, DDIM eta > 0) is not built: the ranks would have to agree "
                                "on the noise; run the unsharded call")
        self.has_cb = bool(callback or callback_on_step_end)
        if self.has_cb:
            if shard is not None:
                raise L.OmgHipError("callbacks with concept_shard are not built: every rank would have to run the same callback")
            bad = [k for k in callback_on_step_end_tensor_inputs if k not in _CALLBACK_TENSORS]
            if bad:
                raise ValueError(f"callback_on_step_end_tensor_inputs {bad}: only {list(_CALLBACK_TENSORS)} exist (lora_pipeline.py:165)")
            if callback and (callback_steps is None or int(callback_steps) <= 0):
                raise ValueError("callback needs a positive callback_steps")
            dedup, stage_cache, drop_unc0 = False, False, False
        if self.cn_multi:
            if shard is not None:
                raise L.OmgHipError("concept_shard with a list of ControlNets / guess_mode is not built: run the unsharded call")
            dedup, stage_cache, drop_unc0 = False, False, False        # the general ControlNet path runs the full batch
        ctl_exact = not has_controller or bool(pure_controller)
        # a stochastic step gives the two samples of a request different noise from step 0: they are never the same computation
        self.twin = bool(dedup) and shard is None and not stochastic and ctl_exact
        self.cn_image_rows = cn_image_shapes[0][0] if self.use_cn else None
        if self.use_cn and self.cn_image_rows not in (1, n):
            # one conditioning image per MAIN ROW (4n): the two samples of a request may differ, and the 2n-row twin batch would not divide it
            # (ADVICE r3); the cache key and drop_unc0's compact rows address images per REQUEST — not built for that layout (the full batch
            # handles it); neither is used instead of being keyed / indexed wrongly
            self.twin, stage_cache, drop_unc0 = False, False, False
        self.fuse_possible = fuse_possible = stage == 2 and Ka > 0 and S > fusion_start + 1
        self.nm, self.ncn = 4 * n, 2 * Ka * n                       # rows of the main block / the concept block
        self.nb = self.nm + (self.ncn if fuse_possible else 0)
        if fuse_possible and not has_concept_models:
            raise ValueError("stage 2 needs concept_models")
        # ---- LoRA slots.  Concept passes: set_adapters(lora) or set_adapters([lora, "style"], [0.7, 0.5]) (lora_pipeline.py:588-591).
        # MAIN pass: inference_lora.py:162-164 loads the style LoRA into the main pipe as well, and the main UNet is called with
        # cross_attention_kwargs={"scale": 0.8} (:546-566), so with styleL every main sample runs with adapter "style" at PEFT
        # weight 1.0 x scale — one more slot of the same bank, selected for the main rows in plain AND fused steps.
        # LoRA scale: the concept UNet is always called with cross_attention_kwargs={'scale': 0.8} (hard-coded, :592-598); the main UNet
        # (style slot) with the caller's cross_attention_kwargs (:546-566; PEFT's default scale is 1.0)
        self.main_scale, self.concept_adapter_scale = float(main_scale), float(concept_adapter_scale)
        # InstantID's concepts are identities (IP-Adapter tokens + IdentityNet), not LoRA adapters: its `lora_list` only counts them
        self.main_adapters = main_adapters = [(str(a), float(w)) for a, w in (main_adapters or ())] or ([("style", 1.0)] if styleL else [])
        self.concept_adapters = concept_adapters = [(str(a), float(w)) for a, w in (concept_adapters or ())]
        if concept_lora and concept_adapters:
            raise ValueError("concept_adapters is the InstantID flow's 'whatever is active' rule; the LoRA flow selects adapters per concept (lora_list)")
        self.use_bank = use_bank = bank_adapters is not None and bool(concept_lora or concept_adapters or main_adapters)
        combos = []
        if fuse_possible and concept_lora:
            combos = [((self.lora_list[c], 0.7), ("style", 0.5)) if styleL else ((self.lora_list[c], 1.0),) for c in self.active]
        scales = [CONCEPT_LORA_SCALE] * len(combos)
        if fuse_possible and concept_adapters:              # one combination for every concept row
            combos, scales = [tuple(concept_adapters)], [self.concept_adapter_scale]
        self.main_slot = -1
        if main_adapters:
            if not use_bank or any(a not in bank_adapters for a, _ in main_adapters):
                raise ValueError(f"adapters {[a for a, _ in main_adapters]} on the main pass need concept_models with a LoraBank holding them"
                                 + (" (styleL=True: the adapter named 'style')" if styleL else ""))
            self.main_slot = len(combos)
            combos = combos + [tuple(main_adapters)]
            scales.append(self.main_scale)
        if concept_adapters and (not use_bank or any(a not in bank_adapters for a, _ in concept_adapters)):
            raise ValueError(f"concept_adapters {[a for a, _ in concept_adapters]} are not in concept_models' LoraBank")
        self.combos, self.scales, self.slots = combos, scales, []
        if fuse_possible:
            if not use_bank or not (concept_lora or concept_adapters):
                self.slots = [-1] * self.ncn
            elif concept_adapters:
                self.slots = [0] * self.ncn
            else:
                self.slots = [s for _ in range(n) for s in range(Ka) for _ in range(2)]
        self.merged = merged = use_bank and (lora_mode if combos else bank_mode) == "merged"      # the caller builds the bank for `combos` in `lora_mode`
        self.batched = batched = fuse_possible and (not use_bank or merged) and shared
        if use_graph and not (not use_bank or merged) and (fuse_possible or self.main_slot >= 0):
            raise L.OmgHipError("use_graph needs lora_mode='merged' (segment-mode K/V projections are not pointer-stable)")
        self.use_idn = use_idn = has_identitynet and fuse_possible
        if use_idn and not batched:
            raise L.OmgHipError("identitynet runs in the batched mode only: merged / no LoRA, and concept_models built on the pipeline's own "
                                "UNet (omg_amd.compat's from_pretrained shares it between the main and the concept pipe)")
        if shard is not None and ((fuse_possible and not batched) or use_idn or not ctl_exact):
            raise L.OmgHipError("concept_shard needs the batched step (merged / no LoRA on one shared UNet), a pure-replacement controller and no IdentityNet")
        self.stage_cache = bool(stage_cache) and shard is None and S > fusion_start + 1
        self.drop_unc0 = bool(drop_unc0) and batched and not use_idn and ctl_exact

    def replace(self, **fields) -> "CallPlan":
        q = CallPlan.__new__(CallPlan)
        vars(q).update(vars(self), **fields)
        return q

    def with_drop0(self) -> "CallPlan":
        """The resumed call without ``unc0``: the compact-row machinery of the concept shard, on ONE rank — main units of three rows
        [unc1, cond0, cond1]."""
        return self.replace(drop0=True, shard=parallel.ConceptShard(rank=0, world=1), twin=False)

    def engine_key(self, shapes_and_ids: tuple = ()) -> tuple:
        """``shapes_and_ids``: what the plan does not decide on — dtype, the shapes of the call's tensors, id() of the models and the controller"""
        return (self.n, self.S, self.K, self.active, self.fuse_possible, self.fusion_start, self.scheduler_name, self.guidance_scale, self.batched,
                self.styleL, tuple(self.main_adapters), tuple(self.concept_adapters), self.concept_adapter_scale, self.main_scale, self.lora_list,
                self.cn_scale, self.idn_scale, self.twin, (self.shard.rank, self.shard.world) if self.shard is not None else None, self.drop0,
                self.stochastic, None if not self.cn_multi else (self.cn_image_shapes, self.cn_guess)) + shapes_and_ids



def all_step_embeddings(net, ts: torch.Tensor, text: torch.Tensor, tids: torch.Tensor) -> torch.Tensor:
    """emb[i] for every step in one batched pass: (S, rows, 4*C0).  Depends only on (t_i, pooled text, time ids) and on the embedding
    layers of ``net``, the model that will consume it: the UNet (the concept pipe's, when it is not the main one), a ControlNet, the IdentityNet."""
    S, rows = ts.numel(), text.shape[0]
    t_all = ts.reshape(S, 1).expand(S, rows).reshape(-1).contiguous()
    return net.time_embed(t_all, S * rows, text.repeat(S, 1), tids.repeat(S, 1)).view(S, rows, -1)


def _fill(dst: torch.Tensor, srcs: Sequence[torch.Tensor], dim: int, rows: Optional[torch.Tensor] = None) -> None:
    """dst <- the tensors ``srcs`` laid end to end along ``dim`` (of each its ``rows`` along ``dim`` only), in place, one copy each"""
    srcs = [s if rows is None else s.index_select(dim, rows) for s in srcs]
    for d, s in zip(dst.split([s.shape[dim] for s in srcs], dim), srcs):
        d.copy_(s)


class RowSet:
    """One set of rows a step runs a UNet forward over — the main rows, the batched main + concept rows, the twin rows of ``dedup``, the
    compact rows of a shard rank or of ``drop_unc0``.  Members: model input ``x`` and output ``y``, text states ``ehs``, the per-step embedding
    table ``emb`` with its current-step row buffer ``emb_cur``, the LoRA ``state``, the keywords ``kw`` of the forward (``omg_images`` = ``n_images``,
    ``omg_main_batch`` = ``main_batch``), and for a ControlNet on the set's first ``n_main`` rows its embedding table ``cn_emb`` with ``cn_emb_cur``
    and its conditioning image ``cn_image``.  Static buffers, allocated once and refilled in place by :meth:`load`: captured graphs point at them."""

    def __init__(self, rows: int, n_images: int, main_batch: int = 4, *, chw, ctx, S, D, dtype, device, x=None, y=None, n_main: int = 0,
                 cn_image=None, cn_image_shape=None):
        """``x`` / ``y``: views of a wider buffer this set shares; ``cn_image``: another set's image to share, ``cn_image_shape``: one of its own"""
        self.rows, self.n_images, self.main_batch, self.n_main = rows, n_images, main_batch, n_main
        self.x = torch.empty((rows,) + chw, dtype=dtype, device=device) if x is None else x
        self.y = torch.empty((rows,) + chw, dtype=torch.float32, device=device) if y is None else y
        self.ehs = torch.empty((rows,) + ctx, dtype=dtype, device=device)
        self.emb = torch.empty((S, rows, D), dtype=dtype, device=device)
        self.emb_cur = torch.empty((rows, D), dtype=dtype, device=device)
        self.cn_emb = self.cn_emb_cur = self.cn_image = None
        if cn_image is not None or cn_image_shape is not None:
            self.cn_emb = torch.empty((S, n_main, D), dtype=dtype, device=device)
            self.cn_emb_cur = torch.empty((n_main, D), dtype=dtype, device=device)
            self.cn_image = torch.empty(cn_image_shape, dtype=torch.float32, device=device) if cn_image is None else cn_image
            self.cn_x, self.cn_ehs = self.x[:n_main], self.ehs[:n_main]

    def load(self, ehs, emb, state, kw: dict, rows: Optional[torch.Tensor] = None, cn_emb=None, cn_image=None) -> None:
        """This call's text states and embedding tables (``ehs`` / ``emb``: lists, laid end to end; with ``rows``: those rows of the source),
        LoRA state and keywords; ``cn_emb``: the table the ControlNet's is taken from likewise, ``cn_image``: the image, unless it is shared."""
        _fill(self.ehs, ehs, 0, rows)
        _fill(self.emb, emb, 1, rows)
        self.state, self.kw = state, dict(kw, omg_main_batch=self.main_batch, omg_images=self.n_images)
        if self.cn_emb is not None:
            _fill(self.cn_emb, [cn_emb], 1, None if rows is None else rows[: self.n_main])
            if cn_image is not None:
                self.cn_image.copy_(cn_image)

    def refresh(self, eng: "StepEngine") -> None:
        """cached cross-attention K/V (and ControlNet conditioning features) must be refreshed eagerly: replayed graphs read the stored tensors"""
        eng.unet.refresh_cross_kv(self.ehs, self.state)
        if self.cn_emb is not None:
            eng.controlnet.refresh_cross_kv(self.cn_ehs)
            eng.controlnet.cond_features(self.cn_image)

    def control(self, eng: "StepEngine") -> list:
        """The ControlNet's residuals for the set's main rows (lora_pipeline.py:519-536); scale 0 = outside its guidance window: not run"""
        if self.cn_emb is None or eng.cur_cn == 0.0:
            return []
        ops.gather_step(self.cn_emb, eng.step_idx, self.cn_emb_cur)
        d_, m_ = eng.controlnet(self.cn_x, None, encoder_hidden_states=self.cn_ehs, controlnet_cond=self.cn_image,
                                conditioning_scale=eng.cur_cn, emb=self.cn_emb_cur)
        return [(0, self.n_main, d_, m_)]

    def forward(self, eng: "StepEngine", kw: dict, residuals: list) -> None:
        """y = UNet(x) at the step the DEVICE counter selects, under the set's LoRA state.  ``residuals``: what the caller collected,
        :meth:`control` 's among them."""
        if residuals:
            kw["omg_residuals"] = residuals
        ops.gather_step(self.emb, eng.step_idx, self.emb_cur)
        eng.unet.set_lora_state(self.state)
        try:
            eng.unet(self.x, None, encoder_hidden_states=self.ehs, cross_attention_kwargs=kw, emb=self.emb_cur, out=self.y)
        finally:
            eng.unet.set_lora_state(None)


class StepEngine:
    """The persistent state of one call shape (:meth:`CallPlan.engine_key`): static buffers, the row sets of its steps and the captured
    step graphs of every regime.  Built once from the plan, :meth:`load` ed with every call's inputs (device-to-device copies; graphs
    keep their pointers), then :meth:`run_step` per step."""

    def __init__(self, unet, plan: CallPlan, t, controller, controlnet, identitynet, cn_nets, concept_models):
        """``t``: the tensors of the first call (``generate_many`` gathers them), for their shapes.  The engine holds no reference to the
        pipeline that owns it: an engine in a reference cycle would be freed, with its captured graphs, whenever the collector runs — a capture included."""
        p, dev, dt = plan, unet.device, unet.dtype
        n, S, nm, ncn, nb, D, ctx = p.n, p.S, p.nm, p.ncn, p.nb, t.emb_main.shape[-1], tuple(t.ehs.shape[1:])
        self.chw = chw = tuple(t.lats[0].shape[1:])
        self.unet, self.plan = unet, plan
        self.controller, self.controlnet, self.identitynet, self.cn_nets = controller, controlnet, identitynet, cn_nets
        # the key holds id()s: keep the objects alive so that an id cannot be recycled for a different object
        self.refs = (controller, controlnet, identitynet, concept_models, cn_nets)
        self.graphs, self.warmed, self.pool = {}, set(), None
        self.coef = torch.empty_like(t.coef)               # the engine's OWN buffer: the scheduler's cached table is shared and read-only
        self.epoch = pointer_epoch()
        self.lat = torch.empty((2 * n,) + chw, dtype=torch.float32, device=dev)
        self.xin = torch.empty((nb,) + chw, dtype=dt, device=dev)
        # drop0: the rows of `unc0` are never written — zeros, so that the step kernel's (discarded) update of the base sample stays finite
        self.nout = (torch.zeros if p.drop0 else torch.empty)((nb,) + chw, dtype=torch.float32, device=dev)
        self.step_idx = torch.zeros(1, dtype=torch.int32, device=dev)
        # request j's fusion + CFG + scheduler update + next model input: the one-step linear table (DDIM, Euler) or the multistep one with
        # the request's rows of the history buffer (DPM-Solver++), or the one-step table plus the request's noise (Euler-ancestral, DDIM eta > 0)
        self.step_op, extra = ops.fuse_cfg_step, [()] * n
        if p.multistep:      # the previous step's data prediction of every sample (captured graphs point at it); order-1 steps do not read it
            self.x0_hist = torch.zeros((2 * n,) + chw, dtype=torch.float32, device=dev)
            self.step_op, extra = ops.fuse_cfg_step_ms, [(self.x0_hist[2 * j: 2 * j + 2],) for j in range(n)]
        if p.stochastic:     # every step's noise of every sample (captured graphs point at it), refilled in place per call
            self.z = torch.empty((S, 2 * n) + chw, dtype=torch.float32, device=dev)
            self.step_op, extra = ops.fuse_cfg_step_noise, [(self.z[:, 2 * j: 2 * j + 2],) for j in range(n)]
        # per request: its rows of the noise prediction, the latents and the model input, what its step kernel reads besides them, and (per
        # concept, None without a mask) its concept pairs' rows of the prediction
        self.per_request = [(self.nout[4 * j: 4 * j + 4], self.lat[2 * j: 2 * j + 2], self.xin[4 * j: 4 * j + 4], extra[j]) for j in range(n)]
        self.no_regions = [None] * p.K
        row = {c: nm + 2 * jj for jj, c in enumerate(p.active)} if p.fuse_possible else {}      # request 0's; request j's: 2 Ka j further on
        self.regions = [[self.nout[row[c] + 2 * p.Ka * j: row[c] + 2 * p.Ka * j + 2] if c in row else None for c in range(p.K)] for j in range(n)]
        self.masks = [[torch.empty(t.mshape, dtype=torch.float32, device=dev) if c in p.active else None for c in range(p.K)] for _ in range(n)]
        shape = dict(chw=chw, ctx=ctx, S=S, D=D, dtype=dt, device=dev)
        self.main = RowSet(nm, n, x=self.xin[:nm], y=self.nout[:nm], n_main=nm, cn_image_shape=p.cn_image_shapes[0] if p.use_cn else None, **shape)
        if p.fuse_possible:      # the concept rows as a forward of their own (concept_models.unet_batched: un-batched fused steps)
            self.conc = RowSet(ncn, n, x=self.xin[nm:], y=self.nout[nm:], **shape)
        if p.batched:
            self.all = RowSet(nb, n, x=self.xin, y=self.nout, n_main=nm, **shape)
        if p.twin:      # compact rows [unc, cond] per request for the steps in which the two samples coincide
            self.twin = RowSet(2 * n, n, n_main=2 * n, cn_image=self.main.cn_image, **shape)
        if p.cn_multi:
            rows_cn = 2 * n if p.cn_guess else nm
            self.cnm_image = [torch.empty(s, dtype=torch.float32, device=dev) for s in p.cn_image_shapes]
            self.cnm_emb = [torch.empty((S, rows_cn, D), dtype=dt, device=dev) for _ in cn_nets]
            self.cnm_emb_cur = [torch.empty((rows_cn, D), dtype=dt, device=dev) for _ in cn_nets]
            if p.cn_guess:      # the conditional rows [cond0, cond1] of every request, compact
                self.cnm_x = torch.empty((rows_cn,) + chw, dtype=dt, device=dev)
                self.cnm_ehs = torch.empty((rows_cn,) + ctx, dtype=dt, device=dev)
        if p.use_idn:
            self.ip_all = torch.empty((ncn,) + tuple(t.ip_l[0].shape[1:]), dtype=dt, device=dev)
            self.kps_all = torch.empty((n,) + tuple(t.kps_l[0].shape[1:]), dtype=torch.float32, device=dev)
            self.idn_emb = torch.empty((S, ncn, D), dtype=dt, device=dev)
            self.idn_emb_cur = torch.empty((ncn, D), dtype=dt, device=dev)
        if p.shard is not None:      # per regime (plain / fused): this rank's units, its compact local batch and every rank's row map
            self.sh = {fz: self._shard_rows(fz, shape) for fz in ((True,) if p.drop0 else (False, True) if p.fuse_possible else (False,))}

    def _shard_rows(self, fused: bool, shape: dict) -> RowSet:
        """The compact rows of this rank in a plain / fused step, with what the exchange needs: ``mains`` / ``concs`` (its units), ``src``
        (the rows of the full model input its ``x`` is gathered from), ``dsts`` / ``counts`` (per rank, where its predictions go in the
        full batch), ``ybuf`` (the equally sized exchange buffer ``y`` is the head of)."""
        p, n, Ka, nm, dev = self.plan, self.plan.n, self.plan.Ka, self.plan.nm, self.lat.device
        rank = p.shard.rank
        if p.drop0:      # every unit on this one rank; a main unit is rows 1..3 of the request's block (`unc0` is not computed)
            per_rank = [(list(range(n)), [(j, c) for j in range(n) for c in range(Ka)])]
            mrows = [4 * j + r for j in range(n) for r in (1, 2, 3)]
            rows = [(mrows + [4 * j + 3 for j, _ in per_rank[0][1] for _ in range(2)],
                     mrows + [nm + 2 * Ka * j + 2 * c + r for j, c in per_rank[0][1] for r in range(2)])]
        else:
            per_rank = parallel.assign_units(n, Ka, fused, p.shard.world)
            rows = parallel.unit_rows(per_rank, n, Ka)
        mains, concs = per_rank[rank]
        src, counts = rows[rank][0], [len(r[1]) for r in rows]
        n_main = (3 if p.drop0 else 4) * len(mains)      # drop0: [unc1, cond0, cond1] — cond1 borrows Q, K of cond0 = row 1 of the block
        ybuf = torch.zeros((max(counts),) + self.chw, dtype=torch.float32, device=dev)
        image = (len(mains) if p.cn_image_rows != 1 else 1,) + p.cn_image_shapes[0][1:] if p.use_cn and n_main else None
        sh = RowSet(len(src), len(mains), 3 if p.drop0 else 4, y=ybuf[: len(src)], n_main=n_main, cn_image_shape=image, **shape)
        sh.mains, sh.concs, sh.counts, sh.ybuf = mains, concs, counts, ybuf
        sh.src = torch.tensor(src, dtype=torch.long, device=dev)
        sh.dsts = [torch.tensor(r[1], dtype=torch.long, device=dev) for r in rows]
        return sh

    def lora_state(self, main_rows: int, concept_slots: Sequence[int] = ()) -> Optional[LoraState]:
        """``main_rows`` rows on the main pass's slot (base weights, or the style slot / ``main_adapters``), then one row per entry of
        ``concept_slots`` (-1: base weights).  None: base weights throughout."""
        p = self.plan
        if not p.use_bank or (p.main_slot < 0 and not concept_slots):
            return None
        if p.merged:
            return self.concept_models.lora_state([p.main_slot + 1] * main_rows + [s + 1 for s in concept_slots], merged=True)
        return self.concept_models.lora_state([p.main_slot] * main_rows, merged=False)

    def load(self, plan: CallPlan, t, resume: StageCache.Resume, sched, concept_models, cross_attention_kwargs, use_graph: bool) -> None:
        """Load a call's inputs into the static buffers; ``t``: its tensors as ``generate_many`` gathered them."""
        p = self.plan = plan
        self.concept_models, self.use_graph, self.first, self.base_traj = concept_models, use_graph, resume.first, resume.base_traj
        n, nm, dev, ctl = p.n, p.nm, self.lat.device, self.controller
        self.lat.copy_(torch.cat(t.lats, dim=0))
        # t.coef, per call: the key holds the scheduler's class and step count, not its configuration — a re-configured scheduler must
        self.coef.copy_(t.coef)                            # not meet a cached table.  In place: captured graphs keep the pointer
        self.step_idx.zero_()
        if p.stochastic:
            for j in range(n):
                self.z[:, 2 * j: 2 * j + 2].copy_(t.z_l[j])
        for j in range(n):
            for c in p.active:
                self.masks[j][c].copy_(t.masks_l[j][c])
        if resume.latents is not None:                                   # resume (decided in front of the engine)
            self.lat.copy_(torch.cat([h.to(dev) for h in resume.latents], dim=0))
            if p.multistep:
                self.x0_hist.copy_(torch.cat([h.to(dev) for h in resume.history], dim=0))
            self.step_idx.fill_(self.first)
            if ctl is not None:
                ctl.cur_step = self.first                                # the host-side counters the skipped steps would have ticked
        cin0 = sched.cin0(dev) if self.first == 0 else torch.tensor([sched.cin[self.first]], dtype=torch.float32, device=dev)
        for nout_j, lat_j, xin_j, _ in self.per_request:
            ops.scale_model_input(lat_j, cin0, xin_j)
        main_kw = dict(cross_attention_kwargs or {})
        main_kw.pop("scale", None)
        # main-only forwards (plain steps; the main half of un-batched fused steps): base weights, or the style slot
        self.main.load([t.ehs], [t.emb_main], self.lora_state(nm), main_kw,
                       cn_emb=all_step_embeddings(self.controlnet, t.ts, t.text, t.tids_main) if p.use_cn else None,
                       cn_image=t.cn_image.to(device=dev, dtype=torch.float32) if p.use_cn else None)
        if p.fuse_possible:
            self.conc.load([t.c_ehs], [t.emb_conc], None, main_kw)
        if p.batched:
            self.all.load([t.ehs, t.c_ehs], [t.emb_main, t.emb_conc], self.lora_state(nm, p.slots), main_kw)
        if p.cn_multi:
            cond_rows = torch.tensor([4 * j + r for j in range(n) for r in (2, 3)], dtype=torch.long, device=dev)
            text_cn, tids_cn = t.text, t.tids_main
            if p.cn_guess:      # add_text_embeds.chunk(2)[1] / add_time_ids.chunk(2)[1] / prompt_embeds.chunk(2)[1] (lora_pipeline.py:497-503)
                text_cn, tids_cn = text_cn.index_select(0, cond_rows), tids_cn.index_select(0, cond_rows)
                self.cnm_ehs.copy_(t.ehs.index_select(0, cond_rows))
            for k_, net in enumerate(self.cn_nets):
                self.cnm_image[k_].copy_(t.cn_images[k_].to(device=dev, dtype=torch.float32))
                self.cnm_emb[k_].copy_(all_step_embeddings(net, t.ts, text_cn, tids_cn))
                if use_graph:
                    net.refresh_cross_kv(self.cnm_ehs if p.cn_guess else self.main.ehs)
                    net.cond_features(self.cnm_image[k_])
        if p.use_idn:
            self.ip_all.copy_(torch.cat(t.ip_l, dim=0))
            self.kps_all.copy_(torch.cat(t.kps_l, dim=0))
            self.idn_emb.copy_(all_step_embeddings(self.identitynet, t.ts, t.ctext, t.tids_conc))
        if p.twin:
            rows2 = torch.tensor([4 * j + r for j in range(n) for r in (0, 2)], dtype=torch.long, device=dev)      # unc0, cond0 of each request
            self.twin.load([t.ehs], [t.emb_main], self.lora_state(2 * n), dict(main_kw, omg_twin=True), rows=rows2, cn_emb=self.main.cn_emb)
        if p.shard is not None:
            for fz, sh in self.sh.items():
                if not sh.rows:
                    continue
                src = self.all if fz else self.main
                image = None if sh.cn_image is None else self.main.cn_image if p.cn_image_rows == 1 else self.main.cn_image[sh.mains]
                sh.load([src.ehs], [src.emb], self.lora_state(sh.n_main, [jj for _, jj in sh.concs for _ in range(2)]), main_kw,
                        rows=sh.dsts[p.shard.rank], cn_emb=self.main.cn_emb, cn_image=image)
                if use_graph:
                    sh.refresh(self)
        elif use_graph:
            if p.twin:
                self.twin.refresh(self)
            self.main.refresh(self)
            if p.batched:
                self.all.refresh(self)
            if p.use_idn:
                self.identitynet.refresh_cross_kv(self.ip_all)
                self.identitynet.cond_features(self.kps_all)
                self.unet.refresh_ip_kv(self.ip_all)      # the UNet's own image-prompt K / V^T of the concept samples
        # the conditioning scales of the CURRENT step (host floats baked into the zero convolutions' epilogues, hence part of the graph regime):
        # scale * controlnet_keep[i] (lora_pipeline.py:511-517; instantid_pipeline.py:566-578: the one window scales the IdentityNet and the t2i net)
        self.cur_cn, self.cur_idn, self.cur_multi = p.cn_scale, p.idn_scale, ()
        # the general prompt-to-prompt edit reads alpha[cur_step] on the device: cur_step == step_idx + offset from here to the end of the
        # call (a resumed call set cur_step = first above; replays advance the host counter by one per step, as step_idx advances)
        self.ctl_step_offset = 0
        if hasattr(ctl, "bind_step_counter"):
            self.ctl_step_offset = ctl.cur_step - self.first
            ctl.bind_step_counter(self.step_idx, self.ctl_step_offset)

    def set_step_scales(self, i: int) -> tuple:
        p, keep = self.plan, self.plan.cn_keep[i]
        self.cur_cn, self.cur_idn = p.cn_scale * keep[0], p.idn_scale * keep[0]
        if p.cn_multi:
            self.cur_multi = tuple(sc * keep[k_] for k_, sc in enumerate(p.cn_scales))
        return (self.cur_cn if p.use_cn else None, self.cur_idn if p.use_idn else None, self.cur_multi)

    def multi_residuals(self) -> list:
        """The general ControlNet block of a step: every net of the list on the main rows (guess_mode: on the conditional rows only), residuals
        summed in list order like MultiControlNetModel.forward — first the nets' residuals among themselves, then onto the skips — and, in
        guess_mode, no residual for the unconditional rows (lora_pipeline.py:531-535 concatenates zeros)."""
        p, n, guess = self.plan, self.plan.n, self.plan.cn_guess
        sum_d = sum_m = None
        if guess:
            self.cnm_x.view((n, 2) + self.chw).copy_(self.main.x.view((n, 4) + self.chw)[:, 2:4])
        for k_, net in enumerate(self.cn_nets):
            sc = self.cur_multi[k_]
            if sc == 0.0:
                continue
            ops.gather_step(self.cnm_emb[k_], self.step_idx, self.cnm_emb_cur[k_])
            d_, m_ = net(self.cnm_x if guess else self.main.x, None, encoder_hidden_states=self.cnm_ehs if guess else self.main.ehs,
                         controlnet_cond=self.cnm_image[k_], conditioning_scale=sc, emb=self.cnm_emb_cur[k_], guess_mode=guess)
            if sum_d is None:
                sum_d, sum_m = d_, m_
            else:
                for a_, b_ in zip(sum_d + [sum_m], d_ + [m_]):
                    ops.add_(a_.permute(0, 2, 3, 1), b_.permute(0, 2, 3, 1))
        if sum_d is None:
            return []
        if not guess:
            return [(0, p.nm, sum_d, sum_m)]
        return [(4 * j + 2, 4 * j + 4, [d_[2 * j: 2 * j + 2] for d_ in sum_d], sum_m[2 * j: 2 * j + 2]) for j in range(n)]

    def fill_region_inputs(self) -> None:
        p = self.plan
        for j in range(p.n):                              # latent_model_input[3:4] duplicated (:583-585), per request
            r0 = p.nm + 2 * p.Ka * j
            self.xin[r0: r0 + 2 * p.Ka].copy_(self.xin[4 * j + 3: 4 * j + 4].expand(2 * p.Ka, -1, -1, -1))

    def twin_body(self) -> None:
        """A step in which samples 0 and 1 of every request are still identical: one [unc, cond] forward per request, the noise
        prediction written to both samples, then the ordinary CFG + scheduler step on all four rows."""
        n, chw, tw = self.plan.n, self.chw, self.twin
        tw.x.view((n, 2) + chw).copy_(self.main.x.view((n, 2, 2) + chw)[:, :, 0])
        tw.forward(self, dict(tw.kw), tw.control(self))
        self.main.y.view((n, 2, 2) + chw).copy_(tw.y.view((n, 2, 1) + chw).expand((n, 2, 2) + chw))
        self.finish(False)

    def step_body(self, fused: bool, twin_step: bool = False) -> None:
        """One denoising iteration; every per-step quantity is selected by the DEVICE step counter."""
        if twin_step:
            return self.twin_body()
        p = self.plan
        rs = self.all if fused and p.batched else self.main
        kw = dict(rs.kw)
        residuals = self.main.control(self)               # ControlNet on the main samples, whichever set they are forwarded in
        if p.cn_multi:
            residuals.extend(self.multi_residuals())
        if fused and p.batched:
            self.fill_region_inputs()
            if p.use_idn:                                 # IdentityNet on the concept samples (instantid_pipeline.py:638-648)
                if self.cur_idn != 0.0:
                    ops.gather_step(self.idn_emb, self.step_idx, self.idn_emb_cur)
                    d_, m_ = self.identitynet(self.xin[p.nm:], None, encoder_hidden_states=self.ip_all, controlnet_cond=self.kps_all,
                                              conditioning_scale=self.cur_idn, emb=self.idn_emb_cur)
                    residuals.append((p.nm, p.nb, d_, m_))
                kw["omg_ip_tokens"], kw["omg_ip_rows"] = self.ip_all, p.nm
        rs.forward(self, kw, residuals)
        if fused and not p.batched:
            self.fill_region_inputs()
            cs = self.conc
            ops.gather_step(cs.emb, self.step_idx, cs.emb_cur)
            self.concept_models.unet_batched(cs.x, None, cs.ehs, p.slots, emb=cs.emb_cur, out=cs.y)
        self.finish(fused)

    def finish(self, fused: bool) -> None:
        """Region fusion + CFG + scheduler update + next model input of every request (one launch each)."""
        last = self.plan.n - 1
        for j in range(last + 1):
            self.scheduler_step(j, fuse=fused, region_preds=self.regions[j] if fused else self.no_regions,
                                masks=self.masks[j] if fused else self.no_regions, advance=(j == last))

    def scheduler_step(self, j: int, **kw) -> None:
        nout_j, lat_j, xin_j, extra = self.per_request[j]
        self.step_op(nout_j, lat_j, self.coef, *extra, self.step_idx, guidance_scale=self.plan.guidance_scale, model_input_next=xin_j, **kw)

    def shard_forward(self, fused: bool, _tw: bool = False) -> None:
        """This rank's units of the step: main blocks first, then concept pairs, as one compact batch."""
        sh = self.sh[fused]
        sh.x.copy_(self.main.x.index_select(0, sh.src))
        sh.forward(self, dict(sh.kw), sh.control(self))

    def run_step(self, i: int) -> None:
        p = self.plan
        fused = p.fuse_possible and i > p.fusion_start
        scales_i = self.set_step_scales(i)
        if p.shard is None:
            # twin: the samples part ways at the first fused step (stage 1: never)
            return self.run_forward(self.step_body, fused, p.twin and not fused, (fused, scales_i))
        sh = self.sh[fused]
        if sh.rows:
            self.run_forward(self.shard_forward, fused, False, ("shard", fused, scales_i))
        elif self.controller is not None:
            self.controller.cur_step += 1          # no unit of this step is ours: only the host-side step counter moves
        p.shard.exchange(sh.ybuf, sh.counts, sh.dsts, self.nout)
        self.finish(fused)
        if p.drop0:      # the base samples were not computed: their latents and next model inputs are the stage-1 call's
            bl, bx = self.base_traj[i + 1]
            self.lat.view((p.n, 2) + self.chw)[:, 0].copy_(bl)
            if i + 1 < p.S:
                self.main.x.view((p.n, 4) + self.chw)[:, 2].copy_(bx)

    def run_forward(self, body: Callable, fused: bool, tw: bool, tag: tuple) -> None:
        """``body`` eagerly, or — ``use_graph`` — as the captured graph of its regime: eager on first sight, captured on the second, replayed after"""
        if not self.use_graph:
            body(fused, tw)
            return
        controller = self.controller
        if self.epoch != pointer_epoch():         # a weight image or cached K/V the graphs point at was freed or re-allocated
            self.graphs.clear()
            self.warmed.clear()
            self.pool = None                      # the pool dies with its last graph: a later capture must open a new one
            self.epoch = pointer_epoch()
        win = controller._self_window() if controller is not None and hasattr(controller, "_self_window") else None
        # the cross edit's kind at this step ("borrow" / "own" / "mixed": different launches); WITHIN a kind one graph serves every
        # step, because the edit's alpha row is selected on the device through the step counter bound in load() (+ its host offset)
        ck = (controller.cross_kind(), self.ctl_step_offset) if hasattr(controller, "cross_kind") else None
        regime = tag + (win, tw, ck)
        g = self.graphs.get(regime)
        if g is not None:
            g.replay()
            if controller is not None:
                controller.cur_step += 1          # the replayed graph does not run the host-side counters
            return
        if regime not in self.warmed:             # first step of a regime runs eagerly (lazy inits, caches)
            body(fused, tw)
            self.warmed.add(regime)
            return
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, pool=self.pool):
            body(fused, tw)                       # records the step; host counters tick as in eager mode
        if self.pool is None:
            self.pool = g.pool()
        self.graphs[regime] = g
        g.replay()


class LoraMultiConceptPipeline:
    """See the module docstring.  ``__call__`` keeps the reference's single-request signature; ``generate_many`` runs
    several independent requests in lock-step through ONE batched UNet forward per step (images are independent,
    SURVEY §8e) — same per-image arithmetic, larger GEMMs."""

    def __init__(self, unet, scheduler=None, encode_prompt: Optional[Callable] = None, vae_decode: Optional[Callable] = None):
        self.unet = unet
        self.scheduler = scheduler or DDIMScheduler()
        self.encode_prompt = encode_prompt
        self.vae_decode = vae_decode
        self.vae_scale_factor = 8
        self._engines: Dict[Tuple, StepEngine] = {}           # call shape -> static buffers + captured step graphs, LRU
        self.max_engines = 8                                   # a few hundred MB of buffers each (+ graph pools): raise for servers with many shapes
        self.engine_evictions = 0

    @property
    def _execution_device(self):
        return self.unet.device

    # ------------------------------------------------------------------ helpers
    def prepare_latents(self, batch, channels, height, width, dtype, device, generator, latents=None):
        """randn / vae_scale_factor, times init_noise_sigma (diffusers prepare_latents; lora_pipeline.py:397-406).
        ``latents=`` injects fixed noise (needed for CPU<->GPU seed parity)."""
        shape = (batch, channels, height // self.vae_scale_factor, width // self.vae_scale_factor)
        if latents is None:
            gen_dev = generator.device if generator is not None else device
            latents = torch.randn(shape, generator=generator, device=gen_dev, dtype=torch.float32).to(device)
        else:
            latents = latents.to(device=device, dtype=torch.float32)
            if tuple(latents.shape) != shape:
                raise ValueError(f"latents shape {tuple(latents.shape)} != {shape}")
        return latents * float(self.scheduler.init_noise_sigma)

    @staticmethod
    def _add_time_ids(original_size, crops, target_size, n, device):
        ids = list(original_size) + list(crops) + list(target_size)
        return torch.tensor([ids] * n, dtype=torch.float32, device=device)

    # ------------------------------------------------------------------ the reference's call signature
    @torch.no_grad()
    def __call__(self, prompt=None, prompt_2=None, image=None, height: Optional[int] = None, width: Optional[int] = None,
                 num_inference_steps: int = 50, guidance_scale: float = 5.0, negative_prompt=None, negative_prompt_2=None,
                 num_images_per_prompt: int = 1, eta: float = 0.0, generator=None, latents: Optional[torch.Tensor] = None,
                 prompt_embeds=None, negative_prompt_embeds=None, pooled_prompt_embeds=None, negative_pooled_prompt_embeds=None,
                 output_type: str = "pil", return_dict: bool = True, cross_attention_kwargs=None,
                 original_size=None, crops_coords_top_left=(0, 0), target_size=None,
                 controller=None, concept_models: Optional[ConceptModels] = None, stage: Optional[int] = None,
                 region_masks: Optional[Sequence[Optional[torch.Tensor]]] = None, lora_list: Optional[Sequence[str]] = None,
                 styleL: Optional[bool] = None, region_prompt_embeds: Optional[Sequence[Tuple[torch.Tensor, ...]]] = None,
                 use_graph: bool = False, trajectory: Optional[list] = None, fusion_start: int = FUSION_START,
                 lora_mode: str = "merged", dedup: bool = False, **kwargs):
        controlnet = kwargs.pop("controlnet", getattr(self, "controlnet", None))
        cn_scale = kwargs.pop("controlnet_conditioning_scale", 1.0)
        # round 6: implemented instead of refused (lora_pipeline.py:236-238; generate_many's docstring)
        guess_mode = bool(kwargs.pop("guess_mode", False))
        cg_start, cg_end = kwargs.pop("control_guidance_start", 0.0), kwargs.pop("control_guidance_end", 1.0)
        clip_skip = kwargs.pop("clip_skip", None)                                                   # lora_pipeline.py:245, :333
        neg_cond = (kwargs.pop("negative_original_size", None), kwargs.pop("negative_crops_coords_top_left", (0, 0)),
                    kwargs.pop("negative_target_size", None))                                       # :242-244, :459-466
        callbacks = dict(callback=kwargs.pop("callback", None), callback_steps=kwargs.pop("callback_steps", None),      # :256-257, :629-632
                         callback_on_step_end=kwargs.pop("callback_on_step_end", None),                                  # :246, :617-626
                         callback_on_step_end_tensor_inputs=kwargs.pop("callback_on_step_end_tensor_inputs", ("latents",)))
        stage_cache, drop_unc0 = kwargs.pop("stage_cache", None), kwargs.pop("drop_unc0", False)
        given = {k: kwargs.pop(k) for k in list(kwargs) if k in _UNIMPLEMENTED}
        given.update(num_images_per_prompt=num_images_per_prompt)
        refuse_unimplemented(given, kwargs, "LoraMultiConceptPipeline.__call__")
        n_nets = len(controlnet.nets) if hasattr(controlnet, "nets") else len(controlnet) if isinstance(controlnet, (list, tuple)) else 1
        if n_nets == 1:
            if isinstance(cn_scale, (list, tuple)):      # lora_pipeline.py:513-515: one ControlNet takes the first entry
                cn_scale = cn_scale[0]
            if isinstance(image, (list, tuple)):         # a one-element list reached generate_many un-unwrapped
                if len(image) != 1:
                    raise L.OmgHipError(f"{len(image)} ControlNet images for one ControlNet: pass one image, or a list of ControlNets (lora_pipeline.py:175-176)")
                image = image[0]
        elif image is not None and (not isinstance(image, (list, tuple)) or len(image) != n_nets):
            raise L.OmgHipError(f"{n_nets} ControlNets need a list of {n_nets} conditioning images (lora_pipeline.py:366-383)")
        if image is not None and controlnet is None:
            raise L.OmgHipError("image= needs a ControlNet: pass controlnet=omg_amd.controlnet.ControlNetModel(...)")
        lora_list = list(lora_list or [])
        # ---- 3. prompt embeddings (global on the main pipe; per-region on the concept pipe)
        if prompt_embeds is None:
            if self.encode_prompt is None:
                raise L.OmgHipError("no text encoders attached: pass prompt_embeds=/pooled_prompt_embeds= (and region_prompt_embeds=) or "
                                    "construct the pipeline with encode_prompt=omg_amd.text_encoder.make_encode_prompt(...)")
            # global prompt on the main pipe (its text encoders carry the style LoRA when one is loaded, inference_lora.py:162-164),
            # region prompts on the concept pipe with the concept's adapters active (lora_pipeline.py:315-347); both with
            # lora_scale = cross_attention_kwargs["scale"]
            te_scale = (cross_attention_kwargs or {}).get("scale", None)
            global_prompt, regions = prompt[0], prompt[1]
            # prompt_2 / negative_prompt_2 / clip_skip act on the GLOBAL prompt only: the region prompts are encoded without them (lora_pipeline.py:340-342)
            extra = {k: v for k, v in (("prompt_2", prompt_2), ("negative_prompt_2", negative_prompt_2), ("clip_skip", clip_skip)) if v is not None}
            prompt_embeds, negative_prompt_embeds, pooled_prompt_embeds, negative_pooled_prompt_embeds = self.encode_prompt(
                global_prompt, negative_prompt, [("style", 1.0)] if styleL else None, te_scale, **extra)
            region_prompt_embeds = []
            for lora_param, (rp, rn) in zip(lora_list, [(r[0], r[1]) for r in regions]):
                if hasattr(concept_models, "encode_prompt"):      # the reference's literal sequence (lora_pipeline.py:337-343)
                    if styleL:
                        concept_models.set_adapters([lora_param, "style"], adapter_weights=[0.7, 0.5])
                    else:
                        concept_models.set_adapters(lora_param)
                    pe, ne, pp, npp = concept_models.encode_prompt(prompt=rp, device=concept_models._execution_device, num_images_per_prompt=1,
                                                                   do_classifier_free_guidance=True, negative_prompt=rn, lora_scale=te_scale)
                else:
                    combo = [(lora_param, 0.7), ("style", 0.5)] if styleL else [(lora_param, 1.0)]
                    pe, ne, pp, npp = self.encode_prompt(rp, rn, combo, te_scale)
                region_prompt_embeds.append((ne, pe, npp, pp))
        req = dict(prompt_embeds=prompt_embeds, negative_prompt_embeds=negative_prompt_embeds,
                   pooled_prompt_embeds=pooled_prompt_embeds, negative_pooled_prompt_embeds=negative_pooled_prompt_embeds,
                   region_prompt_embeds=region_prompt_embeds, region_masks=region_masks, latents=latents, generator=generator)
        traj_many = [] if trajectory is not None else None
        lat = self.generate_many([req], height=height, width=width, num_inference_steps=num_inference_steps,
                                 guidance_scale=guidance_scale, cross_attention_kwargs=cross_attention_kwargs,
                                 original_size=original_size, crops_coords_top_left=crops_coords_top_left, target_size=target_size,
                                 controller=controller, concept_models=concept_models, stage=stage, lora_list=lora_list,
                                 styleL=styleL, use_graph=use_graph, trajectory=traj_many, fusion_start=fusion_start,
                                 lora_mode=lora_mode, controlnet=controlnet if image is not None else None, controlnet_image=image,
                                 controlnet_conditioning_scale=cn_scale, dedup=dedup, stage_cache=stage_cache, drop_unc0=drop_unc0,
                                 guess_mode=guess_mode and image is not None, control_guidance_start=cg_start, control_guidance_end=cg_end,
                                 negative_original_size=neg_cond[0], negative_crops_coords_top_left=neg_cond[1], negative_target_size=neg_cond[2],
                                 eta=eta, **callbacks)[0]
        if trajectory is not None:
            trajectory.extend(t[0] for t in traj_many)
        images = self._postprocess(lat, output_type)
        if not return_dict:
            return (images,)
        return StableDiffusionXLPipelineOutput(images=images)

    def _postprocess(self, lat: torch.Tensor, output_type: str):
        """The reference's tail (lora_pipeline.py:635-661): VAE decode + ``image_processor.postprocess``.  ``"latent"``: the final
        latents; ``"pt"``: decoded (n, 3, H, W) in [0, 1]; ``"np"``; ``"pil"`` (the reference's default): a list of PIL images."""
        if output_type == "latent":
            return lat
        if output_type not in ("pil", "pt", "np"):
            raise ValueError(f"output_type {output_type!r}")
        if self.vae_decode is None:
            raise L.OmgHipError("no VAE attached: use output_type='latent' or construct the pipeline with "
                                "vae_decode=omg_amd.vae.AutoencoderKLDecoder(...).decode_latents")
        images = self.vae_decode(lat)
        if output_type == "pt":
            return images
        arr = images.detach().float().cpu().permute(0, 2, 3, 1).numpy()
        if output_type == "np":
            return arr
        from PIL import Image
        return [Image.fromarray(a) for a in (arr * 255).round().astype("uint8")]

    # ------------------------------------------------------------------ n independent requests in lock-step
    @torch.no_grad()
    def generate_many(self, requests: Sequence[dict], *, height: Optional[int] = None, width: Optional[int] = None,
                      num_inference_steps: int = 50, guidance_scale: float = 5.0, cross_attention_kwargs=None,
                      original_size=None, crops_coords_top_left=(0, 0), target_size=None, controller=None,
                      concept_models: Optional[ConceptModels] = None, stage: Optional[int] = None,
                      lora_list: Optional[Sequence[str]] = None, styleL: Optional[bool] = None, use_graph: bool = False,
                      trajectory: Optional[list] = None, fusion_start: int = FUSION_START, lora_mode: str = "merged",
                      controlnet=None, controlnet_image: Optional[torch.Tensor] = None, controlnet_conditioning_scale: float = 1.0,
                      identitynet=None, identitynet_conditioning_scale: float = 1.0, dedup: bool = False,
                      concept_lora: bool = True, concept_shard=None,
                      main_adapters: Optional[Sequence[Tuple[str, float]]] = None,
                      concept_adapters: Optional[Sequence[Tuple[str, float]]] = None, concept_adapter_scale: float = 1.0,
                      stage_cache: Optional[StageCache] = None, drop_unc0: bool = False, guess_mode: bool = False,
                      control_guidance_start=0.0, control_guidance_end=1.0, negative_original_size=None, negative_crops_coords_top_left=(0, 0),
                      negative_target_size=None, callback: Optional[Callable] = None, callback_steps: Optional[int] = None,
                      callback_on_step_end: Optional[Callable] = None, callback_on_step_end_tensor_inputs=("latents",),
                      eta: float = 0.0) -> torch.Tensor:
        """Each request: dict(prompt_embeds (2,77,Cx), negative_prompt_embeds, pooled_prompt_embeds (2,P),
        negative_pooled_prompt_embeds, region_prompt_embeds [(neg, pos, neg_pooled, pos_pooled)] * K, region_masks [K],
        latents | generator).  Returns final latents (n, 2, C, H/8, W/8): [base sample, edited sample] per request.
        All requests must agree on which concepts have a mask.

        ``controlnet`` + ``controlnet_image`` (1|n,3,H,W in [0,1]): ControlNet on the MAIN pass of every step
        (lora_pipeline.py:519-536; ``controlnet2``/``t2i_image`` of instantid_pipeline.py:574-592).
        Round 6: ``controlnet`` may be a LIST of ControlNets (or an object with ``.nets``: the reference wraps a list in diffusers' MultiControlNetModel,
        lora_pipeline.py:175-176) with a list of images and of scales — every net sees its own image at its own scale, the residuals are summed in list
        order (:366-383, :511-512); ``control_guidance_start`` / ``_end`` (scalars or one per net) give ``controlnet_keep[i]`` — the per-step factor 0 / 1 on
        the conditioning scale (:275-286, :421-428, :511-517; a net whose factor is 0 in a step is not run: adding its zero residuals = not adding them),
        for the IdentityNet and the t2i ControlNet of the InstantID flow too (instantid_pipeline.py:477-483, :566-578); ``guess_mode=True``
        (:497-503, :531-535): the nets see only the CONDITIONAL rows ``[cond0, cond1]`` of every request, with diffusers' logspace residual scaling, and the
        unconditional rows get no residual.
        ``negative_original_size`` + ``negative_target_size`` (+ ``negative_crops_coords_top_left``): SDXL's negative micro-conditioning as the reference
        EXECUTES it (lora_pipeline.py:459-474): ``cat([negative_ids, ids]).repeat(2, 1)`` — the four main rows get [negative, positive, negative,
        positive] time ids, i.e. alternating, NOT [neg, neg, pos, pos] like the prompt embeddings.  Kept as executed.
        ``callback_on_step_end(pipe, i, t, {name: tensor})`` after every step with the tensors named in ``callback_on_step_end_tensor_inputs``
        (``latents`` (2, C, H/8, W/8) fp32, ``prompt_embeds`` (4, 77, Cx) = [neg, neg, pos, pos], ``negative_prompt_embeds`` (2, 77, Cx)), once per request;
        a returned ``{"latents": ...}`` replaces the request's latents for the next step (:617-626; a multistep scheduler keeps its data
        prediction of the step, as diffusers' ``model_outputs`` list does).  Returned prompt embeddings are refused (the
        cached cross-attention K / V would have to follow).  ``callback(i, t, latents)`` every ``callback_steps`` steps (:629-632).  Callbacks switch off
        ``dedup`` / ``stage_cache`` (they may make the two samples differ) and run between hipGraph replays.
        ``identitynet`` (InstantID, instantid_pipeline.py:638-674): ControlNet on the CONCEPT pass fed with the face tokens and
        the request's ``kps_image`` (1,3,H,W); requests then also carry ``region_image_embeds`` = [(2,16,Cx) [zero-id, id]] * K and
        the UNet must have an :class:`omg_amd.ip_adapter.IPAdapter` installed.

        ``main_adapters`` / ``concept_adapters`` [(name, weight)]: adapters of ``concept_models.bank`` that are simply ACTIVE on the main /
        on every concept row — PEFT's state after ``load_lora_weights`` when nobody calls ``set_adapters`` (inference_instantid.py:220-222
        loads a style LoRA into both pipes and the InstantID loop never selects adapters).  Main rows run them at the caller's
        ``cross_attention_kwargs["scale"]`` (instantid_pipeline.py:596-616), concept rows at ``concept_adapter_scale`` (the concept UNet is
        called with ``cross_attention_kwargs=None``, :665-674: scale 1.0).  ``styleL=True`` is ``main_adapters=[("style", 1.0)]`` plus the
        LoRA flow's [concept, style] combination on the concept rows.

        ``stage_cache`` (:class:`StageCache`, OFF by default): the steps in front of the first fused step of a stage-2 call
        repeat the stage-1 call of the same image; with a cache shared by the two calls the second one starts at step ``fusion_start + 1``.
        ``drop_unc0=True`` (with a cache that also holds the stage-1 call's trajectory of the base sample): the resumed steps do not compute
        ``unc0`` — 3 main rows per request instead of 4; the base sample's latents come from the cache at every step (last item:
        100 + 238 = 338 of the reference's 536 sample-forwards for both stages; bitwise the same latents, tests/test_pipeline_gpu.py).

        ``dedup=True`` (OFF by default; SURVEY §7.4, "flag when used"): the reference duplicates the latents (:409) and is called
        with two equal prompts, so until the first fused step the two samples of a request are the same computation twice
        (stage 1: for the whole call).  With the batch-invariant kernels of this package those steps run ``[unc, cond]`` once per
        request and write the result to both samples — bitwise the same latents as the full batch (tests/test_pipeline_gpu.py),
        16 x 2 of the 336 sample-forwards of a 50-step stage-2 call fewer.  Used only where it is provably exact: equal prompt /
        pooled / negative embeddings of the two samples, no controller or a pure-replacement one, and a ControlNet conditioning image
        that is shared (1 image) or per request (n images) — with one image per main row the call falls back to the full batch.

        ``concept_shard`` (:class:`omg_amd.parallel.ConceptShard`, every rank of its group calls with the SAME requests): the step's
        independent forward units — the main block of a request, each concept pair — are split over the ranks, one all_gather
        per step exchanges the noise predictions and every rank applies the same fusion + CFG + scheduler kernel, so all ranks
        return the same latents, bitwise equal to the unsharded call (SURVEY §8(e) finer-grain option; latency, not throughput).

        Stochastic steps: with :class:`omg_amd.schedulers.EulerAncestralDiscreteScheduler`, or :class:`DDIMScheduler` and ``eta > 0``, every step adds
        fresh Gaussian noise (the reference passes ``eta`` and ``generator`` to ``scheduler.step``, lora_pipeline.py:615; other schedulers ignore
        ``eta``, as diffusers' ``prepare_extra_step_kwargs`` does).  Right after a request's initial latents its ``generator`` draws S tensors
        (2, C, H/8, W/8), one per step, in step order: ``torch.randn(..., generator=g, device=<g's device, or the pipeline's without one>,
        dtype=float32)`` — with one request per call the reference's order of use.  The reference draws them in fp16, the UNet's dtype; they are
        fp32 here, as the latents are.  A resumed stage-2 call still draws all S.  The engine holds every step's noise of the call in ``eng.z``
        (S, 2n, C, H/8, W/8) fp32, which captured graphs point at (S = 50, n = 8 at 1024²: 210 MB).  ``dedup`` falls back to the full batch (the two
        samples of a request get different noise), a ``StageCache`` key also holds the generator's state in front of the noise draws (the noise
        itself without a generator), ``concept_shard`` is refused (the ranks would have to agree on the noise), and a callback that replaces
        ``latents`` leaves the noise as drawn."""
        dev, dt = self.unet.device, self.unet.dtype
        n = len(requests)
        height = height or self.unet.config.sample_size * self.vae_scale_factor
        width = width or self.unet.config.sample_size * self.vae_scale_factor
        lora_list = list(lora_list or [])
        S = num_inference_steps
        self.scheduler.set_timesteps(S, device=dev)
        original_size = original_size or (height, width)
        target_size = target_size or (height, width)
        stochastic = is_stochastic(self.scheduler, eta)      # omg_fuse_cfg_step_noise + the per-step noise eng.z
        nets = None if controlnet is None else list(controlnet.nets) if hasattr(controlnet, "nets") else list(controlnet) if isinstance(controlnet, (list, tuple)) else [controlnet]
        imgs = list(controlnet_image) if isinstance(controlnet_image, (list, tuple)) else [controlnet_image]
        # ---- 1. per-request tensors
        t = self._gather_requests(requests, len(lora_list), S, stage, stochastic, height, width, identitynet is not None)
        # ---- 2. the plan: every decision that needs no device buffer
        # one batched forward needs ONE UNet behind both pipes (omg_amd.compat shares it; hand-built ConceptModels may not)
        cm_bank = concept_models.bank if concept_models is not None else None
        plan = CallPlan(
            n=n, lora_list=lora_list, S=S, stage=stage, fusion_start=fusion_start, active=t.active, scheduler_cls=type(self.scheduler),
            stochastic=stochastic, guidance_scale=guidance_scale, use_graph=use_graph, n_nets=None if nets is None else len(nets),
            cn_image_shapes=[None if im is None else tuple(im.shape) for im in imgs] if nets is not None else (),
            controlnet_conditioning_scale=controlnet_conditioning_scale, guess_mode=guess_mode, control_guidance_start=control_guidance_start,
            control_guidance_end=control_guidance_end, has_identitynet=identitynet is not None,
            identitynet_conditioning_scale=identitynet_conditioning_scale, dedup=dedup, stage_cache=stage_cache is not None, drop_unc0=drop_unc0,
            concept_shard=concept_shard, has_controller=controller is not None, pure_controller=getattr(controller, "is_pure_replacement", False),
            callback=callback is not None, callback_steps=callback_steps, callback_on_step_end=callback_on_step_end is not None,
            callback_on_step_end_tensor_inputs=callback_on_step_end_tensor_inputs, has_concept_models=concept_models is not None,
            shared=concept_models is None or getattr(concept_models, "_unet", self.unet) is self.unet,
            bank_adapters=None if cm_bank is None else cm_bank.adapters, bank_mode=None if cm_bank is None else cm_bank.mode, lora_mode=lora_mode,
            concept_lora=concept_lora, styleL=styleL, main_adapters=main_adapters, concept_adapters=concept_adapters,
            concept_adapter_scale=concept_adapter_scale, main_scale=(cross_attention_kwargs or {}).get("scale", 1.0))
        controlnet, cn_nets = (nets[0], None) if plan.use_cn else (None, nets if plan.cn_multi else None)
        t.cn_image, t.cn_images = (imgs[0], None) if plan.use_cn else (None, imgs if plan.cn_multi else None)
        bank = cm_bank if plan.use_bank else None
        if bank is not None and plan.combos:
            if [tuple(c) for c in plan.combos] != list(bank.slots) or bank.scale != tuple(plan.scales) or bank.mode != lora_mode:
                bank.build(plan.combos, scale=plan.scales, mode=lora_mode)
        if plan.twin:      # both samples of every request must be the same computation: [neg0, neg1, pos0, pos1] with equal halves.
            # ONE fused device comparison and one host sync per call (four torch.equal syncs per request before every call)
            e_all, t_all = torch.stack(t.ehs_l), torch.stack(t.text_l)                   # (n, 4, 77, Cx), (n, 4, P)
            same = (e_all[:, 0] == e_all[:, 1]).all() & (e_all[:, 2] == e_all[:, 3]).all() & (t_all[:, 0] == t_all[:, 1]).all() & (t_all[:, 2] == t_all[:, 3]).all()
            plan.twin = bool(same)
        t.ehs, t.text = torch.cat(t.ehs_l, dim=0).contiguous(), torch.cat(t.text_l, dim=0)          # (4n, 77, Cx), (4n, P)
        t.tids_main = self._add_time_ids(original_size, crops_coords_top_left, target_size, plan.nm, dev)
        if negative_original_size is not None and negative_target_size is not None:
            # lora_pipeline.py:459-474 as executed: cat([negative_add_time_ids, add_time_ids]).repeat(batch_size, 1) -> rows [neg, pos, neg, pos]
            tids_neg = self._add_time_ids(negative_original_size, negative_crops_coords_top_left, negative_target_size, plan.nm, dev)
            t.tids_main = torch.where((torch.arange(plan.nm, device=dev) % 2 == 0)[:, None], tids_neg, t.tids_main)
        t.emb_main = all_step_embeddings(self.unet, t.ts, t.text, t.tids_main)
        if plan.fuse_possible:
            t.c_ehs, t.ctext = torch.cat(t.cehs_l, dim=0).contiguous(), torch.cat(t.ctext_l, dim=0)  # (2Ka*n, 77, Cx)
            t.tids_conc = self._add_time_ids(original_size, crops_coords_top_left, target_size, plan.ncn, dev)
            t.emb_conc = all_step_embeddings(getattr(concept_models, "_unet", None) or self.unet, t.ts, t.ctext, t.tids_conc)
        # DDIM's table depends on eta (column 3: the noise coefficient); eta = 0 is the deterministic table, byte for byte
        t.coef = self.scheduler.coef_table(dev, eta=eta) if isinstance(self.scheduler, DDIMScheduler) else self.scheduler.coef_table(dev)
        # ---- stage cache: decided in front of the engine because a resumed call without `unc0` runs a different row plan
        cache_keys: List[str] = []
        resume = StageCache.Resume()
        if plan.stage_cache:
            sizes = (height, width, tuple(original_size),
                     None if negative_original_size is None or negative_target_size is None else
                     (tuple(negative_original_size), tuple(negative_crops_coords_top_left), tuple(negative_target_size)),
                     tuple(crops_coords_top_left), tuple(target_size), str(dt))
            cache_keys = stage_cache_keys(plan, sizes, self.unet, bank, controller, controlnet, t)
            resume = stage_cache.lookup(cache_keys, plan, dev, dt)
        if resume.base_traj is not None:
            plan = plan.with_drop0()
        # ---- 3. the persistent engine of this call shape (static buffers + captured step graphs), reused across calls of the same shape
        Cl, Hl, Wl = t.lats[0].shape[1:]
        t.mshape = tuple(t.masks_l[0][t.active[0]].shape) if t.active else (0, 0)
        key = plan.engine_key((str(dt), Cl, Hl, Wl, t.mshape, tuple(t.ehs.shape), id(controller), id(controlnet), id(identitynet),
                               tuple(id(x) for x in cn_nets or ())))
        eng = self._engines.pop(key, None)
        if eng is None:
            eng = StepEngine(self.unet, plan, t, controller, controlnet, identitynet, cn_nets, concept_models)
            while len(self._engines) >= self.max_engines:      # least recently used first; its captured graphs go with it
                self._engines.pop(next(iter(self._engines)))
                self.engine_evictions += 1
                if self.engine_evictions in (1, 10, 100):
                    warnings.warn(f"LoraMultiConceptPipeline: step engine evicted ({self.engine_evictions} so far): more than max_engines="
                                  f"{self.max_engines} call shapes alternate and each eviction re-captures its hipGraphs; raise pipe.max_engines")
        self._engines[key] = eng                               # most recently used last
        # ---- 4. this call's inputs into the engine's buffers, 5. the denoising loop
        eng.load(plan, t, resume, self.scheduler, concept_models, cross_attention_kwargs, use_graph)
        for i in range(resume.first, S):
            eng.run_step(i)
            if plan.has_cb:
                self._step_callbacks(eng, i, callback, callback_steps, callback_on_step_end, callback_on_step_end_tensor_inputs)
            if trajectory is not None:
                trajectory.append(eng.lat.clone().view(n, 2, Cl, Hl, Wl))
            if cache_keys and resume.first == 0:
                stage_cache.store(cache_keys, i, fusion_start, eng.lat, eng.xin, eng.x0_hist if plan.multistep else None)
        if hasattr(controller, "bind_step_counter"):
            controller.bind_step_counter(None)      # the counter is the controller's own again (direct UNet calls)
        return eng.lat.clone().view(n, 2, Cl, Hl, Wl)

    def _gather_requests(self, requests: Sequence[dict], K: int, S: int, stage, stochastic: bool, height: int, width: int,
                         with_identity: bool) -> SimpleNamespace:
        """The per-request tensors of a call on the device, one list entry per request, and ``active``: the concepts that have a mask."""
        dev, dt = self.unet.device, self.unet.dtype
        t = SimpleNamespace(ts=self.scheduler.timesteps.to(torch.float32), lats=[], ehs_l=[], text_l=[], masks_l=[], cehs_l=[], ctext_l=[], ip_l=[],
                            kps_l=[], z_l=[], zid_l=[], active=None)      # z_l / zid_l (stochastic): per request the (S, 2, C, H, W) noise and what identifies it
        for r in requests:
            pe, ne = r["prompt_embeds"], r["negative_prompt_embeds"]
            if pe.shape[0] != 2:
                raise ValueError("prompt_embeds must hold the 2 global prompts [p, p] (lora_pipeline.py:291)")
            lat0 = self.prepare_latents(1, self.unet.config.in_channels, height, width, torch.float32, dev, r.get("generator"), r.get("latents"))
            t.lats.append(torch.cat([lat0, lat0.clone()]))                                            # duplicated x2 (:409)
            if stochastic:      # then one (2, C, H/8, W/8) draw per step, one at a time (a single (S, 2, ...) draw gives other numbers)
                g = r.get("generator")
                z_id = g.get_state() if g is not None else None
                zs = [draw_noise((2,) + tuple(lat0.shape[1:]), g, dev) for _ in range(S)]
                t.z_l.append(torch.stack(zs))
                t.zid_l.append(z_id if z_id is not None else t.z_l[-1])
            t.ehs_l.append(torch.cat([ne, pe], dim=0).to(device=dev, dtype=dt))                       # CFG order [neg, pos] (:467-474)
            t.text_l.append(torch.cat([r["negative_pooled_prompt_embeds"], r["pooled_prompt_embeds"]], dim=0).to(device=dev, dtype=dt))
            rpe = r.get("region_prompt_embeds") or []
            if len(rpe) != K:
                raise ValueError("one (neg_embeds, pos_embeds, neg_pooled, pos_pooled) tuple per entry of lora_list is required")
            masks = [None] * K
            if stage == 2:
                rm = r.get("region_masks")
                if rm is None or len(rm) != K:
                    raise ValueError("stage 2 needs one region mask (or None) per entry of lora_list")
                masks = [m.to(device=dev, dtype=torch.float32).contiguous() if m is not None else None for m in rm]
            act = [c for c in range(K) if masks[c] is not None]
            if t.active is None:
                t.active = act
            elif act != t.active:
                raise ValueError("requests batched together must have masks for the same concepts")
            t.masks_l.append(masks)
            if act:
                t.cehs_l.append(torch.cat([torch.cat([rpe[c][0], rpe[c][1]], dim=0) for c in act], dim=0).to(device=dev, dtype=dt))
                t.ctext_l.append(torch.cat([torch.cat([rpe[c][2], rpe[c][3]], dim=0) for c in act], dim=0).to(device=dev, dtype=dt))
                if with_identity:
                    rie = r.get("region_image_embeds")
                    if rie is None or len(rie) != K or r.get("kps_image") is None:
                        raise ValueError("identitynet needs region_image_embeds [(2,16,Cx)] * K and kps_image per request")
                    t.ip_l.append(torch.cat([rie[c] for c in act], dim=0).to(device=dev, dtype=dt))
                    t.kps_l.append(r["kps_image"].to(device=dev, dtype=torch.float32))
        return t

    def _step_callbacks(self, eng: "StepEngine", i: int, callback, callback_steps, callback_on_step_end, tensor_inputs) -> None:
        """The reference's callbacks after step i (lora_pipeline.py:617-632), once per request; see ``generate_many``."""
        t_i = self.scheduler.timesteps[i]
        ehs = eng.main.ehs
        for j in range(eng.plan.n):
            lj = eng.lat[2 * j: 2 * j + 2]
            if callback_on_step_end is not None:
                avail = {"latents": lj, "prompt_embeds": ehs[4 * j: 4 * j + 4], "negative_prompt_embeds": ehs[4 * j: 4 * j + 2]}
                outs = dict(callback_on_step_end(self, i, t_i, {k: avail[k] for k in tensor_inputs}) or {})
                new = outs.pop("latents", lj)
                for k_, v_ in outs.items():
                    if k_ in avail and v_ is not avail[k_] and not torch.equal(v_.to(avail[k_]), avail[k_]):
                        raise L.OmgHipError(f"callback_on_step_end returned a new {k_}: only `latents` can be replaced mid-loop")
                if new is not lj:
                    lj.copy_(new.to(device=lj.device, dtype=torch.float32))
                    if i + 1 < eng.plan.S:      # the step kernel wrote the next model input from ITS latents: redo it from the callback's
                        ops.scale_model_input(lj, torch.tensor([self.scheduler.cin[i + 1]], dtype=torch.float32, device=lj.device), eng.xin[4 * j: 4 * j + 4])
            if callback is not None and i % int(callback_steps) == 0:
                callback(i // getattr(self.scheduler, "order", 1), t_i, lj)


class InstantidMultiConceptPipeline(LoraMultiConceptPipeline):
    """OMG + InstantID (/root/reference src/pipelines/instantid_pipeline.py:157-768, BASELINE config 3) on the same step engine.

    Reference roles -> here: ``self.controlnet`` (IdentityNet, applied to every CONCEPT pass with the face tokens as context and the
    key-point image as conditioning, :638-648) = ``identitynet``; ``self.controlnet2`` + ``t2i_image`` (optional pose/depth ControlNet on the
    MAIN pass, :574-616) = ``controlnet2``; the concept UNet's IP-Adapter processors (instantid_single_pieline.py:186-213) = an
    :class:`omg_amd.ip_adapter.IPAdapter` installed on the shared UNet.  Face detection / ArcFace embedding (``face_app``) and the
    Resampler that turns a 512-d embedding into 16 tokens run once per image outside the hot path: pass the
    resulting tokens as ``region_image_embeds`` = [(2, 16, Cx) = [tokens of the zero embedding, tokens of the identity]] per concept
    (:class:`omg_amd.resampler.Resampler` computes them from the embedding: ``resampler(torch.stack([zeros, emb]).view(2, 1, 512))``,
    instantid_single_pieline.py:221-243)."""

    def __init__(self, unet, identitynet, scheduler=None, controlnet2=None, **kw):
        super().__init__(unet, scheduler, **kw)
        self.controlnet = identitynet
        self.controlnet2 = controlnet2

    @torch.no_grad()
    def __call__(self, prompt_embeds=None, negative_prompt_embeds=None, pooled_prompt_embeds=None, negative_pooled_prompt_embeds=None,
                 image: Optional[torch.Tensor] = None, t2i_image: Optional[torch.Tensor] = None, height=None, width=None,
                 num_inference_steps: int = 50, guidance_scale: float = 5.0, generator=None, latents=None,
                 controlnet_conditioning_scale: float = 1.0, t2i_controlnet_conditioning_scale: float = 1.0, controller=None,
                 concept_models: Optional[ConceptModels] = None, stage: Optional[int] = None, region_masks=None,
                 region_prompt_embeds=None, region_image_embeds=None, output_type: str = "pil", return_dict: bool = True,
                 use_graph: bool = False, trajectory: Optional[list] = None, fusion_start: int = FUSION_START, dedup: bool = False,
                 cross_attention_kwargs=None, main_adapters=None, concept_adapters=None, lora_mode: str = "merged", eta: float = 0.0,
                 original_size=None, crops_coords_top_left=(0, 0), target_size=None, guess_mode: bool = False,
                 control_guidance_start=0.0, control_guidance_end=1.0, **kwargs):
        """``main_adapters`` / ``concept_adapters`` [(name, weight)]: LoRA adapters of ``concept_models.bank`` that PEFT would have active
        on the main / the concept pipe (inference_instantid.py:220-222 loads a style LoRA into both; nothing deactivates it).  The main
        UNet is called with ``cross_attention_kwargs`` (its ``"scale"`` is the LoRA scale, :596-616), the concept UNet with
        ``cross_attention_kwargs=None`` (:665-674): LoRA scale 1.0."""
        if prompt_embeds is None:
            raise L.OmgHipError("pass prompt_embeds=/pooled_prompt_embeds= (text encoders are outside this package's scope)")
        stage_cache = kwargs.pop("stage_cache", None)
        if guess_mode:
            # the reference's OWN InstantID loop cannot run it: the IdentityNet is fed the two concept rows and its residuals are then concatenated with
            # zeros to FOUR rows for a two-row concept UNet (instantid_pipeline.py:638-657), and the t2i net's two-row residuals meet the four-row main
            # UNet without that concatenation (:580-616) — a shape error either way.  The LoRA flow's guess_mode is implemented (generate_many).
            raise L.OmgHipError("guess_mode=True: the reference's InstantID loop itself fails on it (residual batch 4 vs 2, instantid_pipeline.py:638-657); "
                                "LoraMultiConceptPipeline implements it")
        for dead in ("face_app", "prompt", "negative_prompt", "prompt_2", "negative_prompt_2", "clip_skip"):      # consumed by omg_amd.compat's front end
            kwargs.pop(dead, None)                                                                                 # (prompt encoding) when the scripts call it; dead here
        neg_cond = (kwargs.pop("negative_original_size", None), kwargs.pop("negative_crops_coords_top_left", (0, 0)), kwargs.pop("negative_target_size", None))
        callbacks = dict(callback=kwargs.pop("callback", None), callback_steps=kwargs.pop("callback_steps", None),
                         callback_on_step_end=kwargs.pop("callback_on_step_end", None),
                         callback_on_step_end_tensor_inputs=kwargs.pop("callback_on_step_end_tensor_inputs", ("latents",)))
        refuse_unimplemented({k: kwargs.pop(k) for k in list(kwargs) if k in _UNIMPLEMENTED}, kwargs, "InstantidMultiConceptPipeline.__call__")
        K = len(region_prompt_embeds or [])
        # stage 1 is called with image=None: no IdentityNet (instantid_pipeline.py:393, :426-428)
        use_idn = stage == 2 and image is not None
        req = dict(prompt_embeds=prompt_embeds, negative_prompt_embeds=negative_prompt_embeds, pooled_prompt_embeds=pooled_prompt_embeds,
                   negative_pooled_prompt_embeds=negative_pooled_prompt_embeds, region_prompt_embeds=region_prompt_embeds or [],
                   region_masks=region_masks, latents=latents, generator=generator,
                   region_image_embeds=region_image_embeds if use_idn else None, kps_image=image if use_idn else None)
        traj_many = [] if trajectory is not None else None
        lat = self.generate_many([req], height=height, width=width, num_inference_steps=num_inference_steps, guidance_scale=guidance_scale,
                                 controller=controller, concept_models=concept_models or ConceptModels(self.unet, None), stage=stage,
                                 lora_list=[f"id{c}" for c in range(K)], styleL=False, use_graph=use_graph, trajectory=traj_many,
                                 fusion_start=fusion_start, identitynet=self.controlnet if use_idn else None,
                                 identitynet_conditioning_scale=controlnet_conditioning_scale,
                                 controlnet=self.controlnet2 if t2i_image is not None else None, controlnet_image=t2i_image,
                                 controlnet_conditioning_scale=t2i_controlnet_conditioning_scale, dedup=dedup, concept_lora=False,
                                 cross_attention_kwargs=cross_attention_kwargs, main_adapters=main_adapters,
                                 concept_adapters=concept_adapters, concept_adapter_scale=1.0, lora_mode=lora_mode,
                                 stage_cache=stage_cache, original_size=original_size, crops_coords_top_left=crops_coords_top_left,
                                 target_size=target_size, control_guidance_start=control_guidance_start, control_guidance_end=control_guidance_end,
                                 negative_original_size=neg_cond[0], negative_crops_coords_top_left=neg_cond[1], negative_target_size=neg_cond[2],
                                 eta=eta, **callbacks)[0]
        if trajectory is not None:
            trajectory.extend(t[0] for t in traj_many)
        lat = self._postprocess(lat, output_type)
        return StableDiffusionXLPipelineOutput(images=lat) if return_dict else (lat,)
