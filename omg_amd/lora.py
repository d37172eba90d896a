"""Multi-adapter LoRA bank for the concept UNet.

Replaces PEFT's un-merged LoRA layers and ``concept_models.set_adapters(...)`` toggling
(/root/reference src/pipelines/lora_pipeline.py:340-342, :588-591; ``peft==0.8.2``,
``inference_lora.py:166-170``): ``y = base(x) + scale * w_a * (alpha_a / r_a) * B_a(A_a(x))`` summed over
the active adapters ``a`` (``[lora, "style"]`` with weights ``[0.7, 0.5]`` when ``styleL``).

MI355X-first: instead of walking the module tree in Python 68 times per image to switch adapters,
every *combination* that the pipeline will use becomes one "slot" — the active adapters' A matrices
stacked along the rank axis, their scaled B matrices stacked likewise — and all slots live in HBM at
once (``lora_down [slots, r, in]``, ``lora_up [slots, out, r]``).  A per-sample int32 vector then
selects the slot inside the GEMM (second K-segment, see ``omg_gemm``), so the K concept passes of a
step run as ONE batched forward with different adapters per sample, and the whole step stays
capturable in a hipGraph.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib as L
from .attention import Attention
from . import ops
from .modules import Conv2d, GEGLU, Linear, bump_pointer_epoch, lora_conv_targets


class LoraTerm:
    """One module's delta in an algebra other than a bare pair, or a pair that carries a DoRA magnitude.  ``factors`` holds the fp32
    tensors under the names the kohya / LyCORIS files use:

    * ``plain``: ``lora_down [r, in]`` / ``[r, Cin, k, k]``, ``lora_up [out, r]``;                       delta = up . down
    * ``hada`` (LoHa): ``hada_w1_a [out, r]``, ``hada_w1_b [r, in k k]``, ``hada_w2_a``, ``hada_w2_b``;   delta = (w1_a . w1_b) * (w2_a . w2_b)
    * ``kron`` (LoKr): ``lokr_w1 [a, b]`` or ``lokr_w1_a [a, r]`` . ``lokr_w1_b [r, b]``, and ``lokr_w2 [c, d]`` / ``[c, d, k, k]`` or
      ``lokr_w2_a [c, r]`` . ``lokr_w2_b [r, d k k]``;   delta[ia c + ic, ib d + id, ky, kx] = w1[ia, ib] w2[ic, id, ky, kx]

    ``alpha`` is the file's value (``None``: absent); ``factor`` is ``alpha / r`` — 1 without ``alpha``, and 1 for a LoKr whose two operands
    are both full matrices, whatever ``alpha`` holds.  ``magnitude`` is DoRA's per-output-channel vector ``[out]`` or ``None``."""

    KINDS = ("plain", "hada", "kron")

    def __init__(self, kind: str, factors: Dict[str, torch.Tensor], alpha: Optional[float] = None, magnitude: Optional[torch.Tensor] = None):
        if kind not in self.KINDS:
            raise ValueError(kind)
        self.kind = kind
        self.factors = {k: v.float() for k, v in factors.items()}
        self.alpha = None if alpha is None else float(alpha)
        self.magnitude = None if magnitude is None else magnitude.float().reshape(-1)

    @property
    def rank(self) -> Optional[int]:
        """The rank ``alpha`` is divided by; ``None`` for a LoKr of two full matrices."""
        f = self.factors
        if self.kind == "plain":
            return f["lora_down"].shape[0]
        if self.kind == "hada":
            return f["hada_w1_b"].shape[0]
        if "lokr_w2_b" in f:
            return f["lokr_w2_b"].shape[0]
        if "lokr_w1_b" in f:
            return f["lokr_w1_b"].shape[0]
        return None

    @property
    def factor(self) -> float:
        r = self.rank
        return 1.0 if self.alpha is None or r is None else self.alpha / r

    @property
    def out_features(self) -> int:
        f = self.factors
        if self.kind == "plain":
            return f["lora_up"].shape[0]
        if self.kind == "hada":
            return f["hada_w1_a"].shape[0]
        return self._kron_operands()[0].shape[0] * self._kron_operands()[1].shape[0]

    def _kron_operands(self, device=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(w1 [a, b], w2 [c, d] / [c, d, k, k] or, from a factored w2, [c, d k k]) with the factored operands multiplied out in fp32."""
        f = {k: (v if device is None else v.to(device)) for k, v in self.factors.items()}
        w1 = f["lokr_w1"] if "lokr_w1" in f else f["lokr_w1_a"] @ f["lokr_w1_b"]
        w2 = f["lokr_w2"] if "lokr_w2" in f else f["lokr_w2_a"] @ f["lokr_w2_b"]
        return w1, w2

    def kernel_term(self, n_out: int, cin: int, ksize: int, device) -> Tuple[str, Tuple[torch.Tensor, ...]]:
        """``(kind, factors)`` as ``ops.lora_merge`` takes them for a layer ``[n_out, ksize * ksize * cin]``: fp32 on ``device``, columns in
        the packed ``(ky, kx, cin)`` order of ``ops.pack_conv_weight`` — a permutation of the small factors, not of the delta.  Raises
        ``ValueError`` with the reason when the factors do not fit the layer."""
        taps, f = ksize * ksize, {k: v.to(device) for k, v in self.factors.items()}

        def cols(m: torch.Tensor, c: int, what: str) -> torch.Tensor:          # [r, c k k] in (c, ky, kx) order -> [r, k k c] packed
            if m.dim() != 2 or m.shape[1] != c * taps:
                raise ValueError(f"{what} {tuple(m.shape)} is not [r, {c * taps}]")
            return m.reshape(m.shape[0], c, taps).permute(0, 2, 1).reshape(m.shape[0], taps * c).contiguous()

        def rows(m: torch.Tensor, r: int, what: str) -> torch.Tensor:
            if m.dim() != 2 or tuple(m.shape) != (n_out, r):
                raise ValueError(f"{what} {tuple(m.shape)} is not [{n_out}, {r}]")
            return m.contiguous()

        if self.kind == "plain":
            down = f["lora_down"]
            down = cols(down.reshape(down.shape[0], -1), cin, "lora_down")
            return "plain", (rows(f["lora_up"].reshape(f["lora_up"].shape[0], -1), down.shape[0], "lora_up"), down)
        if self.kind == "hada":
            b1, b2 = cols(f["hada_w1_b"], cin, "hada_w1_b"), cols(f["hada_w2_b"], cin, "hada_w2_b")
            return "hada", (rows(f["hada_w1_a"], b1.shape[0], "hada_w1_a"), b1, rows(f["hada_w2_a"], b2.shape[0], "hada_w2_a"), b2)
        w1, w2 = self._kron_operands(device)
        if w1.dim() != 2 or w1.shape[0] < 1 or w1.shape[1] < 1 or n_out % w1.shape[0] or cin % w1.shape[1]:
            raise ValueError(f"lokr_w1 {tuple(w1.shape)} does not divide [{n_out}, {cin}]")
        c, d = n_out // w1.shape[0], cin // w1.shape[1]
        if w2.shape[0] != c or w2.numel() != c * d * taps or (w2.dim() == 4 and tuple(w2.shape[1:]) != (d, ksize, ksize)) or w2.dim() not in (2, 4):
            raise ValueError(f"lokr_w2 {tuple(w2.shape)} is not [{c}, {d}" + (f", {ksize}, {ksize}]" if ksize > 1 else "]"))
        return "kron", (w1.contiguous(), w2.reshape(c, d, taps).permute(0, 2, 1).contiguous())

    def dense(self) -> torch.Tensor:
        """The fp32 delta ``[out, in]`` of a Linear target, without ``factor`` (the text encoders merge it on the host side of the packing)."""
        f = self.factors
        if self.kind == "plain":
            return f["lora_up"] @ f["lora_down"]
        if self.kind == "hada":
            return (f["hada_w1_a"] @ f["hada_w1_b"]) * (f["hada_w2_a"] @ f["hada_w2_b"])
        w1, w2 = self._kron_operands()
        return torch.kron(w1, w2)


class LoraAdapter:
    """One named adapter: ``weights[module_path] = (A [r, in], B [out, r])`` and its ``alpha``.  For a convolution target
    (LoCon / PEFT ``Conv2d``) the pair is ``A [r, Cin, k, k]`` — a conv with the base layer's kernel, stride and padding — and
    ``B [out, r]`` or ``[out, r, 1, 1]``.

    Layers may have different ranks (PEFT ``rank_pattern``, common in kohya files): ``rank`` is the largest one — the width a
    layer occupies in the slot stacks, smaller layers are zero-padded — and the PEFT factor ``alpha / r`` uses each layer's own
    ``r``.  ``alpha=None`` means "alpha equals the rank of every layer" (factor 1), PEFT's and diffusers' default and what the
    file loaders produce after folding a per-layer ``alpha`` into B.  ``text_encoder`` optionally carries the text-encoder
    half of the file: ``{1 | 2: {module_path: (A, B)}}`` with factors already folded into B (omg_amd/loaders.py), or a
    :class:`LoraTerm` for a LoHa / LoKr entry.

    ``terms[module_path]`` holds a :class:`LoraTerm` for every module whose delta is not a bare pair: LoHa, LoKr, and any algebra
    (a plain pair included) with a DoRA magnitude.  A module is in ``weights`` or in ``terms``, never in both.  ``rank`` is defined by
    the plain pairs of ``weights`` alone — the width of the un-merged stacks — and is 0 for an adapter without any."""

    def __init__(self, name: str, weights: Dict[str, Tuple[torch.Tensor, torch.Tensor]], alpha: Optional[float] = None,
                 text_encoder: Optional[Dict[int, Dict[str, Tuple[torch.Tensor, torch.Tensor]]]] = None,
                 terms: Optional[Dict[str, LoraTerm]] = None):
        self.name, self.weights = name, weights
        self.terms = dict(terms or {})
        both = sorted(set(self.terms) & set(weights))
        if both:
            raise ValueError(f"adapter {name!r}: {both[0]} is both a plain pair and a term")
        self.rank = max(a.shape[0] for a, _ in weights.values()) if weights else 0
        self._alpha_given = alpha is not None
        self.alpha = float(alpha) if alpha is not None else float(self.rank)
        self.text_encoder = text_encoder or {}

    def scaling(self, key: str) -> float:
        """PEFT's ``lora_alpha / r`` of one layer."""
        return self.alpha / self.weights[key][0].shape[0] if self._alpha_given else 1.0


def lora_target_names(unet) -> List[str]:
    """All attention + feed-forward Linear layers (synthetic coverage of SURVEY.md §8d)."""
    out = []
    for name, m in unet.named_modules():
        if isinstance(m, Linear) and any(s in name for s in (".to_q", ".to_k", ".to_v", ".to_out.0", ".ff.net.0.proj", ".ff.net.2")):
            out.append(name)
    return out


def lora_conv_target_names(unet) -> List[str]:
    """Every convolution a LoRA may target (:func:`omg_amd.modules.lora_conv_targets`)."""
    return list(lora_conv_targets(unet))


def make_synthetic_adapter(unet, name: str, rank: int, seed: int, conv: bool = False) -> LoraAdapter:
    """Random adapter generated on the device: A ~ N(0, 1/in), B ~ N(0, 1e-2).  ``conv=True`` adds every convolution target,
    drawn AFTER all Linear ones (the Linear weights of a seed do not depend on it)."""
    g = torch.Generator(device=unet.device).manual_seed(seed)
    w = {}
    for key in lora_target_names(unet):
        lin = unet.get_submodule(key)
        a = torch.randn(rank, lin.in_features, generator=g, device=unet.device) * lin.in_features ** -0.5
        b = torch.randn(lin.out_features, rank, generator=g, device=unet.device) * 0.1
        w[key] = (a.to(unet.dtype), b.to(unet.dtype))
    if conv:
        for key in lora_conv_target_names(unet):
            cv = unet.get_submodule(key)
            fan_in = cv.cin * cv.ksize * cv.ksize
            a = torch.randn(rank, cv.cin, cv.ksize, cv.ksize, generator=g, device=unet.device) * fan_in ** -0.5
            b = torch.randn(cv.cout, rank, generator=g, device=unet.device) * 0.1
            w[key] = (a.to(unet.dtype), b.to(unet.dtype))
    return LoraAdapter(name, w)


class LoraBank:
    def __init__(self, unet, adapters: Sequence[LoraAdapter]):
        self.unet = unet
        self.adapters = {a.name: a for a in adapters}
        self.slots: List[Tuple[Tuple[str, float], ...]] = []
        self.scale = 1.0
        self.mode = "merged"
        self.version = 0             # advances with every build(): engines keyed on it never reuse stale slot stacks

    def slot_of(self, combo: Sequence[Tuple[str, float]]) -> int:
        return self.slots.index(tuple((n, float(w)) for n, w in combo))

    def build(self, slots: Sequence[Sequence[Tuple[str, float]]], scale: float = 1.0, mode: str = "merged", merge: str = "auto") -> None:
        """Materialise the slot stacks on every target Linear and Conv2d (conv stacks in the packed ``[.., ky, kx, Cin]`` column order
        of the conv weight, so that the merge ``W + s*B A`` is the same matrix product as for a Linear).  ``slots[s]`` = [(adapter name, weight), ...];
        ``scale`` is ``cross_attention_kwargs['scale']`` (0.8 in OMG, lora_pipeline.py:596) — a float, or one value per slot.

        mode="segment": keep A/B un-merged (PEFT's arithmetic: base(x) + s*B(A(x)), second K-segment of omg_gemm).
        mode="merged" : additionally build ``w_slots[1+S, out, in] = [W, W + s*B_1 A_1, ...]`` (fp32 merge, one
        rounding) so that a batch mixing base and concept samples runs ONE GEMM per layer with a per-sample weight
        slot and zero LoRA overhead — 4.4 GB of HBM per concept, which a 288 GB part has to spare.

        ``merge`` chooses who forms the slots of a layer.  ``"auto"``: a layer whose terms are plain pairs without a magnitude in every
        slot goes through the fp32 torch expression ``W + up @ down`` it always went through (its ``w_slots`` keep their bits); every other
        layer — LoHa, LoKr, a DoRA magnitude (``LoraAdapter.terms``) — is merged by ``omg_lora_merge``:
        ``W_slot = round16(W (1 + sum_a (g_a - 1)) + sum_a g_a s_a delta_a)``, ``g_a = m_a / ||W + s_a delta_a||`` per output channel
        (1 without a magnitude), ``s_a`` = slot scale x adapter weight x ``alpha / r``.  ``"hip"`` sends every layer through the kernel;
        ``"torch"`` refuses non-plain terms.  ``mode="segment"`` refuses them too: those deltas are not low-rank.  The un-merged stacks
        ``lora_down`` / ``lora_up`` carry plain pairs only."""
        if mode not in ("merged", "segment"):
            raise ValueError(mode)
        if merge not in ("auto", "hip", "torch"):
            raise ValueError(merge)
        self.mode = mode
        self.slots = [tuple((n, float(w)) for n, w in s) for s in slots]
        # one scale for every slot, or one per slot (the reference's concept passes hard-code 0.8, lora_pipeline.py:596, while
        # the main pass's style adapter takes the caller's cross_attention_kwargs["scale"], :546-566)
        per_slot = [float(x) for x in scale] if isinstance(scale, (list, tuple)) else [float(scale)] * len(self.slots)
        if len(per_slot) != len(self.slots):
            raise ValueError("one LoRA scale per slot")
        self.scale = tuple(per_slot) if isinstance(scale, (list, tuple)) else scale
        dev, dt = self.unet.device, self.unet.dtype
        used = [self.adapters[n] for n in dict.fromkeys(n for s in self.slots for n, _ in s)]
        if mode == "segment":
            for a in used:
                if a.terms:
                    raise L.OmgHipError(f"adapter {a.name!r}, module {sorted(a.terms)[0]}: a LoHa / LoKr delta or a DoRA magnitude is no low-rank "
                                        f"second K-segment; build the bank with mode='merged'")
        keys = set()
        for a in self.adapters.values():
            keys.update(a.weights)
            keys.update(a.terms)
        r_tot = max(sum(self.adapters[n].rank for n, _ in s) for s in self.slots)
        r_tot = (r_tot + 7) // 8 * 8
        self.clear()
        conv_ok = lora_conv_targets(self.unet)
        for key in sorted(keys):
            mod = self.unet.get_submodule(key)
            is_conv = isinstance(mod, Conv2d)
            if is_conv:
                if key not in conv_ok:
                    raise L.OmgHipError(f"LoRA target {key}: conv_in / conv_out, fp32-storage convolutions and convolutions whose input "
                                        f"channels are no multiple of 64 are not LoRA targets")
                n_in, n_out = mod.ksize * mod.ksize * mod.cin, mod.cout
            elif isinstance(mod, Linear):
                n_in, n_out = mod.in_features, mod.out_features
            else:
                raise L.OmgHipError(f"LoRA target {key} is neither a Linear nor a Conv2d layer")
            has_plain = any(key in a.weights for a in self.adapters.values())
            plain_only = not any(key in a.terms for a in used)
            if not plain_only and merge == "torch":
                raise L.OmgHipError(f"LoRA target {key}: merge='torch' forms up @ down only; LoHa / LoKr / DoRA terms need the merge kernel")
            # the un-merged stacks carry plain pairs only; an adapter set without any (rank 0) gets none: no zero-width stack reaches a kernel
            down = up = None
            if has_plain and r_tot > 0:
                down = torch.zeros(len(self.slots), r_tot, n_in, dtype=torch.float32, device=dev)
                up = torch.zeros(len(self.slots), n_out, r_tot, dtype=torch.float32, device=dev)
                for s, combo in enumerate(self.slots):
                    r0 = 0
                    for name, w in combo:
                        ad = self.adapters[name]
                        if key not in ad.weights:
                            r0 += ad.rank
                            continue
                        a, b = self._fit_pair(key, mod, is_conv, *ad.weights[key])
                        r = a.shape[0]                                   # <= ad.rank; the rest of the adapter's band stays zero
                        down[s, r0:r0 + r] = a.to(dev).float()
                        up[s, :, r0:r0 + r] = b.to(dev).float() * (per_slot[s] * w * ad.scaling(key))
                        r0 += ad.rank
                mod.lora_down = down.to(dt).contiguous()
                mod.lora_up = up.to(dt).contiguous()
            if mode != "merged":
                continue
            if merge == "torch" or (merge == "auto" and plain_only):
                if down is None:
                    continue
                base = (ops.pack_conv_weight(mod.weight.data) if is_conv else mod.weight.data).float()
                mod.w_slots = torch.stack([base] + [base + up[s_] @ down[s_] for s_ in range(len(self.slots))]).to(dt).contiguous()
            else:
                mod.w_slots = self._merge_hip(key, mod, is_conv, n_out, n_in, per_slot)
        if mode == "merged":
            # the fused q|k|v (k|v) GEMM takes one weight stack per slot: an attention whose adapter targets only some of
            # its projections (custom PEFT target_modules) gets the base weight repeated for the others
            for m in self.unet.modules():
                if isinstance(m, Attention):
                    projs = (m.to_q, m.to_k, m.to_v)
                    if any(l.w_slots is not None for l in projs):
                        for l in projs:
                            if l.w_slots is None:
                                l.w_slots = l.weight.data.unsqueeze(0).repeat(1 + len(self.slots), 1, 1).contiguous()
            for m in self.unet.modules():      # the phase images of the new conv slots, here and not inside a captured forward
                if isinstance(m, Conv2d) and m.upsamples and m.w_slots is not None and m._phase_form(True, None, None):
                    m.slot_phase_weight()
        self.version += 1
        self._invalidate_packed()

    @staticmethod
    def _fit_pair(key, mod, is_conv, a, b):
        """A plain pair in the layer's GEMM form: ``(down [r, K], up [out, r])``, a convolution's down in the packed column order."""
        if is_conv:
            if a.dim() != 4 or tuple(a.shape[1:]) != (mod.cin, mod.ksize, mod.ksize) or b.reshape(b.shape[0], -1).shape != (mod.cout, a.shape[0]):
                raise L.OmgHipError(f"LoRA target {key}: down {tuple(a.shape)} / up {tuple(b.shape)} do not fit a "
                                    f"{mod.ksize}x{mod.ksize} convolution {mod.cin} -> {mod.cout}")
            a, b = ops.pack_conv_weight(a), b.reshape(b.shape[0], -1)
        return a, b

    def _merge_hip(self, key, mod, is_conv, n_out, n_in, per_slot) -> torch.Tensor:
        """``w_slots[1 + S, out, K]`` of one layer through ``omg_lora_merge``: per slot, the active adapters' terms — plain pairs, LoHa, LoKr,
        each with or without a DoRA gain ``m / ||W + s delta||`` (``omg_lora_rownorm``, one norm per adapter, PEFT's rule for several
        active adapters) — are added to the 16-bit base in fp32 and rounded once.  No dense fp32 delta or ``[1 + S, N, K]`` temporary."""
        dev = self.unet.device
        base = (ops.pack_conv_weight(mod.weight.data) if is_conv else mod.weight.data).contiguous()
        cin, ksize = (mod.cin, mod.ksize) if is_conv else (n_in, 1)
        w_slots = torch.empty(1 + len(self.slots), n_out, n_in, dtype=base.dtype, device=dev)
        w_slots[0] = base
        fitted = {}                                               # adapter name -> (kind, device factors): shared by the slots that use it
        for s, combo in enumerate(self.slots):
            terms = []
            for name, w in combo:
                ad = self.adapters[name]
                if key not in ad.weights and key not in ad.terms:
                    continue
                if name not in fitted:
                    if key in ad.weights:
                        a, b = self._fit_pair(key, mod, is_conv, *ad.weights[key])
                        fitted[name] = ("plain", (b.to(dev).float().contiguous(), a.to(dev).float().contiguous()), ad.scaling(key), None)
                    else:
                        t = ad.terms[key]
                        try:
                            kind, f = t.kernel_term(n_out, cin, ksize, dev)
                        except ValueError as e:
                            raise L.OmgHipError(f"adapter {name!r}, LoRA target {key}: {e}") from None
                        if t.magnitude is not None and t.magnitude.numel() != n_out:
                            raise L.OmgHipError(f"adapter {name!r}, LoRA target {key}: a magnitude of {t.magnitude.numel()} values for {n_out} output channels")
                        fitted[name] = (kind, f, t.factor, None if t.magnitude is None else t.magnitude.to(dev).contiguous())
                kind, f, factor, mag = fitted[name]
                term = {"kind": kind, "f": f, "s": per_slot[s] * w * factor}
                if mag is not None:
                    term["gain"] = (mag / ops.lora_rownorm(base, term)).contiguous()
                terms.append(term)
            if len(terms) > L.LORA_MAX_TERMS:
                raise L.OmgHipError(f"LoRA target {key}, slot {s}: {len(terms)} adapter terms, at most {L.LORA_MAX_TERMS} per slot and layer")
            ops.lora_merge(base, terms, w_slots[1 + s])
        return w_slots

    def _invalidate_packed(self) -> None:
        """Only the modules whose packed images contain LoRA material (fused q|k|v stacks, GEGLU row-interleaved stacks).  The
        convolutions' slot stacks (``Conv2d.lora_down`` / ``lora_up`` / ``w_slots``) are replaced by ``build`` / ``clear`` themselves
        and are no part of ``Conv2d._packed``: the base convs' packed weights keep their form and their pointers.  Graphs that hold
        pointers of the old stacks are dropped through ``version`` (engines) and the pointer epoch."""
        for m in self.unet.modules():
            if isinstance(m, (GEGLU, Attention)):
                m.invalidate_packed()
            elif isinstance(m, Linear):
                m.invalidate_mx8_slots()

    def clear(self) -> None:
        had_conv = False
        for m in self.unet.modules():
            if isinstance(m, Linear):
                m.lora_down = m.lora_up = m.w_slots = None
            elif isinstance(m, Conv2d):
                had_conv |= m.has_lora_slots()
                m.lora_down = m.lora_up = m.w_slots = None
                m.drop_slot_phase()
        if had_conv:      # captured graphs hold the freed conv stacks' pointers (and, in fp8 mode, took the other kernel)
            bump_pointer_epoch()
        self._invalidate_packed()
