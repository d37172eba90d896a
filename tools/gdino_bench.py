#!/usr/bin/env python
"""A/B of GroundingDINO's feature enhancer at full width: omg_amd.GroundingDinoEncoder (six layers, d_model 256, 8 heads, FFN 2048,
four levels, Swin-B's 256 / 512 / 1024 channels into the neck; seeded synthetic weights, fp16, batch 1) against a per-layer torch
evaluation of the SAME weights on the same device in fp16 — F.conv2d + F.group_norm for the neck, F.layer_norm / F.linear, the
library's grid_sample composition of the deformable attention (four grid_sample calls, a stack and a weighted sum), its materialised
bi-attention ([4, N, T] scores, the shifts and clamps, two softmaxes, two bmm), F.scaled_dot_product_attention with the phrase mask.
Masks, position embeddings and reference points are computed by the same torch code on both sides.

    python tools/gdino_bench.py [--sizes 800x800 800x1200] [--texts 16 256] [--log profiles/gdino_bench.log] [--timeout 900]

Per (image size, text length): 2 warm-up calls of each path, then two interleaved rounds (torch, HIP, torch, HIP, ...) of ``--calls``
synchronised calls each; per round the median is reported.  Then every new kernel alone at one layer's shape against its torch
composition.  No ratio is a criterion: the log says what was measured, and says so plainly where the HIP path loses.  The tool ends
itself after ``--timeout`` seconds.
"""
import argparse
import math
import os
import signal
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch
import torch.nn.functional as F

from omg_amd import gdino, ops

CFG = dict(d_model=256, encoder_attention_heads=8, encoder_ffn_dim=2048, encoder_n_points=4, num_feature_levels=4, encoder_layers=6,
           activation_function="relu", position_embedding_type="sine", positional_embedding_temperature=20, layer_norm_eps=1e-5,
           max_text_len=256, text_hidden=768, in_channels=[256, 512, 1024])


def seed_model(model, seed):
    """Seeded synthetic weights, drawn on the device: matrices at 1 / sqrt(fan_in) (offsets at 2 / sqrt), norms and layer scales near
    1, small biases (offset biases of 1.5 pixels)."""
    g = torch.Generator(device=model._device).manual_seed(seed)
    sd = {}
    for key, t in model.state_dict().items():
        z = torch.randn(t.shape, generator=g, device=t.device, dtype=torch.float32)
        if key.endswith("_param"):
            v = 1.0 + 0.2 * z
        elif key == "level_embed":
            v = z
        elif t.dim() == 1 and key.endswith("weight"):
            v = 1.0 + 0.2 * z
        elif key.endswith("bias"):
            v = (1.5 if "sampling_offsets" in key else 0.1) * z
        else:
            v = z * (2.0 if "sampling_offsets" in key else 1.0) / math.sqrt(t[0].numel())
        sd[key] = v
    model.load_state_dict(sd, strict=True)


def msdeform_torch(value, ow, ref, spatial, heads, keep):
    """The library's composition from the value_proj rows and the fused offsets | logits rows."""
    B, N, d = value.shape
    Nq, Lv, hd = ow.shape[1], len(spatial), d // heads
    if keep is not None:
        value = value.masked_fill(~keep[..., None], 0.0)
    value = value.view(B, N, heads, hd)
    off = ow[..., :heads * Lv * 8].view(B, Nq, heads, Lv, 4, 2)
    aw = F.softmax(ow[..., heads * Lv * 8:].view(B, Nq, heads, Lv * 4), -1)
    norm = torch.tensor([[w, h] for h, w in spatial], dtype=value.dtype, device=value.device)
    loc = ref.to(value.dtype)[:, :, None, :, None, :] + off / norm[None, None, None, :, None, :]
    grids = 2 * loc - 1
    vals = value.split([h * w for h, w in spatial], dim=1)
    sampled = []
    for l, (h, w) in enumerate(spatial):
        vl = vals[l].flatten(2).transpose(1, 2).reshape(B * heads, hd, h, w)
        gl = grids[:, :, :, l].transpose(1, 2).flatten(0, 1)
        sampled.append(F.grid_sample(vl, gl, mode="bilinear", padding_mode="zeros", align_corners=False))
    aw = aw.transpose(1, 2).reshape(B * heads, 1, Nq, Lv * 4)
    return (torch.stack(sampled, dim=-2).flatten(-2) * aw).sum(-1).view(B, heads * hd, Nq).transpose(1, 2).contiguous()


def bi_torch(vis, txt, heads, text_keep, vis_keep):
    """The library's materialised bi-attention from the fused rows vision q | v and text k | v -> (vision side, text side)."""
    B, N, E2 = vis.shape
    E, hd = E2 // 2, E2 // 2 // heads
    sh = lambda x: x.reshape(B, -1, heads, hd).transpose(1, 2).reshape(B * heads, -1, hd)
    q, vv, k, tv = sh(vis[..., :E] * hd ** -0.5), sh(vis[..., E:]), sh(txt[..., :E]), sh(txt[..., E:])
    a = torch.bmm(q, k.transpose(1, 2))
    a = torch.clamp(a - a.max(), min=-50000, max=50000)
    at = a.transpose(1, 2)
    ta = torch.clamp(at - torch.max(at, dim=-1, keepdim=True)[0], min=-50000, max=50000)
    if vis_keep is not None:
        ta = ta.masked_fill(~vis_keep[:, None, None, :].repeat(1, heads, 1, 1).flatten(0, 1), float("-inf"))
    ta = ta.softmax(dim=-1)
    if text_keep is not None:
        a = a.masked_fill(~text_keep[:, None, None, :].repeat(1, heads, 1, 1).flatten(0, 1), float("-inf"))
    va = a.softmax(dim=-1)
    ov = torch.bmm(va, tv).view(B, heads, N, hd).transpose(1, 2).reshape(B, N, E)
    ot = torch.bmm(ta, vv).view(B, heads, -1, hd).transpose(1, 2).reshape(B, -1, E)
    return ov, ot


def masked_torch(q, k, v, heads, keep):
    B, T, d = q.shape
    sh = lambda x: x.reshape(B, T, heads, d // heads).transpose(1, 2)
    return F.scaled_dot_product_attention(sh(q), sh(k), sh(v), attn_mask=keep[:, None]).transpose(1, 2).reshape(B, T, d)


class TorchGdino:
    """The neck and the encoder of ``model`` evaluated layer by layer by torch, in the storage dtype, on the module's own parameters."""

    def __init__(self, model):
        self.m, self.w, self.pk = model, model._w, model._pk()

    @torch.no_grad()
    def __call__(self, fms, text, token_keep, self_keep, position_ids):
        m, w, pk, c = self.m, self.w, self.pk, self.m.cfg
        d, eps, H8, dt = 256, c["eps"], 8, m.dtype
        B, T = text.shape[:2]
        maps = []
        for l in range(c["levels"]):
            P = f"input_proj_vision.{l}."
            if l < len(fms):
                y = F.conv2d(fms[l], w[P + "0.weight"], w[P + "0.bias"])
            else:
                y = F.conv2d(fms[-1] if l == len(fms) else maps[-1], w[P + "0.weight"], w[P + "0.bias"], stride=2, padding=1)
            maps.append(F.group_norm(y, 32, w[P + "1.weight"], w[P + "1.bias"], 1e-5))
        spatial = [tuple(x.shape[-2:]) for x in maps]
        v = torch.cat([x.flatten(2).transpose(1, 2) for x in maps], dim=1)
        masks = [torch.ones((B,) + s, dtype=torch.bool, device=v.device) for s in spatial]
        pos = torch.cat([gdino.sine_position(mk, d, c["temperature"]) + w["level_embed"][l].float().view(1, 1, -1) for l, mk in enumerate(masks)], 1).to(dt)
        vr = torch.ones(B, len(spatial), 2, device=v.device)
        ref = gdino.reference_points(spatial, vr)
        tpos = gdino.text_position(position_ids, d).to(dt)
        t = F.linear(text, w["text_projection.weight"], w["text_projection.bias"])
        for i in range(c["layers"]):
            p = f"encoder.layers.{i}."
            f = p + "fusion_layer."
            vn = F.layer_norm(v, (d,), w[f + "layer_norm_vision.weight"], w[f + "layer_norm_vision.bias"], eps)
            tn = F.layer_norm(t, (d,), w[f + "layer_norm_text.weight"], w[f + "layer_norm_text.bias"], eps)
            ov, ot = bi_torch(F.linear(vn, pk[f + "attn.vis.weight"], pk[f + "attn.vis.bias"]), F.linear(tn, pk[f + "attn.txt.weight"], pk[f + "attn.txt.bias"]),
                              H8 // 2, token_keep, None)
            v = vn + F.linear(ov, pk[f + "attn.out_vision.weight"], pk[f + "attn.out_vision.bias"])
            t = tn + F.linear(ot, pk[f + "attn.out_text.weight"], pk[f + "attn.out_text.bias"])
            e = p + "text_enhancer_layer."
            qk = F.linear(t + tpos, pk[e + "self_attn.qk.weight"], pk[e + "self_attn.qk.bias"])
            o = masked_torch(qk[..., :d], qk[..., d:], F.linear(t, w[e + "self_attn.value.weight"], w[e + "self_attn.value.bias"]), H8 // 2, self_keep)
            t = F.layer_norm(t + F.linear(o, w[e + "self_attn.out_proj.weight"], w[e + "self_attn.out_proj.bias"]), (d,),
                             w[e + "layer_norm_before.weight"], w[e + "layer_norm_before.bias"], eps)
            t = F.layer_norm(t + F.linear(F.relu(F.linear(t, w[e + "fc1.weight"], w[e + "fc1.bias"])), w[e + "fc2.weight"], w[e + "fc2.bias"]), (d,),
                             w[e + "layer_norm_after.weight"], w[e + "layer_norm_after.bias"], eps)
            s = p + "deformable_layer."
            ow = F.linear(v + pos, pk[s + "self_attn.ow.weight"], pk[s + "self_attn.ow.bias"])
            val = F.linear(v, w[s + "self_attn.value_proj.weight"], w[s + "self_attn.value_proj.bias"])
            a = msdeform_torch(val, ow, ref, spatial, H8, None)
            v = F.layer_norm(v + F.linear(a, w[s + "self_attn.output_proj.weight"], w[s + "self_attn.output_proj.bias"]), (d,),
                             w[s + "self_attn_layer_norm.weight"], w[s + "self_attn_layer_norm.bias"], eps)
            v = F.layer_norm(v + F.linear(F.relu(F.linear(v, w[s + "fc1.weight"], w[s + "fc1.bias"])), w[s + "fc2.weight"], w[s + "fc2.bias"]), (d,),
                             w[s + "final_layer_norm.weight"], w[s + "final_layer_norm.bias"], eps)
        return v, t


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def rounds(old, new, calls, n_rounds=2):
    out = []
    for _ in range(n_rounds):
        t_old, t_new = [], []
        for _ in range(calls):
            t_old.append(timed(old))
            t_new.append(timed(new))
        out.append((statistics.median(t_old), statistics.median(t_new)))
    return out


def fmt(r):
    verdict = "HIP is not slower in both rounds" if all(n <= o for o, n in r) else "HIP is SLOWER in at least one round"
    return "; ".join(f"round {i + 1}: per-layer torch {o:.3f} ms, HIP {n:.3f} ms, torch / HIP = {o / n:.2f}" for i, (o, n) in enumerate(r)) + "; " + verdict


def rel(a, b):
    return ((a.float() - b.float()).abs().max() / b.float().pow(2).mean().sqrt()).item()


def text_inputs(T, dev):
    g = torch.Generator().manual_seed(T)
    text = torch.randn(1, T, CFG["text_hidden"], generator=g).to(dev).half()
    keep = torch.ones(1, T, dtype=torch.bool, device=dev)
    self_keep = torch.eye(T, dtype=torch.bool, device=dev)[None].clone()
    pos = torch.zeros(1, T, dtype=torch.long, device=dev)
    s = 1
    while s < T - 1:                       # phrases of 7 tokens between separators
        e = min(T - 1, s + 7)
        self_keep[:, s:e, s:e] = True
        pos[:, s:e] = torch.arange(e - s, device=dev)
        s = e + 1
    return text, keep, self_keep, pos


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["800x800", "800x1200"])
    ap.add_argument("--texts", nargs="+", type=int, default=[16, 256])
    ap.add_argument("--log", default=None)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=900)
    a = ap.parse_args()
    signal.alarm(a.timeout)
    dev = torch.device("cuda:0")
    lines = [f"GroundingDINO feature enhancer (neck + 6 layers), fp16, batch 1, {torch.cuda.get_device_name(0)}; medians of {a.calls} synchronised calls, two interleaved rounds"]

    def emit(s):
        lines.append(s)
        print(s, flush=True)
        if a.log:
            with open(a.log, "w") as f:
                f.write("\n".join(lines) + "\n")

    print(lines[0], flush=True)
    model = gdino.GroundingDinoEncoder(CFG, dtype=torch.float16, device=dev)
    seed_model(model, 30)
    tv = TorchGdino(model)
    sizes = [tuple(int(v) for v in s.split("x")) for s in a.sizes]
    for H, W in sizes:
        grids = [(-(-H // s), -(-W // s)) for s in (8, 16, 32)]
        g = torch.Generator().manual_seed(H + W)
        nhwc = [torch.randn(1, h, w, c, generator=g).to(dev).half() for c, (h, w) in zip(CFG["in_channels"], grids)]
        views = [x.permute(0, 3, 1, 2) for x in nhwc]                  # what SwinBackbone hands over: NCHW views of NHWC rows
        nchw = [x.contiguous() for x in views]                         # what torch's convolution wants
        for T in a.texts:
            text, keep, self_keep, pos = text_inputs(T, dev)
            old = lambda: tv(nchw, text, keep, self_keep, pos)                                                                        # noqa: E731
            new = lambda: model(views, None, text, keep, self_keep, pos)                                                             # noqa: E731
            for _ in range(2):
                old(); new()
            o, n = old(), new()
            N = n.last_hidden_state_vision.shape[1]
            emit(f"enhancer {H} x {W} (N = {N}), T = {T}: " + fmt(rounds(old, new, a.calls)) +
                 f"; max |d| / rms between the two paths: vision {rel(n.last_hidden_state_vision, o[0]):.2e}, text {rel(n.last_hidden_state_text, o[1]):.2e}")
    # ---- every new kernel alone, at one layer's shape of the last size
    H, W = sizes[-1]
    spatial = [(-(-H // s), -(-W // s)) for s in (8, 16, 32)]
    spatial.append(((spatial[-1][0] - 1) // 2 + 1, (spatial[-1][1] - 1) // 2 + 1))
    N = sum(h * w for h, w in spatial)
    g = torch.Generator(device=dev).manual_seed(5)
    value = torch.randn(1, N, 256, generator=g, device=dev).half()
    ow = torch.cat([torch.randn(1, N, 256, generator=g, device=dev) * 3.0, torch.randn(1, N, 128, generator=g, device=dev) * 2.0], -1).half()
    ref = gdino.reference_points(spatial, torch.ones(1, 4, 2, device=dev))
    out = torch.empty(1, N, 256, dtype=torch.float16, device=dev)
    old = lambda: msdeform_torch(value, ow, ref, spatial, 8, None)                                                                   # noqa: E731
    new = lambda: ops.msdeform_attn(value, ow, ref, spatial, heads=8, out=out)                                                       # noqa: E731
    for _ in range(2):
        old(); new()
    emit(f"deformable attention alone, N = {N}: " + fmt(rounds(old, new, 4 * a.calls)) + f"; max |d| / rms {rel(new(), old()):.2e}")
    for T in a.texts:
        vis = torch.randn(1, N, 2048, generator=g, device=dev).half()
        txt = torch.randn(1, T, 2048, generator=g, device=dev).half()
        old = lambda: bi_torch(vis, txt, 4, None, None)                                                                              # noqa: E731
        nv = lambda: ops.attn_bi_vision(vis, txt, 4, 256 ** -0.5)                                                                    # noqa: E731
        nt = lambda: ops.attn_bi_text(vis, txt, 4, 256 ** -0.5)                                                                      # noqa: E731
        new = lambda: (nv(), nt())                                                                                                   # noqa: E731
        for _ in range(2):
            old(); new()
        o, n = old(), new()
        emit(f"bi-attention alone (both sides), N = {N}, T = {T}: " + fmt(rounds(old, new, 4 * a.calls)) +
             f"; max |d| / rms vision {rel(n[0], o[0]):.2e}, text {rel(n[1], o[1]):.2e}; HIP vision side {statistics.median([timed(nv) for _ in range(9)]):.3f} ms, "
             f"text side {statistics.median([timed(nt) for _ in range(9)]):.3f} ms")
        _, _, self_keep, _ = text_inputs(T, dev)
        qk = torch.randn(1, T, 512, generator=g, device=dev).half()
        tvv = torch.randn(1, T, 256, generator=g, device=dev).half()
        old = lambda: masked_torch(qk[..., :256], qk[..., 256:], tvv, 4, self_keep)                                                   # noqa: E731
        new = lambda: ops.attn_masked(qk[..., :256], qk[..., 256:], tvv, 4, 0.125, mask=self_keep)                                    # noqa: E731
        for _ in range(2):
            old(); new()
        emit(f"masked text attention alone, T = {T}: " + fmt(rounds(old, new, 4 * a.calls)) + f"; max |d| / rms {rel(new(), old()):.2e}")


if __name__ == "__main__":
    main()
