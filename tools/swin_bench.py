#!/usr/bin/env python
"""A/B of the Swin backbone at GroundingDINO's width: omg_amd.SwinBackbone (Swin-B: embed 128, depths 2 / 2 / 18 / 2, heads 4 / 8 / 16 /
32, window 12; seeded synthetic weights, fp16, batch 1) against a per-layer torch evaluation of the SAME weights on the same device in
fp16 — F.layer_norm, F.pad, torch.roll, window partition, F.linear, F.scaled_dot_product_attention with the materialised
[windows, heads, 144, 144] bias + mask as its attn_mask, window reverse, roll back, crop.  The region mask of a grid size is built once
and kept (the library rebuilds it every call); the bias gather from the table and its sum with the mask happen in every call, as in
the library.

    python tools/swin_bench.py [--sizes 800x800 800x1200] [--log profiles/swin_bench.log] [--timeout 900]

Per input size: 2 warm-up calls of each path, then two interleaved rounds (torch, HIP, torch, HIP, ...) of ``--calls`` synchronised
calls each; per round the median is reported.  Then the attention alone — omg_attn_swin on fused QKV rows against the torch
composition from the same rows — at the four stage shapes of the first size, unshifted and shifted.  No ratio is a criterion: the log
says what was measured, and says so plainly where the HIP path loses.  The tool ends itself after ``--timeout`` seconds.
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

from omg_amd import ops
from omg_amd.swin import SwinBackbone

SWIN_B = dict(model_type="swin", embed_dim=128, depths=[2, 2, 18, 2], num_heads=[4, 8, 16, 32], window_size=12, mlp_ratio=4.0, qkv_bias=True,
              hidden_act="gelu", patch_size=4, num_channels=3, layer_norm_eps=1e-5, out_features=["stage2", "stage3", "stage4"])


def seed_model(model, seed):
    """Seeded synthetic weights, drawn on the device: matrices at 1 / sqrt(fan_in), norms near 1, small biases, bias tables at 1."""
    g = torch.Generator(device=model._device).manual_seed(seed)
    sd = {}
    for key, t in model.state_dict().items():
        z = torch.randn(t.shape, generator=g, device=t.device, dtype=torch.float32)
        if key.endswith("relative_position_bias_table"):
            v = z
        elif "norm" in key and t.dim() == 1:
            v = 1.0 + 0.2 * z if key.endswith("weight") else 0.1 * z
        elif key.endswith("bias"):
            v = 0.1 * z
        else:
            v = z / math.sqrt(t[0].numel())
        sd[key] = v
    model.load_state_dict(sd, strict=True)


def partition(x, S):
    B, H, W, C = x.shape
    return x.view(B, H // S, S, W // S, S, C).transpose(2, 3).reshape(-1, S * S, C)


def reverse(w, S, H, W):
    C = w.shape[-1]
    return w.view(-1, H // S, W // S, S, S, C).transpose(2, 3).reshape(-1, H, W, C)


class TorchSwin:
    """The backbone of ``model`` evaluated layer by layer by torch, in the storage dtype, on the module's own parameters."""

    def __init__(self, model):
        self.m, self.w, self.pk = model, model._w, model._pk()
        S = model.cfg["window_size"]
        c = torch.stack(torch.meshgrid([torch.arange(S), torch.arange(S)], indexing="ij")).flatten(1)
        rel = c[:, :, None] - c[:, None, :]
        self.index = ((rel[0] + S - 1) * (2 * S - 1) + rel[1] + S - 1).view(-1).to(model._device)
        self.masks = {}

    def mask(self, Hp, Wp, S, shift, dtype, dev):
        key = (Hp, Wp, shift)
        if key not in self.masks:
            hi, wi = torch.arange(Hp, device=dev), torch.arange(Wp, device=dev)
            hr = (hi >= Hp - S).long() + (hi >= Hp - shift).long()
            wr = (wi >= Wp - S).long() + (wi >= Wp - shift).long()
            mw = partition((hr[None, :, None, None] * 3 + wr[None, None, :, None]).to(dtype), S).view(-1, S * S)
            d = mw.unsqueeze(1) - mw.unsqueeze(2)
            self.masks[key] = torch.where(d != 0, torch.full_like(d, -100.0), torch.zeros_like(d))
        return self.masks[key]

    def windows(self, full, S, shift, heads, table):
        """[1, Hp, Wp, 3 C] fused q | k | v of the padded grid -> [1, Hp, Wp, C]: roll, partition, SDPA with bias + mask, reverse, roll."""
        _, Hp, Wp, C3 = full.shape
        C = C3 // 3
        if shift:
            full = torch.roll(full, shifts=(-shift, -shift), dims=(1, 2))
        win = partition(full, S)
        nW, N = win.shape[:2]
        q, k, v = win.view(nW, N, 3, heads, C // heads).permute(2, 0, 3, 1, 4)
        bias = table[self.index].view(N, N, heads).permute(2, 0, 1)[None]
        if shift:
            bias = bias + self.mask(Hp, Wp, S, shift, full.dtype, full.device)[:, None]
        else:
            bias = bias.expand(nW, -1, -1, -1)
        o = F.scaled_dot_product_attention(q, k, v, attn_mask=bias)
        o = reverse(o.transpose(1, 2).reshape(nW, N, C), S, Hp, Wp)
        return torch.roll(o, shifts=(shift, shift), dims=(1, 2)) if shift else o

    def attention_from_rows(self, qkv, H, W, S, shift, heads, table, pad_kv):
        """The attention alone, from the fused QKV rows of the H x W grid (what omg_attn_swin reads): padded positions get k | v = pad_kv."""
        C = qkv.shape[1] // 3
        Hp, Wp = -(-H // S) * S, -(-W // S) * S
        full = torch.cat([torch.zeros(C, dtype=qkv.dtype, device=qkv.device), pad_kv]).expand(1, Hp, Wp, 3 * C).clone()
        full[0, :H, :W] = qkv.view(H, W, 3 * C)
        return self.windows(full, S, shift, heads, table)[:, :H, :W].reshape(H * W, C)

    @torch.no_grad()
    def __call__(self, x):
        m, w, pk, c = self.m, self.w, self.pk, self.m.cfg
        S, eps = c["window_size"], c["layer_norm_eps"]
        P = "swin.embeddings."
        x = F.pad(x, (0, (4 - x.shape[3] % 4) % 4, 0, (4 - x.shape[2] % 4) % 4))
        t = F.conv2d(x, w[P + "patch_embeddings.projection.weight"], w[P + "patch_embeddings.projection.bias"], stride=4)
        B, E, H, W = t.shape
        t = F.layer_norm(t.flatten(2).transpose(1, 2), (E,), w[P + "norm.weight"], w[P + "norm.bias"], 1e-5)
        maps = []
        n = len(c["depths"])
        for li, (depth, heads) in enumerate(zip(c["depths"], c["num_heads"])):
            C = E << li
            for bi in range(depth):
                p = f"swin.encoder.layers.{li}.blocks.{bi}."
                a = p + "attention."
                y = F.layer_norm(t, (C,), w[p + "layernorm_before.weight"], w[p + "layernorm_before.bias"], eps).view(B, H, W, C)
                y = F.pad(y, (0, 0, 0, (S - W % S) % S, 0, (S - H % S) % S))
                o = self.windows(F.linear(y, pk[a + "qkv.weight"], pk[a + "qkv.bias"]), S, 0 if bi % 2 == 0 else S // 2, heads,
                                 w[a + "relative_position_bias.relative_position_bias_table"])[:, :H, :W].reshape(B, H * W, C)
                t = t + F.linear(o, w[a + "o_proj.weight"], w[a + "o_proj.bias"])
                y = F.layer_norm(t, (C,), w[p + "layernorm_after.weight"], w[p + "layernorm_after.bias"], eps)
                t = t + F.linear(F.gelu(F.linear(y, w[p + "mlp.fc1.weight"], w[p + "mlp.fc1.bias"])), w[p + "mlp.fc2.weight"], w[p + "mlp.fc2.bias"])
            st = f"stage{li + 1}"
            if st in c["out_features"]:
                f = F.layer_norm(t, (C,), w[f"hidden_states_norms.{st}.weight"], w[f"hidden_states_norms.{st}.bias"], 1e-5)
                maps.append(f.view(B, H, W, C).permute(0, 3, 1, 2))
            if li < n - 1:
                p = f"swin.encoder.layers.{li}.downsample."
                g = F.pad(t.view(B, H, W, C), (0, 0, 0, W % 2, 0, H % 2))
                g = torch.cat([g[:, r::2, cc::2] for cc in range(2) for r in range(2)], dim=-1).view(B, -1, 4 * C)
                t = F.linear(F.layer_norm(g, (4 * C,), w[p + "norm.weight"], w[p + "norm.bias"], 1e-5), w[p + "reduction.weight"])
                H, W = (H + 1) // 2, (W + 1) // 2
        return tuple(maps)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["800x800", "800x1200"])
    ap.add_argument("--log", default=None)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=900)
    a = ap.parse_args()
    signal.alarm(a.timeout)
    dev = torch.device("cuda:0")
    lines = [f"Swin-B backbone (GroundingDINO), fp16, batch 1, {torch.cuda.get_device_name(0)}; medians of {a.calls} synchronised calls, two interleaved rounds"]

    def emit(s):
        lines.append(s)
        print(s, flush=True)
        if a.log:
            with open(a.log, "w") as f:
                f.write("\n".join(lines) + "\n")

    print(lines[0], flush=True)
    model = SwinBackbone(SWIN_B, dtype=torch.float16, device=dev)
    seed_model(model, 30)
    tv = TorchSwin(model)
    sizes = [tuple(int(v) for v in s.split("x")) for s in a.sizes]
    for H, W in sizes:
        x = torch.randn(1, 3, H, W, generator=torch.Generator().manual_seed(1)).to(dev).half()
        old = lambda: tv(x)                            # noqa: E731
        new = lambda: model(x).feature_maps            # noqa: E731
        for _ in range(2):
            old(); new()
        rel = max(((g.float() - r.float()).abs().max() / r.float().pow(2).mean().sqrt()).item() for g, r in zip(new(), old()))
        emit(f"backbone {H} x {W}: " + fmt(rounds(old, new, a.calls)) + f"; max |d| / rms between the two paths' feature maps {rel:.2e}")
    H0, W0 = (sizes[0][0] + 3) // 4, (sizes[0][1] + 3) // 4
    S = 12
    for li, heads in enumerate(SWIN_B["num_heads"]):
        H, W, C = H0, W0, 128 << li
        g = torch.Generator(device=dev).manual_seed(li)
        qkv = torch.randn(H * W, 3 * C, generator=g, device=dev).half()
        table = torch.randn((2 * S - 1) ** 2, heads, generator=g, device=dev).half()
        pad = torch.randn(2 * C, generator=g, device=dev).half()
        out = torch.empty(H * W, C, dtype=torch.float16, device=dev)
        for shift in (0, S // 2):
            old = lambda: tv.attention_from_rows(qkv, H, W, S, shift, heads, table, pad)                                      # noqa: E731
            new = lambda: ops.attn_swin(qkv, 1, H, W, heads, table, 32 ** -0.5, window=S, shift=shift, pad_kv=pad, out=out)   # noqa: E731
            for _ in range(2):
                old(); new()
            rel = ((new().float() - old().float()).abs().max() / old().float().pow(2).mean().sqrt()).item()
            emit(f"attention alone, stage {li + 1}: grid {H} x {W}, {heads} heads, shift {shift}: " + fmt(rounds(old, new, 4 * a.calls)) + f"; max |d| / rms {rel:.2e}")
        H0, W0 = (H0 + 1) // 2, (W0 + 1) // 2


if __name__ == "__main__":
    main()
