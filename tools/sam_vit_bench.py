#!/usr/bin/env python
"""A/B of SAM's ViT image encoder and of the whole segmenter call at full width: omg_amd.segment_anything (vit_b / vit_l / vit_h, seeded
synthetic weights) against a per-layer torch evaluation of the SAME weights on the same device in fp16 — F.linear, F.layer_norm,
F.pad + window partition, the decomposed relative-position bias materialised as the attn_mask of F.scaled_dot_product_attention (what
the reference runs: a [heads, 4096, 4096] bias per global layer), the decoder as tests/sam_torch.py's classes moved to the device.

    python tools/sam_vit_bench.py [--variants vit_b vit_l vit_h] [--log profiles/sam_vit_ab.log] [--timeout 900]

Per variant: 2 warm-up calls of each path, then two interleaved rounds (torch, HIP, torch, HIP, ...) of ``--calls`` synchronised
calls each; per round the median is reported.  Timed: ``image_encoder`` on a preprocessed 1024 x 1024 input (batch 1), and
``set_image`` + ``predict_torch`` for one and for eight boxes.  The criterion the log answers: the HIP encoder of vit_h is not slower
than the torch evaluation in both rounds.  Nothing is tuned toward it; the log says what was measured.  The tool ends itself after
``--timeout`` seconds.
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

import numpy as np
import torch
import torch.nn.functional as F

from omg_amd import segment_anything as sa
from tests import sam_torch as st


def seed_model(model, seed):
    """Seeded synthetic weights, drawn on the device: matrices at 1 / sqrt(fan_in), norms near 1, small biases, pos_embed at 0.5."""
    g = torch.Generator(device=model.device).manual_seed(seed)
    with torch.no_grad():
        for key, t in model.state_dict().items():
            if not t.dtype.is_floating_point:
                continue
            z = torch.randn(t.shape, generator=g, device=t.device, dtype=torch.float32)
            if key.endswith("pos_embed"):
                v = 0.5 * z
            elif "norm" in key or ".neck.1." in key or ".neck.3." in key or "output_upscaling.1." in key or "mask_downscaling.1." in key or "mask_downscaling.4." in key:
                v = 1.0 + 0.2 * z if key.endswith("weight") else 0.1 * z
            elif key.endswith("bias"):
                v = 0.1 * z
            elif t.dim() < 2 or "gaussian_matrix" in key or "embed" in key or "token" in key:
                v = z
            elif "output_upscaling" in key:
                v = z / math.sqrt(t.shape[0])
            else:
                v = z / math.sqrt(t[0].numel())
            t.copy_(v.to(t.dtype))


class TorchViT:
    """The encoder of ``model`` evaluated layer by layer by torch, in the storage dtype, on the module's own parameters."""

    def __init__(self, enc):
        self.e = enc

    def attention(self, a, x):
        B, H, W, C = x.shape
        nh = a.num_heads
        qkv = F.linear(x, a.qkv.weight, a.qkv.bias).reshape(B, H * W, 3, nh, -1).permute(2, 0, 3, 1, 4)
        q, k, v = qkv[0], qkv[1], qkv[2]
        iy, ix = torch.arange(H, device=x.device), torch.arange(W, device=x.device)
        qg = q.reshape(B, nh, H, W, -1)
        bh = torch.einsum("bnhwc,hkc->bnhwk", qg, a.rel_pos_h[iy[:, None] - iy[None, :] + H - 1])
        bw = torch.einsum("bnhwc,wkc->bnhwk", qg, a.rel_pos_w[ix[:, None] - ix[None, :] + W - 1])
        bias = (bh[..., :, None] + bw[..., None, :]).reshape(B, nh, H * W, H * W)
        o = F.scaled_dot_product_attention(q, k, v, attn_mask=bias)
        return F.linear(o.view(B, nh, H, W, -1).permute(0, 2, 3, 1, 4).reshape(B, H, W, C), a.proj.weight, a.proj.bias)

    @torch.no_grad()
    def __call__(self, x):
        e = self.e
        D = e.embed_dim
        x = F.conv2d(x, e.patch_embed.proj.weight, e.patch_embed.proj.bias, stride=e.patch_size).permute(0, 2, 3, 1) + e.pos_embed
        for blk in e.blocks:
            y = F.layer_norm(x, (D,), blk.norm1.weight, blk.norm1.bias, 1e-6)
            S = blk.window_size
            if S:
                B, H, W, C = y.shape
                ph, pw = (S - H % S) % S, (S - W % S) % S
                y = F.pad(y, (0, 0, 0, pw, 0, ph))
                Hp, Wp = H + ph, W + pw
                y = y.view(B, Hp // S, S, Wp // S, S, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, S, S, C)
                y = self.attention(blk.attn, y)
                y = y.view(B, Hp // S, Wp // S, S, S, C).permute(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, C)[:, :H, :W]
            else:
                y = self.attention(blk.attn, y)
            x = x + y
            y = F.layer_norm(x, (D,), blk.norm2.weight, blk.norm2.bias, 1e-6)
            x = x + F.linear(F.gelu(F.linear(y, blk.mlp.lin1.weight, blk.mlp.lin1.bias)), blk.mlp.lin2.weight, blk.mlp.lin2.bias)
        n = e.neck
        t = F.conv2d(x.permute(0, 3, 1, 2), n[0].weight)
        t = F.layer_norm(t.permute(0, 2, 3, 1), (e.out_chans,), n[1].weight, n[1].bias, 1e-6).permute(0, 3, 1, 2)
        t = F.conv2d(t, n[2].weight, padding=1)
        return F.layer_norm(t.permute(0, 2, 3, 1), (e.out_chans,), n[3].weight, n[3].bias, 1e-6).permute(0, 3, 1, 2)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", nargs="+", default=["vit_b", "vit_l", "vit_h"])
    ap.add_argument("--log", default=None)
    ap.add_argument("--boxes", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=900)
    a = ap.parse_args()
    signal.alarm(a.timeout)
    dev = torch.device("cuda:0")
    image = np.random.RandomState(0).randint(0, 256, (1024, 1024, 3)).astype(np.uint8)
    rs = np.random.RandomState(1)
    lines = [f"SAM ViT, 1024x1024 image, fp16, {torch.cuda.get_device_name(0)}; medians of {a.calls} synchronised calls, two interleaved rounds"]

    def emit(s):
        lines.append(s)
        print(s, flush=True)
        if a.log:
            with open(a.log, "w") as f:
                f.write("\n".join(lines) + "\n")

    print(lines[0], flush=True)
    for variant in a.variants:
        model = sa.sam_model_registry[variant](device=dev)
        seed_model(model, 30)
        pred = sa.SamPredictor(model)
        tv = TorchViT(model.image_encoder)
        pe, md = st.build()
        pe.load_state_dict({k: v.float().cpu() for k, v in model.prompt_encoder.state_dict().items()})
        md.load_state_dict({k: v.float().cpu() for k, v in model.mask_decoder.state_dict().items()})
        md16 = md.half().to(dev)
        dense_pe16 = pe.get_dense_pe().half().to(dev)
        x = model.preprocess(torch.from_numpy(image).permute(2, 0, 1)[None].to(dev)).half()
        old = lambda: tv(x)
        new = lambda: model.image_encoder(x)
        for _ in range(2):
            old(); new()
        ref, got = old().float(), new().float()
        rel = ((got - ref).abs().max() / ref.pow(2).mean().sqrt()).item()
        r = rounds(old, new, a.calls)
        verdict = "not slower in both rounds" if all(n <= o for o, n in r) else "SLOWER in at least one round"
        emit(f"{variant} image_encoder (batch 1): " + "; ".join(f"round {i + 1}: per-layer torch {o:.2f} ms, HIP {n:.2f} ms, torch / HIP = {o / n:.2f}" for i, (o, n) in enumerate(r))
             + f"; HIP is {verdict}; max |d| / rms between the two embeddings {rel:.2e}")
        for nb in a.boxes:
            xy = rs.uniform(0, 500, (nb, 2))
            boxes_np = np.concatenate([xy, xy + rs.uniform(100, 500, (nb, 2))], axis=1)

            def new_call():
                pred.set_image(image)
                boxes = pred.transform.apply_boxes_torch(torch.as_tensor(boxes_np, device=dev), image.shape[:2])
                return pred.predict_torch(point_coords=None, point_labels=None, boxes=boxes, multimask_output=False)

            def old_call():
                resized = pred.transform.apply_image(image)
                xi = model.preprocess(torch.as_tensor(resized, device=dev).permute(2, 0, 1).contiguous()[None]).half()
                feat = tv(xi)
                with torch.no_grad():
                    sparse, dense = pe(points=None, boxes=torch.as_tensor(pred.transform.apply_boxes(boxes_np, image.shape[:2]), dtype=torch.float), masks=None)
                    low, iou = md16(feat, dense_pe16, sparse.half().to(dev), dense[:1].half().to(dev), False)
                    masks = st.postprocess_masks(low.float(), 1024, tuple(resized.shape[:2]), image.shape[:2]) > model.mask_threshold
                return masks, iou, low

            for _ in range(2):
                old_call(); new_call()
            agree = (old_call()[0] == new_call()[0]).float().mean().item()
            r = rounds(old_call, new_call, a.calls)
            emit(f"{variant} set_image + predict_torch, {nb} box(es): " + "; ".join(f"round {i + 1}: per-layer torch {o:.2f} ms, HIP {n:.2f} ms, torch / HIP = {o / n:.2f}" for i, (o, n) in enumerate(r))
                 + f"; mask pixels equal on both paths: {100 * agree:.2f} %")
        del model, pred, tv, md16, x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
