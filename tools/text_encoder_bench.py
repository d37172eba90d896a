#!/usr/bin/env python3
"""Wall time of `encode_prompt` on both SDXL text encoders at full width (CLIP-L: 12 layers x 12 heads, OpenCLIP-bigG: 32 x 20) with
synthetic weights, at B = 1 and B = 8 prompts: the median of synchronised calls after warm-up, one JSON line.

    python tools/text_encoder_bench.py [--iters 7] [--warmup 2] [--label new]

Public API only (ClipTextConfig / ClipTextEncoder / encode_prompt), so the same file measures any commit that has the encoders:
copy it into that checkout's tools/ and run it there.  encode_prompt lies outside bench.py's timed region; every pipeline call
pays it once per prompt batch."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def make(cfg, dev, seed):
    import torch
    from omg_amd.text_encoder import ClipTextEncoder
    enc = ClipTextEncoder(cfg, dtype=torch.float16, device=dev)
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in enc.state_dict().items():
        if "layer_norm" in k and k.endswith(".weight"):
            w = 1.0 + 0.1 * torch.randn(v.shape, generator=g)
        elif k.endswith(".bias"):
            w = 0.1 * torch.randn(v.shape, generator=g)
        elif "embedding" in k:
            w = 0.5 * torch.randn(v.shape, generator=g)
        else:
            w = torch.randn(v.shape, generator=g) * v.shape[-1] ** -0.5
        sd[k] = w.to(torch.float16).to(dev)
    enc.load_state_dict(sd)
    return enc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    import torch
    from omg_amd.text_encoder import ClipTextConfig, encode_prompt
    dev = torch.device("cuda:0")
    enc_l, enc_g = make(ClipTextConfig.clip_l(), dev, 1), make(ClipTextConfig.open_clip_bigg(), dev, 2)
    out = {"label": args.label, "iters": args.iters, "warmup": args.warmup}
    for B in (1, 8):
        g = torch.Generator().manual_seed(B)
        ids = torch.randint(2, 49000, (B, 77), generator=g)
        ids[:, 0] = 49406
        for b in range(B):
            ids[b, 5 + 9 * b:] = 49407
        ids = ids.to(dev)
        ts = []
        for it in range(args.warmup + args.iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            emb, pooled = encode_prompt(enc_l, enc_g, ids, ids)
            torch.cuda.synchronize()
            if it >= args.warmup:
                ts.append(time.perf_counter() - t0)
        assert emb.shape == (B, 77, 2048) and pooled.shape == (B, 1280) and bool(torch.isfinite(emb).all())
        out[f"B{B}_median_ms"] = round(1e3 * statistics.median(ts), 3)
        out[f"B{B}_min_ms"] = round(1e3 * min(ts), 3)
        out[f"B{B}_max_ms"] = round(1e3 * max(ts), 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
