#!/usr/bin/env python
"""What conv LoRA slots cost per launch: ``omg_conv2d`` with one shared weight (the path without conv LoRA) against ``omg_conv2d_slots`` with
three distinct weight slots (merged mode) and against the segment mode (LoRA-down conv + base conv with the second K-segment) at ranks 16 and
64, on the benchmark's own conv launch shapes at B = 8.  The modes are interleaved in one process; every figure is the median of ``--reps``
timings of ``--iters`` back-to-back launches between two events, after a warm-up.  One JSON line per shape; reported, not gated.

    python tools/conv_slots_bench.py [--dtype fp16] [--out profiles/conv_slots_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from omg_amd import _lib as L          # noqa: E402
from omg_amd import ops                # noqa: E402

# (name, H, W, C1, C2, Cout, stride)   — 3x3, B = 8: the resnet convs of the three resolutions, one concat (up block) and the stride-2 downsampler
SHAPES = [("128x128x320", 128, 128, 320, 0, 320, 1), ("64x64x640", 64, 64, 640, 0, 640, 1), ("32x32x1280", 32, 32, 1280, 0, 1280, 1),
          ("64x64 concat 1280+640 -> 640", 64, 64, 1280, 640, 640, 1), ("128x128x320 stride 2", 128, 128, 320, 0, 320, 2)]


def timed(fn, iters, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / iters * 1e3)      # us
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="fp16", choices=["fp16", "bf16"])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dt = torch.float16 if a.dtype == "fp16" else torch.bfloat16
    dev = torch.device("cuda:0")
    B = 8
    g = torch.Generator(device=dev).manual_seed(0)
    rows = []
    for name, H, W, C1, C2, Cout, stride in SHAPES:
        K = 9 * (C1 + C2)
        x1 = torch.randn(B, H, W, C1, generator=g, device=dev).to(dt)
        x2 = torch.randn(B, H, W, C2, generator=g, device=dev).to(dt) if C2 else None
        w = (torch.randn(4, Cout, K, generator=g, device=dev) * K ** -0.5).to(dt)          # base + three slots
        bias = torch.randn(Cout, generator=g, device=dev).to(dt)
        gb = torch.randn(B, Cout, generator=g, device=dev).to(dt)
        ids = torch.tensor([1, 2, 3, 1, 2, 3, 1, 2], dtype=torch.int32, device=dev)
        seg_ids = ids - 1
        w0 = w[0].contiguous()
        kw = dict(stride=stride, x2=x2, bias=bias, group_bias=gb)
        Ho, Wo = (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1
        modes = {"shared": lambda: ops.conv2d(x1, w0, 3, **kw), "slots": lambda: ops.conv2d(x1, w, 3, w_group_adapter=ids, **kw)}
        for r in (16, 64):
            down = (torch.randn(3, r, K, generator=g, device=dev) * K ** -0.5).to(dt)
            up = (torch.randn(3, Cout, r, generator=g, device=dev) * 0.1).to(dt)
            t = torch.empty(B, Ho, Wo, r, dtype=dt, device=dev)

            def seg(down=down, up=up, t=t):
                ops.conv2d(x1, down, 3, stride=stride, x2=x2, w_group_adapter=seg_ids, out=t)
                return ops.conv2d(x1, w0, 3, lora=ops.LoraSpec(t, up, seg_ids), **kw)
            modes[f"segment_r{r}"] = seg
        lib = L.lib()
        variant = {"shared": lib.omg_debug_choose_variant(B * Ho * Wo, 1, Cout, 1), "slots": lib.omg_debug_choose_variant(Ho * Wo, B, Cout, 1)}
        times = {m: [] for m in modes}
        for _ in range(2):                               # interleaved: every mode twice, alternating
            for m, fn in modes.items():
                times[m] += timed(fn, a.iters, a.reps)
        med = {m: statistics.median(v) for m, v in times.items()}
        flops = 2.0 * B * Ho * Wo * Cout * K
        row = dict(shape=name, dtype=a.dtype, B=B, variant=variant, us={m: round(v, 1) for m, v in med.items()},
                   spread_us={m: [round(min(v), 1), round(max(v), 1)] for m, v in times.items()},
                   tflops_shared=round(flops / med["shared"] / 1e6, 1),
                   ratio_vs_shared={m: round(v / med["shared"], 3) for m, v in med.items() if m != "shared"})
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
