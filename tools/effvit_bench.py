#!/usr/bin/env python
"""A/B of the EfficientViT-SAM l0 image encoder at 512 x 512: this package's module (omg_amd/efficientvit.py) against a per-layer
fallback (every convolution F.conv2d in fp16 on the GPU with the same folded weights, LiteMLA as the HIP module; tests/effvit_torch.py).

    python tools/effvit_bench.py [--log profiles/r10_effvit_ab.log] [--batches 1 8]
    python tools/effvit_bench.py --profile-run        one warm-up and three calls of the module at batch 1, nothing else: the
                                                      program to put behind `rocprofv3 --kernel-trace --stats --`

Per batch size: seeded weights, 3 warm-up calls of each path, then fallback / new / fallback / new ... interleaved, 7 synchronised
calls each, the median reported.  No speed-up is promised by either side; the log says what was measured.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

from omg_amd.efficientvit import EfficientViTSamImageEncoder
from tests.effvit_torch import TorchEncoder, seed_encoder


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=None)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--profile-run", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    m = EfficientViTSamImageEncoder("l0", dtype=torch.float16, device=dev)
    seed_encoder(m, 30)
    if a.profile_run:
        x = torch.randn(1, 3, 512, 512, device=dev).half()
        for _ in range(4):
            m(x)
        torch.cuda.synchronize()
        return
    fb = TorchEncoder(m, rounded=True)
    lines = [f"EfficientViT-SAM l0 image encoder, 512x512, fp16, {torch.cuda.get_device_name(0)}; median of {a.calls} synchronised calls, interleaved"]
    for B in a.batches:
        x = torch.randn(B, 3, 512, 512, device=dev, generator=torch.Generator(device=dev).manual_seed(B)).half()
        new = lambda: m(x)
        old = lambda: fb.features(x)["out"]
        for _ in range(3):
            old(); new()
        t_old, t_new = [], []
        for _ in range(a.calls):
            t_old.append(timed(old))
            t_new.append(timed(new))
        mo, mn = statistics.median(t_old), statistics.median(t_new)
        lines.append(f"batch {B}: per-layer fallback {mo:.3f} ms  (min {min(t_old):.3f}, max {max(t_old):.3f});  "
                     f"HIP module {mn:.3f} ms  (min {min(t_new):.3f}, max {max(t_new):.3f});  fallback / module = {mo / mn:.2f}")
    text = "\n".join(lines)
    print(text)
    if a.log:
        with open(a.log, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
