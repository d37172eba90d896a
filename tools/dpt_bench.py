#!/usr/bin/env python
"""A/B of the DPT-hybrid depth estimator at full width (dpt-hybrid-midas's config, seeded synthetic weights, 384 x 384, batch 1):
omg_amd.DPTForDepthEstimation against a per-layer torch evaluation of the SAME weights on the same device in fp16 — tests/dpt_torch.py's
module moved to the device: F.conv2d with the weight standardised on every call (as transformers' BiT does), F.group_norm,
F.max_pool2d, F.linear, softmax attention, F.interpolate.

    python tools/dpt_bench.py [--log profiles/dpt_bench.log] [--calls 10] [--timeout 600]

2 warm-up calls of each path, then two interleaved rounds (torch, HIP, torch, HIP) of ``--calls`` synchronised calls each; per round
the median is reported.  Also timed: ``depth_condition`` (image processor on the host, the estimator, omg_depth_tail to 1024 x 1024)
and its device part alone.  The log says what was measured; nothing is asserted about which path is faster.  The tool ends itself
after ``--timeout`` seconds.
"""
import argparse
import os
import signal
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from omg_amd import dpt as hip_dpt
from omg_amd import ops
from tests import dpt_torch as dt


def timed(fn, calls):
    ts = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=None)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--seed", type=int, default=31)
    a = ap.parse_args()
    signal.alarm(a.timeout)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda:0")
    cfg = dt.full_cfg()
    oracle = dt.seed_state(dt.DPTHybrid(cfg).eval(), a.seed)
    hip = hip_dpt.DPTForDepthEstimation(dt.hf_config_dict(cfg), dtype=torch.float16, device=dev)
    hip.load_state_dict(oracle.state_dict(), strict=True)
    hip.eval()
    ref = oracle.half().to(dev)
    x = dt.seeded_input(7, 1, 384).to(dev)
    xh = x.half()
    say(f"# dpt_bench: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, dpt-hybrid-midas config, seed {a.seed}, 384 x 384, batch 1, fp16, {a.calls} calls per round")

    def run_torch():
        with torch.no_grad():
            return ref(xh)

    def run_hip():
        return hip(x).predicted_depth

    for _ in range(2):
        run_torch()
        run_hip()
    with torch.no_grad():
        d_t, d_h = run_torch().float(), run_hip()
    say(f"predicted_depth: HIP against the torch fp16 evaluation, rms difference / rms {dt.rel_rms(d_h.cpu(), d_t.cpu()):.3e}")
    for r in range(2):
        mt, bt = timed(run_torch, a.calls)
        mh, bh = timed(run_hip, a.calls)
        say(f"round {r}: torch per-layer fp16 median {mt:.3f} ms (best {bt:.3f})   HIP median {mh:.3f} ms (best {bh:.3f})   torch / HIP {mt / mh:.2f}")

    proc = hip_dpt.DPTImageProcessor()
    img = np.random.RandomState(1).randint(0, 256, (768, 1024, 3), dtype=np.uint8)
    for _ in range(2):
        hip_dpt.depth_condition(hip, proc, img)
    for r in range(2):
        mc, bc = timed(lambda: hip_dpt.depth_condition(hip, proc, img), a.calls)
        md, bd = timed(lambda: ops.depth_tail(hip(x).predicted_depth, (1024, 1024)), a.calls)
        mtail, btail = timed(lambda: ops.depth_tail(d_h, (1024, 1024)), a.calls)
        say(f"round {r}: depth_condition (768 x 1024 image -> 1024 x 1024, host resize and copies included) median {mc:.3f} ms (best {bc:.3f});"
            f"   estimator + omg_depth_tail {md:.3f} ms (best {bd:.3f});   omg_depth_tail alone {mtail:.3f} ms (best {btail:.3f})")
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
