#!/usr/bin/env python
"""A/B of the EfficientViT-SAM l0 image encoder at 512 x 512: this package's module (omg_amd/efficientvit.py) against a per-layer
fallback (every convolution F.conv2d in fp16 on the GPU with the same folded weights, LiteMLA as the HIP module; tests/effvit_torch.py).

    python tools/effvit_bench.py [--log profiles/r10_effvit_ab.log] [--batches 1 8]
    python tools/effvit_bench.py --profile-run        one warm-up and three calls of the module at batch 1, nothing else: the
                                                      program to put behind `rocprofv3 --kernel-trace --stats --`

    python tools/effvit_bench.py --variant xl1 [--log profiles/effvit_xl_bench.log]
                                                      xl0 | xl1 at 1024 x 1024, batch 1: the HIP path against the per-layer fallback,
                                                      the share of time per kernel family (ops.set_profiler), LiteMLA's aggregation
                                                      "fused" against "gemm" on xl1's two shapes, and the packed-weight bytes of both

Per batch size: seeded weights, 3 warm-up calls of each path, then fallback / new / fallback / new ... interleaved, 7 synchronised
calls each, the median reported.  The xl run does two such interleaved rounds (--calls each, default 3 there) and reports both.  No
speed-up is promised by either side; the log says what was measured.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

from omg_amd import ops
from omg_amd.efficientvit import EfficientViTSamConfig, EfficientViTSamImageEncoder
from omg_amd.litemla import LiteMLA
from tests.effvit_torch import TorchEncoder, seed_encoder


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def interleaved(old, new, calls, rounds=2):
    """[(median old, min, max, median new, min, max)] per round: old / new / old / new ..., synchronised calls."""
    out = []
    for _ in range(rounds):
        t_old, t_new = [], []
        for _ in range(calls):
            t_old.append(timed(old))
            t_new.append(timed(new))
        out.append((statistics.median(t_old), min(t_old), max(t_old), statistics.median(t_new), min(t_new), max(t_new)))
    return out


def derived_bytes(mods, params):
    """Device bytes of packed tensors that are not the module's own parameters (views of a parameter cost nothing)."""
    own = {p.untyped_storage().data_ptr() for p in params}
    seen, total = set(), 0
    for pk in mods:
        for v in pk.values():
            for t in (v if isinstance(v, list) else [v]):
                if torch.is_tensor(t) and t.untyped_storage().data_ptr() not in own and t.untyped_storage().data_ptr() not in seen:
                    seen.add(t.untyped_storage().data_ptr())
                    total += t.untyped_storage().nbytes()
    return total


def say(lines, text):
    lines.append(text)
    print(text, flush=True)


def aggreg_ab(lines, dev, calls):
    """LiteMLA's aggregation alone on xl1's two shapes: omg_litemla_aggreg against omg_dwconv2d + the block-diagonal omg_gemm, writing
    the same column slice of the same qkv buffer."""
    for (side, c) in ((32, 512), (16, 1024)):
        mods = {}
        for aggreg in ("gemm", "fused"):
            m = LiteMLA(c, c, dim=32, scales=(3,), dtype=torch.float16, device=dev, aggreg=aggreg)
            g = torch.Generator(device=dev).manual_seed(c)
            with torch.no_grad():
                for p in m.parameters():
                    p.copy_(torch.randn(p.shape, generator=g, device=dev) * 0.1)
            m.invalidate_packed()
            mods[aggreg] = m
        T3, M = 3 * c, side * side
        buf = (torch.randn(M, 2 * T3, device=dev, generator=torch.Generator(device=dev).manual_seed(1))).half()
        pg, pf = mods["gemm"]._pk(), mods["fused"]._pk()

        def run_gemm():
            t = ops.dwconv2d(buf[:, :T3], pg["taps"][0], 1, side, side, 3)
            ops.gemm(t, pg["wbd"][0], out=buf[:, T3:])

        def run_fused():
            ops.litemla_aggreg(buf[:, :T3], pf["taps"][0], pf["wg"][0], 1, side, side, 3, 32, out=buf[:, T3:])

        for _ in range(5):
            run_gemm(); run_fused()
        reps = 20

        def many(fn):
            return lambda: [fn() for _ in range(reps)]
        for r, (mo, lo, ho, mn, ln, hn) in enumerate(interleaved(many(run_gemm), many(run_fused), calls)):
            say(lines, f"aggregation {side}x{side} x {c} channels (3T = {T3}), round {r + 1}: dwconv2d + block-diagonal gemm {mo / reps * 1e3:.1f} us "
                         f"(min {lo / reps * 1e3:.1f}, max {ho / reps * 1e3:.1f});  litemla_aggreg {mn / reps * 1e3:.1f} us (min {ln / reps * 1e3:.1f}, "
                         f"max {hn / reps * 1e3:.1f});  gemm path / fused = {mo / mn:.2f}")
        bg = derived_bytes([pg], list(mods["gemm"].parameters()))
        bf = derived_bytes([pf], list(mods["fused"].parameters()))
        say(lines, f"aggregation {side}x{side} x {c}: packed-weight bytes of one LiteMLA block: gemm {bg} ({bg / 1e6:.2f} MB), fused {bf} ({bf / 1e6:.2f} MB)")


def xl_main(a, dev):
    cfg = getattr(EfficientViTSamConfig, a.variant)()
    m = EfficientViTSamImageEncoder(cfg, dtype=torch.float16, device=dev)
    seed_encoder(m, 30)
    x = torch.randn(1, 3, 1024, 1024, device=dev, generator=torch.Generator(device=dev).manual_seed(1)).half()
    calls = a.calls if a.calls is not None else 3
    lines = []
    say(lines, f"EfficientViT-SAM {a.variant} image encoder, 1024x1024, batch 1, fp16, {torch.cuda.get_device_name(0)}; seeded weights; "
             f"two interleaved rounds of {calls} synchronised calls, medians")
    fb = TorchEncoder(m, rounded=True)
    new = lambda: m(x)
    old = lambda: fb.features(x)["out"]
    for _ in range(2):
        old(); new()
    if not torch.isfinite(new()).all():
        say(lines, "note: seed_encoder's gains take this deeper model's activations past fp16's largest number in the neck, so the output is not "
                   "finite; the kernels do the same work on the same shapes either way")
    for r, (mo, lo, ho, mn, ln, hn) in enumerate(interleaved(old, new, calls)):
        say(lines, f"round {r + 1}: per-layer fallback {mo:.3f} ms  (min {lo:.3f}, max {ho:.3f});  HIP module {mn:.3f} ms  (min {ln:.3f}, max {hn:.3f});  "
                     f"fallback / module = {mo / mn:.2f}")
    prof = ops.KernelProfiler()
    ops.set_profiler(prof)
    new()
    torch.cuda.synchronize()
    ops.set_profiler(None)
    summ = prof.summary()
    total = sum(d["ms"] for d in summ.values())
    say(lines, f"kernel families of one profiled call (HIP events round every launch; layernorm and the layout permutes are not recorded): {total:.3f} ms in kernels")
    for kind, d in sorted(summ.items(), key=lambda kv: -kv[1]["ms"]):
        say(lines, f"  {kind:16s} {d['launches']:4d} launches  {d['ms']:9.3f} ms  {100 * d['ms'] / total:5.1f} %  {d['flops'] / 1e9:10.1f} GFLOP  "
                     f"{d['flops'] / max(d['ms'], 1e-9) / 1e9:8.1f} TFLOP/s")
    mlas = [l for l in m.modules() if isinstance(l, LiteMLA)]
    fused_bytes = derived_bytes([l._packed for l in mlas], list(m.parameters()))
    gemm_bytes = fused_bytes + sum(len(l.scales) * (3 * l.total_dim) ** 2 * 2 for l in mlas)
    say(lines, f"packed LiteMLA weights of the {len(mlas)} att@3 blocks of {a.variant}: fused {fused_bytes} bytes ({fused_bytes / 1e6:.1f} MB); "
                 f"with the block-diagonal images of the gemm path {gemm_bytes} bytes ({gemm_bytes / 1e6:.1f} MB)")
    del m, fb
    torch.cuda.empty_cache()
    aggreg_ab(lines, dev, calls)
    text = "\n".join(lines)
    if a.log:
        with open(a.log, "w") as f:
            f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=None)
    ap.add_argument("--variant", default="l0", choices=["l0", "xl0", "xl1"])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--calls", type=int, default=None)
    ap.add_argument("--profile-run", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.variant != "l0":
        return xl_main(a, dev)
    a.calls = 7 if a.calls is None else a.calls
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
