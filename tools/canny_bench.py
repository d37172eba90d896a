#!/usr/bin/env python
"""What the demos' Canny edge condition costs at 1024 x 1024 x 3 (``cv2.Canny(image, 100, 200)``), per input content, in two
interleaved rounds:

  hip eager     ``ops.canny``: five launches (omg_canny_nms, then the four of omg_canny_hysteresis) and two allocations;
  hip graph     the same call replayed from a ``torch.cuda.graph``;
  nms / hyst    the two entry points on their own (``ops.canny_nms``; ``ops.canny_hysteresis`` on its state map);
  torch         a composition of torch device ops: ``F.conv2d`` Sobel on the replicated pad, the non-maximum suppression as tensor
                expressions in int64, the hysteresis as repeated 3x3 ``max_pool2d`` dilation under the candidate mask to its fixpoint,
                with the host check (``torch.equal``) that ends the loop — its result must equal the kernels';
  host          the numpy model (``omg_amd.canny.canny_reference``) between a device-to-host and a host-to-device copy, wall time.

Device times: median of ``--reps`` timings of ``--iters`` back-to-back calls between two events.  The NMS kernel moves 4 bytes per pixel
(three read, one written); its time is stated against the memory time of those bytes at 6.3 TB/s, the copy rate this part reaches.
Contents: ``blur`` 5x5 box-blurred noise (dense candidates, many weak ones), ``shapes`` flat discs and boxes on a gradient (the sparse
edges of a picture), ``noise`` raw noise (every pixel a strong candidate: the hysteresis' worst case).
Reported, not gated.

    python tools/canny_bench.py > profiles/canny_bench.log
"""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from omg_amd import canny as cn                                                          # noqa: E402
from omg_amd import ops                                                                  # noqa: E402

HBM = 6.3e12


def make_image(kind, H, W, dev, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    if kind == "noise":
        return torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).to(dev)
    if kind == "blur":
        n = torch.randint(0, 256, (1, 3, H + 4, W + 4), generator=g).float()
        return F.avg_pool2d(n, 5, 1).floor()[0].permute(1, 2, 0).to(torch.uint8).contiguous().to(dev)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    img = torch.stack([(xx * 96 // W + 40), (yy * 96 // H + 60), ((xx + yy) * 48 // (H + W) + 80)], dim=2)
    for i in range(40):
        cy, cx, r = (int(torch.randint(0, v, (1,), generator=g)) for v in (H, W, max(min(H, W) // 6, 2)))
        col = torch.randint(0, 256, (3,), generator=g)
        m = ((yy - cy) ** 2 + (xx - cx) ** 2 < r * r) if i % 2 else ((yy - cy).abs() < r) & ((xx - cx).abs() < r // 2 + 1)
        img[m] = col
    return img.to(torch.uint8).contiguous().to(dev)


def torch_canny(u8, low, high):
    """cv2.Canny of a cuda uint8 [H, W, 3] image as torch device ops -> uint8 [H, W]; the loop's exit is a host check per sweep."""
    dev = u8.device
    x = u8.permute(2, 0, 1).float()[None]
    k = torch.tensor([[-1., 0., 1.], [-2., 0., 2.], [-1., 0., 1.]], device=dev)
    w = torch.stack([k, k.t()] * 3)[:, None]                        # [6, 1, 3, 3]: dx, dy per channel
    g = F.conv2d(F.pad(x, (1, 1, 1, 1), mode="replicate"), w, groups=3)[0].long()
    dx, dy = g[0::2], g[1::2]
    mag = dx.abs() + dy.abs()
    mag, ch = mag.max(dim=0, keepdim=True)                          # the first maximum
    dx, dy, mag = dx.gather(0, ch)[0], dy.gather(0, ch)[0], mag[0]
    H, W = mag.shape
    mp = F.pad(mag, (1, 1, 1, 1))
    nb = lambda oy, ox: mp[1 + oy:1 + oy + H, 1 + ox:1 + ox + W]
    ax, ay = dx.abs(), dy.abs() << 15
    t22 = ax * 13573
    t67 = t22 + (ax << 16)
    horiz, vert, same = ay < t22, ay > t67, (dx ^ dy) >= 0
    keep = torch.where(horiz, (mag > nb(0, -1)) & (mag >= nb(0, 1)),
           torch.where(vert, (mag > nb(-1, 0)) & (mag >= nb(1, 0)),
           torch.where(same, (mag > nb(-1, -1)) & (mag > nb(1, 1)), (mag > nb(-1, 1)) & (mag > nb(1, -1)))))
    keep &= mag > low
    cand = keep.float()[None, None]
    out = (keep & (mag > high)).float()[None, None]
    sweeps = 0
    while True:
        new = F.max_pool2d(out, 3, 1, 1) * cand
        sweeps += 1
        if torch.equal(new, out):
            break
        out = new
    return (out[0, 0] * 255).to(torch.uint8), sweeps


def device_us(fn, iters, reps):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1000 / iters)
    return statistics.median(times)


def wall_us(fn, reps):
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t) * 1e6)
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--host-reps", type=int, default=1)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    H = W = a.size
    mem_us = 4 * H * W / HBM * 1e6
    print(f"# cv2.Canny(image, 100, 200) at {H} x {W} x 3; memory time of the NMS kernel's 4 bytes per pixel at 6.3 TB/s: {mem_us:.2f} us")
    print("# us per call; device times between events, torch and host include their host side (wall time)")
    for kind in ("blur", "shapes", "noise"):
        u8 = make_image(kind, H, W, dev)
        state = ops.canny_nms(u8, 100, 200)
        edges = ops.canny(u8, 100, 200)
        ref, sweeps = torch_canny(u8, 100, 200)
        host = lambda: torch.from_numpy(cn.canny_reference(u8.cpu().numpy(), 100, 200)).to(dev)
        same_torch, same_host = torch.equal(ref, edges), torch.equal(host(), edges)
        print(f"# {kind}: {int((state == 1).sum())} weak, {int((state == 2).sum())} strong, {int((edges != 0).sum())} edge pixels; "
              f"torch composition equal: {same_torch} ({sweeps} dilation sweeps); numpy model equal: {same_host}")
        x = u8.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            ops.canny(x, 100, 200)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            ops.canny(x, 100, 200)
        for r in range(a.rounds):
            eager = device_us(lambda: ops.canny(u8, 100, 200), a.iters, a.reps)
            replay = device_us(graph.replay, a.iters, a.reps)
            nms = device_us(lambda: ops.canny_nms(u8, 100, 200), a.iters, a.reps)
            hyst = device_us(lambda: ops.canny_hysteresis(state, check=False), a.iters, a.reps)
            planar = device_us(lambda: ops.canny(u8, 100, 200, out_dtype=torch.float16), a.iters, a.reps)
            tor = wall_us(lambda: torch_canny(u8, 100, 200), 3)
            hst = wall_us(host, a.host_reps)
            print(f"{kind:>6} round {r}: hip eager {eager:8.1f} | hip graph {replay:8.1f} | nms {nms:7.1f} ({nms / mem_us:5.1f}x memory time) | "
                  f"hysteresis {hyst:8.1f} | eager, planar fp16 {planar:8.1f} | torch {tor:10.1f} ({tor / eager:6.1f}x eager) | "
                  f"host {hst:12.1f} ({hst / eager:8.1f}x eager)")


if __name__ == "__main__":
    main()
