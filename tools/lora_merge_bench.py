#!/usr/bin/env python
"""What building the weight slots of a LoRA bank costs: ``LoraBank.build`` for the benchmark's two-concept configuration (two slots of one
adapter each, scale 0.8) on the full-width UNet with seeded weights, three ways —

  (a) ``merge="torch"`` on plain rank-32 adapters: the fp32 torch expression ``W + up @ down`` per layer and slot (the default for plain pairs);
  (b) ``merge="hip"`` on the same adapters: every layer through ``omg_lora_merge``;
  (c) LoHa rank-16 adapters on the same targets through the kernel, against the same merge written out in torch fp32 inside this tool
      (``W + s (w1_a @ w1_b) * (w2_a @ w2_b)``, stacked and rounded once) —

in two interleaved rounds (wall time around a device synchronisation: the builds include their host side), and then, per distinct layer
shape, the kernel alone (median of ``--reps`` timings of ``--iters`` back-to-back launches between two events) against the memory time of
its ``4 N K`` bytes (W read once, the slot written once, 16 bits each) at 6.3 TB/s, the copy rate this part reaches of its 8 TB/s; last,
on the largest shape, a copy, the kernel without a term and plain terms of growing rank.
Reported, not gated.

    python tools/lora_merge_bench.py [--dtype fp16] [--tiny] > profiles/lora_merge_bench.log
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from omg_amd import _lib as L                                                            # noqa: E402
from omg_amd import ops                                                                  # noqa: E402
from omg_amd.lora import LoraAdapter, LoraBank, LoraTerm, lora_target_names, make_synthetic_adapter   # noqa: E402
from omg_amd.unet import UNet2DConditionModel, UNetConfig                               # noqa: E402

HBM = 6.3e12
SCALE = 0.8


def make_loha_adapter(unet, name, rank, seed):
    g = torch.Generator(device=unet.device).manual_seed(seed)
    terms = {}
    for key in lora_target_names(unet):
        lin = unet.get_submodule(key)
        rn = lambda *s: torch.randn(*s, generator=g, device=unet.device)
        terms[key] = LoraTerm("hada", {"hada_w1_a": rn(lin.out_features, rank) * 0.3, "hada_w1_b": rn(rank, lin.in_features) * lin.in_features ** -0.25,
                                       "hada_w2_a": rn(lin.out_features, rank) * 0.3, "hada_w2_b": rn(rank, lin.in_features) * lin.in_features ** -0.25}, alpha=rank / 2)
    return LoraAdapter(name, {}, terms=terms)


def torch_loha_build(unet, adapters, slots, scale):
    """The LoHa merge of (c) as a torch composition: fp32 dense products per layer and slot, one stack, one rounding."""
    out = {}
    for key in adapters[0].terms:
        lin = unet.get_submodule(key)
        base = lin.weight.data.float()
        rows = [base]
        for (name, w), in slots:
            t = next(a for a in adapters if a.name == name).terms[key]
            f = t.factors
            rows.append(base + (scale * w * t.factor) * ((f["hada_w1_a"] @ f["hada_w1_b"]) * (f["hada_w2_a"] @ f["hada_w2_b"])))
        out[key] = torch.stack(rows).to(lin.weight.dtype).contiguous()
    return out


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


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
    return statistics.median(out)


def launcher(w, terms, out):
    """One ``omg_lora_merge`` launch with its argument block built once: the loop times the kernel, not the Python that checks the shapes."""
    import ctypes
    args, fn, stream = ops.lora_merge_args(w, terms, out), L.lib().omg_lora_merge, torch.cuda.current_stream().cuda_stream
    return lambda: fn(ctypes.byref(args), stream)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="fp16", choices=["fp16", "bf16"])
    ap.add_argument("--tiny", action="store_true")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dt = torch.float16 if a.dtype == "fp16" else torch.bfloat16
    dev = torch.device("cuda:0")
    unet = UNet2DConditionModel(UNetConfig.tiny() if a.tiny else UNetConfig.sdxl(), dtype=dt, device=dev).init_synthetic_(seed=0)
    plain = [make_synthetic_adapter(unet, f"concept{c}", 32 if not a.tiny else 8, seed=1000 + c) for c in range(2)]
    loha = [make_loha_adapter(unet, f"loha{c}", 16 if not a.tiny else 4, seed=2000 + c) for c in range(2)]
    n_layers = len(plain[0].weights)
    elems = sum(unet.get_submodule(k).weight.numel() for k in plain[0].weights)
    print(f"# {a.dtype}, {'tiny' if a.tiny else 'full-width'} UNet: {n_layers} Linear targets, {elems / 1e6:.1f} M weight elements, 2 slots; "
          f"memory time of the two slots' 4 N K bytes at {HBM / 1e12:.1f} TB/s: {2 * 4 * elems / HBM * 1e3:.2f} ms")
    bank_p, bank_l = LoraBank(unet, plain), LoraBank(unet, loha)
    slots_p, slots_l = [(("concept0", 1.0),), (("concept1", 1.0),)], [(("loha0", 1.0),), (("loha1", 1.0),)]
    for rnd in range(2):
        t_a, _ = wall(lambda: bank_p.build(slots_p, scale=SCALE, merge="torch"))
        ref = {k: unet.get_submodule(k).w_slots for k in plain[0].weights}
        t_b, _ = wall(lambda: bank_p.build(slots_p, scale=SCALE, merge="hip"))
        diff = max((unet.get_submodule(k).w_slots.float() - ref[k].float()).abs().max().item() for k in ref)
        same = sum(torch.equal(unet.get_submodule(k).w_slots, ref[k]) for k in ref)
        del ref
        bank_p.clear()
        t_c, _ = wall(lambda: bank_l.build(slots_l, scale=SCALE))
        got = {k: unet.get_submodule(k).w_slots for k in loha[0].terms}
        t_ct, want = wall(lambda: torch_loha_build(unet, loha, slots_l, SCALE))
        diff_c = max((got[k].float() - want[k].float()).abs().max().item() for k in got)
        del got, want
        bank_l.clear()
        print(f"round {rnd}: (a) plain r32 merge=torch {t_a:8.1f} ms | (b) plain r32 merge=hip {t_b:8.1f} ms  (max |a - b| {diff:.2e}, {same}/{n_layers} stacks bitwise equal) | "
              f"(c) LoHa r16 kernel {t_c:8.1f} ms vs torch fp32 composition {t_ct:8.1f} ms  (max |d| {diff_c:.2e})")
    # ---- the kernel alone, per distinct layer shape
    shapes = sorted({(unet.get_submodule(k).out_features, unet.get_submodule(k).in_features) for k in plain[0].weights})
    print("# per shape, one slot: kernel us (x memory time) | the same merge as a torch fp32 composition, us")
    print(f"# {'N x K':>14} {'mem us':>8} | {'plain r32':>16} {'torch':>8} | {'hada r16':>16} {'torch':>8} | {'kron 4x8':>16} {'torch':>8} | {'hada r16 + gain':>16} {'rownorm':>8}")
    g = torch.Generator(device=dev).manual_seed(0)
    rn = lambda *s: torch.randn(*s, generator=g, device=dev)
    for N, K in shapes:
        w = (rn(N, K) * K ** -0.5).to(dt)
        out = torch.empty_like(w)
        mem = 4 * N * K / HBM * 1e6
        tp = {"kind": "plain", "f": (rn(N, 32), rn(32, K)), "s": 0.8}
        th = {"kind": "hada", "f": (rn(N, 16), rn(16, K), rn(N, 16), rn(16, K)), "s": 0.8}
        tk = {"kind": "kron", "f": (rn(4, 8), rn(N // 4, 1, K // 8)), "s": 0.8}
        thg = dict(th, gain=torch.rand(N, generator=g, device=dev) + 0.5)
        cells = []
        for t, comp in ((tp, lambda: (w.float() + 0.8 * (tp["f"][0] @ tp["f"][1])).to(dt)),
                        (th, lambda: (w.float() + 0.8 * ((th["f"][0] @ th["f"][1]) * (th["f"][2] @ th["f"][3]))).to(dt)),
                        (tk, lambda: (w.float() + 0.8 * torch.kron(tk["f"][0], tk["f"][1][:, 0, :])).to(dt))):
            us = timed(launcher(w, [t], out), a.iters, a.reps)
            cells.append(f"{us:8.1f} ({us / mem:4.1f}x) {timed(comp, a.iters, a.reps):8.1f}")
        us = timed(launcher(w, [thg], out), a.iters, a.reps)
        un = timed(lambda: ops.lora_rownorm(w, th), a.iters, a.reps)
        print(f"  {N:>6} x {K:<6} {mem:8.1f} | " + " | ".join(cells) + f" | {us:8.1f} ({us / mem:4.1f}x) {un:8.1f}")
    # ---- where the time goes, on the largest shape: a copy, the kernel without a term, and plain terms of growing rank
    N, K = max(shapes, key=lambda nk: nk[0] * nk[1])
    w = (rn(N, K) * K ** -0.5).to(dt)
    out = torch.empty_like(w)
    cells = [f"copy_ {timed(lambda: out.copy_(w), a.iters, a.reps):.1f}", f"no term {timed(launcher(w, [], out), a.iters, a.reps):.1f}"]
    for r in (1, 8, 32, 64):
        cells.append(f"plain r{r} {timed(launcher(w, [{'kind': 'plain', 'f': (rn(N, r), rn(r, K)), 's': 0.8}], out), a.iters, a.reps):.1f}")
    print(f"# rank sweep on {N} x {K} (memory time {4 * N * K / HBM * 1e6:.1f} us), us: " + " | ".join(cells))


if __name__ == "__main__":
    main()
