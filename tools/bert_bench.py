#!/usr/bin/env python
"""GroundingDINO's BERT text encoder at full width (BERT-base: 12 layers, 768 / 3072, 12 heads, vocabulary 30522; seeded synthetic
weights, batch 1), one caption of T tokens in three phrases under the block mask of ``text_masks_from_input_ids``:

  the library's BertModel in fp32 (what ``GroundingDinoDetector.from_pretrained(text_backbone="torch")`` runs), the same module in fp16,
  omg_amd.BertTextEncoder(linear="gemm") and (linear="skinny") eager, and the last replayed from a ``torch.cuda.graph``;

and the four Linear shapes of a layer alone (q | k | v 2304 x 768, attention output 768 x 768, intermediate 3072 x 768 with its GELU,
output 768 x 3072; bias and residual as the layer uses them), omg_gemm_skinny against omg_gemm (+ omg_gelu_erf where the layer needs it),
each replayed from a graph of ``--reps`` back-to-back launches so that the figure is the kernel and not the launch, with weight bytes /
time in TB/s.  THE WEIGHTS ARE CACHE-RESIDENT in these figures: the launches of a replay run on the same 1.2 - 4.7 MB weight, so from the
second on it comes from L2 / the Infinity Cache, for both kernels alike — the comparison is fair, the rate is not an HBM stream rate.

    python tools/bert_bench.py [--tokens 4 8 16 32 64 128 256] [--log profiles/bert_bench.log] [--timeout 600]

Per T: 2 warm-up calls of each path, then two interleaved rounds of ``--calls`` synchronised calls each; per round the median is
reported.  The last line names the largest T of the list up to which omg_gemm_skinny is no slower than omg_gemm on the sum of a layer's
four Linears in both rounds: ``omg_amd.bert.T_SKINNY`` is set from it.  No ratio is a criterion: the log says what was measured, and
says so plainly where the HIP path loses.  The tool ends itself after ``--timeout`` seconds.
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

from omg_amd import bert as hip_bert
from omg_amd import ops
from omg_amd.gdino_decoder import text_masks_from_input_ids

CFG = dict(hidden_size=768, num_attention_heads=12, intermediate_size=3072, num_hidden_layers=12, vocab_size=30522,
           max_position_embeddings=512, type_vocab_size=2, layer_norm_eps=1e-12, hidden_act="gelu", position_embedding_type="absolute")
# (name, N, K, gelu, residual) of a layer's four Linears
LINEARS = [("qkv", 2304, 768, False, False), ("attn.out", 768, 768, False, True), ("intermediate", 3072, 768, True, False),
           ("output", 768, 3072, False, True)]


def seed_state(model, seed):
    g = torch.Generator(device=model._device).manual_seed(seed)
    sd = {}
    for key, t in model.state_dict().items():
        z = torch.randn(t.shape, generator=g, device=t.device, dtype=torch.float32)
        if "embeddings.weight" in key:
            v = z
        elif "LayerNorm.weight" in key:
            v = 1.0 + 0.2 * z
        elif key.endswith("bias"):
            v = 0.1 * z
        else:
            v = z * (2.0 if (".query." in key or ".key." in key) else 1.0) / math.sqrt(t.shape[1])
        sd[key] = v
    return sd


def caption(T, dev):
    """[CLS] w .. w . w .. w ? w .. w . [SEP]: three phrases (fewer where T has no room)."""
    g = torch.Generator().manual_seed(T)
    ids = (2000 + torch.randint(0, 20000, (T,), generator=g)).tolist()
    ids[0], ids[-1] = 101, 102
    for frac, tok in ((1 / 3, 1012), (2 / 3, 1029), (1.0, 1012)):
        p = min(T - 2, max(1, int(round(frac * (T - 2)))))
        if 0 < p < T - 1:
            ids[p] = tok
    return torch.tensor([ids], device=dev)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def rounds(fns, calls, n_rounds=2):
    out = []
    for _ in range(n_rounds):
        ts = [[] for _ in fns]
        for _ in range(calls):
            for t, f in zip(ts, fns):
                t.append(timed(f))
        out.append([statistics.median(t) for t in ts])
    return out


def graph_of(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    g.replay()
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", nargs="+", type=int, default=[4, 8, 16, 32, 64, 128, 256])
    ap.add_argument("--log", default=None)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=600)
    a = ap.parse_args()
    signal.alarm(a.timeout)
    dev = torch.device("cuda:0")
    lines = [f"BERT-base text encoder (12 layers, 768 / 3072, vocabulary 30522), batch 1, {torch.cuda.get_device_name(0)}; medians of {a.calls} "
             f"synchronised calls, two interleaved rounds; single Linears: {a.reps} launches a graph replay on the SAME weight, which is "
             f"therefore cache-resident (L2 / Infinity Cache) from the second launch on, for both kernels: TB/s = weight bytes / time, not an HBM rate"]

    def emit(s):
        lines.append(s)
        print(s, flush=True)
        if a.log:
            with open(a.log, "w") as f:
                f.write("\n".join(lines) + "\n")

    print(lines[0], flush=True)
    from transformers import BertConfig, BertModel
    hip = {k: hip_bert.BertTextEncoder(CFG, dtype=torch.float16, device=dev, linear=k) for k in ("gemm", "skinny")}
    sd = seed_state(hip["gemm"], 30)
    for m in hip.values():
        m.load_state_dict(sd, strict=True)
    lib32 = BertModel(BertConfig(**CFG), add_pooling_layer=False).eval()
    lib32.load_state_dict({k: v.float().cpu() for k, v in sd.items()}, strict=False)
    lib32 = lib32.to(dev)
    lib16 = BertModel(BertConfig(**CFG), add_pooling_layer=False).eval()
    lib16.load_state_dict({k: v.float().cpu() for k, v in sd.items()}, strict=False)
    lib16 = lib16.to(device=dev, dtype=torch.float16)
    g = torch.Generator(device=dev).manual_seed(1)
    W = {n: (torch.randn(N, K, generator=g, device=dev) / math.sqrt(K)).half() for n, N, K, _, _ in LINEARS}
    Bv = {n: torch.randn(N, generator=g, device=dev).half() for n, N, K, _, _ in LINEARS}
    best = 0
    still = True
    for T in a.tokens:
        ids = caption(T, dev)
        mask, pos = text_masks_from_input_ids(ids)
        types = torch.zeros_like(ids)
        with torch.no_grad():
            f32 = lambda: lib32(input_ids=ids, attention_mask=mask[:, None], token_type_ids=types, position_ids=pos)[0]     # noqa: E731
            f16 = lambda: lib16(input_ids=ids, attention_mask=mask[:, None], token_type_ids=types, position_ids=pos)[0]     # noqa: E731
            hg = lambda: hip["gemm"](ids, mask, types, pos)                                                                     # noqa: E731
            hs = lambda: hip["skinny"](ids, mask, types, pos)                                                                   # noqa: E731
            fns = [f32, f16, hg, hs]
            for _ in range(2):
                for f in fns:
                    f()
            ref = f32().float()
            err = [float((f().float() - ref).norm() / ref.norm()) for f in (f16, hg, hs)]
            r = rounds(fns, a.calls)
            graph = graph_of(hs)
            tg = statistics.median([timed(graph.replay) for _ in range(2 * a.calls)])
        emit(f"T = {T}: " + "; ".join(f"round {i + 1}: library fp32 {x[0]:.3f} ms, library fp16 {x[1]:.3f} ms, HIP gemm {x[2]:.3f} ms, HIP skinny {x[3]:.3f} ms"
                                      for i, x in enumerate(r)) + f"; HIP skinny replayed from a graph {tg:.3f} ms; rms difference from the library's "
             f"fp32 output / its rms: library fp16 {err[0]:.1e}, HIP gemm {err[1]:.1e}, HIP skinny {err[2]:.1e}")
        slower = [n for n, k in (("library fp32", 0), ("library fp16", 1)) if any(min(x[2], x[3]) > x[k] for x in r)]
        if slower:
            emit(f"    at T = {T} the eager HIP module is SLOWER than " + " and ".join(slower) + " in at least one round")
        # ---- the four Linears alone
        x768, x3072 = torch.randn(T, 768, generator=g, device=dev).half(), torch.randn(T, 3072, generator=g, device=dev).half()
        res = torch.randn(T, 768, generator=g, device=dev).half()
        tot = [[0.0, 0.0], [0.0, 0.0]]
        for n, N, K, gelu, use_res in LINEARS:
            x = x3072 if K == 3072 else x768
            rr = res if use_res else None
            out = torch.empty(T, N, device=dev, dtype=torch.float16)

            def sk():
                for _ in range(a.reps):
                    ops.gemm_skinny(x, W[n], bias=Bv[n], gelu=gelu, residual=rr, out=out)

            def gm():
                for _ in range(a.reps):
                    ops.gemm(x, W[n], bias=Bv[n], residual=rr, out=out)
                    if gelu:
                        ops.gelu_erf(out, out=out)

            gs, gg = graph_of(sk), graph_of(gm)
            rl = rounds([gs.replay, gg.replay], a.calls)
            for i, (ts, tg_) in enumerate(rl):
                tot[i][0] += ts / a.reps
                tot[i][1] += tg_ / a.reps
            emit(f"    Linear {n} [{T} x {K}] x [{N} x {K}]^T: " + "; ".join(
                f"round {i + 1}: skinny {ts / a.reps * 1e3:.2f} us ({N * K * 2 / (ts / a.reps * 1e-3) / 1e12:.2f} TB/s, weights cache-resident), "
                f"omg_gemm {tg_ / a.reps * 1e3:.2f} us ({N * K * 2 / (tg_ / a.reps * 1e-3) / 1e12:.2f} TB/s)" for i, (ts, tg_) in enumerate(rl)))
        ok = all(t[0] <= t[1] for t in tot)
        emit(f"    a layer's four Linears at T = {T}: " + "; ".join(f"round {i + 1}: skinny {t[0] * 1e3:.2f} us, omg_gemm {t[1] * 1e3:.2f} us"
                                                                      for i, t in enumerate(tot))
             + ("; skinny is not slower in both rounds" if ok else "; skinny is SLOWER in at least one round"))
        still = still and ok
        if still:
            best = T
    emit(f"t_skinny: the largest T of {a.tokens} up to which (and at every smaller T of the list) omg_gemm_skinny is no slower than omg_gemm on "
         f"the sum of a layer's four Linears in both rounds: {best}")


if __name__ == "__main__":
    main()
