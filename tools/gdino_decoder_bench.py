#!/usr/bin/env python
"""A/B of GroundingDINO's query selection, decoder and heads at full width: omg_amd.GroundingDinoDecoderHead (six layers, 900 queries,
d_model 256, 8 heads, FFN 2048, four levels; seeded synthetic weights, fp16, batch 1) against a per-layer torch evaluation of the SAME
weights on the same device in fp16, composed as the library composes it — the [B, N, T] contrastive logits written and reduced, the box
MLP on all N rows and a gather, six value_proj passes over the image memory, F.scaled_dot_product_attention for the two attentions, the
grid_sample composition of the deformable attention at box references, the reference bookkeeping as elementwise torch ops.  The
proposals are computed by the same torch code on both sides.

    python tools/gdino_decoder_bench.py [--sizes 800x800 800x1200] [--texts 16 256] [--log profiles/gdino_decoder_bench.log] [--timeout 600]

Per (image size, text length): 2 warm-up calls of each path, then two interleaved rounds (torch, HIP, torch, HIP, ...) of ``--calls``
synchronised calls each; per round the median is reported; then the HIP call replayed from a ``torch.cuda.graph``.  No ratio is a
criterion: the log says what was measured, and says so plainly where the HIP path loses.  The tool ends itself after ``--timeout``
seconds.
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

from omg_amd import gdino_decoder as gdd

CFG = dict(d_model=256, decoder_attention_heads=8, decoder_ffn_dim=2048, decoder_n_points=4, num_feature_levels=4, decoder_layers=6,
           num_queries=900, activation_function="relu", layer_norm_eps=1e-5, max_text_len=256, query_dim=4, two_stage=True,
           embedding_init_target=True, decoder_bbox_embed_share=True)


def seed_model(model, seed):
    g = torch.Generator(device=model._device).manual_seed(seed)
    sd = {}
    for key, t in model.state_dict().items():
        z = torch.randn(t.shape, generator=g, device=t.device, dtype=torch.float32)
        if t.dim() == 1 and key.endswith("weight"):
            v = 1.0 + 0.2 * z
        elif key.endswith("bias"):
            v = (1.5 if "sampling_offsets" in key else 0.1) * z
        elif key == "query_position_embeddings.weight":
            v = z
        else:
            v = z * (2.0 if "sampling_offsets" in key else 1.0) / math.sqrt(t[0].numel())
        sd[key] = v
    model.load_state_dict(sd, strict=True)


def sine_embed(pos):
    dim_t = torch.arange(128, dtype=torch.float32, device=pos.device)
    dim_t = 10000 ** (2 * torch.div(dim_t, 2, rounding_mode="floor") / 128)
    es = [c[..., None] * (2 * math.pi) / dim_t for c in pos.unbind(-1)]
    es = [torch.stack((e[..., 0::2].sin(), e[..., 1::2].cos()), dim=-1).flatten(-2) for e in es]
    es[0], es[1] = es[1], es[0]
    return torch.cat(es, dim=-1)


class TorchDecoder:
    """The selection, the decoder and the last level's heads of ``model`` evaluated op by op by torch, in the storage dtype."""

    def __init__(self, model):
        self.m, self.w = model, model._w

    def lin(self, x, n):
        return F.linear(x, self.w[n + ".weight"], self.w[n + ".bias"])

    def ln(self, x, n):
        return F.layer_norm(x, (256,), self.w[n + ".weight"], self.w[n + ".bias"], self.m.cfg["eps"])

    def box(self, x, n):
        return self.lin(F.relu(self.lin(F.relu(self.lin(x, n + ".layers.0")), n + ".layers.1")), n + ".layers.2")

    def mha(self, p, q, k, v, keep):
        B, Nq, d = q.shape
        sh = lambda x: x.reshape(B, -1, 8, 32).transpose(1, 2)
        mask = None if keep is None else keep[:, None, None, :]
        o = F.scaled_dot_product_attention(sh(self.lin(q, p + "query")), sh(self.lin(k, p + "key")), sh(self.lin(v, p + "value")), attn_mask=mask)
        return self.lin(o.transpose(1, 2).reshape(B, Nq, d), p + "out_proj")

    def msdeform(self, p, hq, mem, keep, ref_input, spatial):
        B, Q, d = hq.shape
        N, Lv = mem.shape[1], len(spatial)
        value = self.lin(mem, p + "value_proj").masked_fill(~keep[..., None], 0.0).view(B, N, 8, 32)
        off = self.lin(hq, p + "sampling_offsets").view(B, Q, 8, Lv, 4, 2)
        aw = F.softmax(self.lin(hq, p + "attention_weights").view(B, Q, 8, Lv * 4), -1)
        r = ref_input.to(hq.dtype)
        loc = r[:, :, None, :, None, :2] + off / 4 * r[:, :, None, :, None, 2:] * 0.5
        grids = 2 * loc - 1
        vals = value.split([h * w for h, w in spatial], dim=1)
        sampled = []
        for l, (h, w) in enumerate(spatial):
            vl = vals[l].flatten(2).transpose(1, 2).reshape(B * 8, 32, h, w)
            gl = grids[:, :, :, l].transpose(1, 2).flatten(0, 1)
            sampled.append(F.grid_sample(vl, gl, mode="bilinear", padding_mode="zeros", align_corners=False))
        aw = aw.transpose(1, 2).reshape(B * 8, 1, Q, Lv * 4)
        out = (torch.stack(sampled, dim=-2).flatten(-2) * aw).sum(-1).view(B, d, Q).transpose(1, 2).contiguous()
        return self.lin(out, p + "output_proj")

    @torch.no_grad()
    def __call__(self, mem, txt, keep, token_keep, spatial, vr):
        c, w = self.m.cfg, self.w
        B, N, d = mem.shape
        Q = c["num_queries"]
        prop, ok = gdd.proposals(keep, spatial)
        oq = self.ln(self.lin(mem.masked_fill(~ok[..., None], 0.0), "enc_output"), "enc_output_norm")
        cls = (oq @ txt.transpose(-1, -2)).masked_fill(~token_keep[:, None, :], float("-inf"))
        coord = self.box(oq, "encoder_output_bbox_embed").float() + prop
        topk = torch.topk(cls.max(-1)[0], Q, dim=1)[1]
        ref = torch.gather(coord, 1, topk[..., None].expand(-1, -1, 4)).sigmoid()
        init = ref
        h = w["query_position_embeddings.weight"][None].repeat(B, 1, 1)
        refs = []
        for i in range(c["layers"]):
            p = f"decoder.layers.{i}."
            ref_input = ref[:, :, None] * torch.cat([vr, vr], -1)[:, None]
            pos = self.lin(F.relu(self.lin(sine_embed(ref_input[:, :, 0]).to(h.dtype), "decoder.reference_points_head.layers.0")),
                           "decoder.reference_points_head.layers.1")
            h = self.ln(h + self.mha(p + "self_attn.", h + pos, h + pos, h, None), p + "self_attn_layer_norm")
            h = self.ln(h + self.mha(p + "encoder_attn_text.", h + pos, txt, txt, token_keep), p + "encoder_attn_text_layer_norm")
            h = self.ln(h + self.msdeform(p + "encoder_attn.", h + pos, mem, keep, ref_input, spatial), p + "encoder_attn_layer_norm")
            h = self.ln(h + self.lin(F.relu(self.lin(h, p + "fc1")), p + "fc2"), p + "final_layer_norm")
            refs.append(ref)
            ref = (self.box(h, f"decoder.bbox_embed.{i}").float() + torch.special.logit(ref, eps=1e-5)).sigmoid()
        hn = self.ln(h, "decoder.layer_norm")
        boxes = (self.box(hn, f"decoder.bbox_embed.{c['layers'] - 1}").float() + torch.special.logit(refs[-1] if c["layers"] > 1 else init, eps=1e-5)).sigmoid()
        logits = torch.full((B, Q, c["max_text_len"]), float("-inf"), device=mem.device)
        logits[..., :txt.shape[1]] = (hn @ txt.transpose(-1, -2)).float().masked_fill(~token_keep[:, None, :], float("-inf"))
        return logits, boxes, topk


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
    ap.add_argument("--texts", nargs="+", type=int, default=[16, 256])
    ap.add_argument("--log", default=None)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=600)
    a = ap.parse_args()
    signal.alarm(a.timeout)
    dev = torch.device("cuda:0")
    lines = [f"GroundingDINO query selection + 6 decoder layers + heads, 900 queries, fp16, batch 1, {torch.cuda.get_device_name(0)}; "
             f"medians of {a.calls} synchronised calls, two interleaved rounds"]

    def emit(s):
        lines.append(s)
        print(s, flush=True)
        if a.log:
            with open(a.log, "w") as f:
                f.write("\n".join(lines) + "\n")

    print(lines[0], flush=True)
    model = gdd.GroundingDinoDecoderHead(CFG, dtype=torch.float16, device=dev)
    seed_model(model, 40)
    tv = TorchDecoder(model)
    for size in a.sizes:
        H, W = (int(v) for v in size.split("x"))
        spatial = [(-(-H // s), -(-W // s)) for s in (8, 16, 32)]
        spatial.append(((spatial[-1][0] - 1) // 2 + 1, (spatial[-1][1] - 1) // 2 + 1))
        N = sum(h * w for h, w in spatial)
        g = torch.Generator(device=dev).manual_seed(H + W)
        mem = torch.randn(1, N, 256, generator=g, device=dev).half()
        keep = torch.ones(1, N, dtype=torch.bool, device=dev)
        vr = torch.ones(1, 4, 2, device=dev)
        for T in a.texts:
            txt = torch.randn(1, T, 256, generator=g, device=dev).half()
            tk = torch.ones(1, T, dtype=torch.bool, device=dev)
            enc = type("Enc", (), dict(last_hidden_state_vision=mem, last_hidden_state_text=txt, spatial_shapes_list=spatial, valid_ratios=vr,
                                       mask_flatten=keep))()
            old = lambda: tv(mem, txt, keep, tk, spatial, vr)                                                                        # noqa: E731
            new = lambda: model(enc, tk)                                                                                             # noqa: E731
            for _ in range(2):
                old(); new()
            o, n = old(), new()
            same = len(set(o[2][0].tolist()) & set(n.topk_proposals[0].tolist()))
            emit(f"decoder {H} x {W} (N = {N}), T = {T}: " + fmt(rounds(old, new, a.calls)) + f"; {same} of 900 selected proposals in common")
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                new()
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                new()
            graph.replay()
            emit(f"    the HIP call replayed from a graph: {statistics.median([timed(graph.replay) for _ in range(2 * a.calls)]):.3f} ms")


if __name__ == "__main__":
    main()
