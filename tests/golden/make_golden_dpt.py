"""Generate tests/golden/dpt_golden.npz: what ``transformers.DPTForDepthEstimation`` computes in fp32 on two small DPT-hybrid configs.

    python tests/golden/make_golden_dpt.py        (from the repository root; CPU only, a few seconds)

The weights are NOT stored: tests/dpt_torch.py's ``seed_state`` regenerates them from the recorded seed (numpy's MT19937 stream on the
fp16 grid), and the per-key checksums pin that.  Two configs (``dpt_torch.small_cfg``), under the prefixes ``s96.`` and ``s192.``:

    s96    96 x 96 input,  6 x 6 + 1 =  37 tokens: the resident-K/V attention path, V^T operand
    s192  192 x 192 input, 12 x 12 + 1 = 145 tokens: the self-attention kernel, row-major V, a key count that is no multiple of 64

Stored per config:
  cfg_seed, cfg_input_seed, cfg_image_size   the seeds and the size (the architecture is dpt_torch.small_cfg(size))
  sd_keys, sum.<key>                         the state-dict keys and a float64 checksum per key
  input_q                                    the input [2, 3, S, S] as int8: pixel value = input_q / 8 (normal, rounded to that grid)
  idx.<name>, <name>                         an intermediate at the rows / columns (or tokens) idx.<name>, as the library has it:
                                             bit_stage1, bit_stage2 (NCHW), vit_tap0, vit_tap1 ([B, N, C]), fused0 .. fused3 (NCHW)
  idx.depth, depth                           predicted_depth [2, S, S] at the 48 rows / columns idx.depth
  zero_share, std_over_mean                  of predicted_depth: the generator asserts zero_share < 5 % (the library's default
                                             initialisation leaves the final ReLU dead; a degenerate output cannot pass)
  twin_err                                   rms error / rms of dpt_torch's fp16 and bf16 twins against the fp32 output, for scale"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import dpt_torch as dt  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "dpt_golden.npz")
CONFIGS = {"s96": dict(size=96, seed=21, input_seed=5), "s192": dict(size=192, seed=22, input_seed=6)}
NAMES = ("bit_stage1", "bit_stage2", "vit_tap0", "vit_tap1", "fused0", "fused1", "fused2", "fused3")


def make_input(seed, size):
    """[2, 3, size, size] normal pixel values on the grid of eighths (int8 / 8: exact in fp16 and bf16)."""
    rs = np.random.RandomState(seed)
    return np.clip(np.round(rs.standard_normal((2, 3, size, size)) * 8.0), -127, 127).astype(np.int8)


def pick(n, k):
    return np.unique(np.round(np.linspace(0, n - 1, min(n, k))).astype(np.int64))


def sub(t, k=7):
    """(indices, values): a [B, C, H, W] map at pick(H) x pick(W); a [B, N, C] sequence at pick(N, 24) tokens."""
    if t.dim() == 4:
        i = pick(t.shape[2], k)
        ti = torch.from_numpy(i)
        return i, t[:, :, ti][:, :, :, ti].numpy()
    i = pick(t.shape[1], 24)
    return i, t[:, torch.from_numpy(i)].numpy()


def library_run(cfg, sd, x):
    """predicted_depth and the named intermediates of the library's class on the state dict ``sd``."""
    from transformers import DPTForDepthEstimation
    hf = DPTForDepthEstimation(dt.to_hf_config(cfg)).eval()
    hf.load_state_dict(sd, strict=True)
    got = {}
    hooks = []
    stages = hf.dpt.embeddings.backbone.bit.encoder.stages
    hooks.append(stages[0].register_forward_hook(lambda m, i, o: got.__setitem__("bit_stage1", o)))
    hooks.append(stages[1].register_forward_hook(lambda m, i, o: got.__setitem__("bit_stage2", o)))
    taps = cfg["backbone_out_indices"][2:]
    for n, li in enumerate(taps):
        hooks.append(hf.dpt.encoder.layer[li].register_forward_hook(lambda m, i, o, n=n: got.__setitem__(f"vit_tap{n}", o[0] if isinstance(o, tuple) else o)))
    for n, ly in enumerate(hf.neck.fusion_stage.layers):
        hooks.append(ly.register_forward_hook(lambda m, i, o, n=n: got.__setitem__(f"fused{n}", o)))
    with torch.no_grad():
        depth = hf(x).predicted_depth
    for h in hooks:
        h.remove()
    return depth, got


def main():
    torch.manual_seed(0)
    out = {}
    for name, c in CONFIGS.items():
        P = name + "."
        cfg = dt.small_cfg(c["size"])
        m = dt.seed_state(dt.DPTHybrid(cfg).eval(), c["seed"])
        sd = m.state_dict()
        out[P + "cfg_seed"], out[P + "cfg_input_seed"], out[P + "cfg_image_size"] = np.array(c["seed"]), np.array(c["input_seed"]), np.array(c["size"])
        out[P + "sd_keys"] = np.array(list(sd))
        for k, v in sd.items():
            out[P + "sum." + k] = dt.checksum(v)
        xq = make_input(c["input_seed"], c["size"])
        out[P + "input_q"] = xq
        x = torch.from_numpy(xq.astype(np.float32) / 8.0)
        depth, got = library_run(cfg, sd, x)
        assert depth.shape == (2, c["size"], c["size"]) and sorted(got) == sorted(NAMES), (depth.shape, sorted(got))
        for k in NAMES:
            out[P + "idx." + k], out[P + k] = sub(got[k])
        i = pick(c["size"], 48)
        out[P + "idx.depth"], out[P + "depth"] = i, depth[:, torch.from_numpy(i)][:, :, torch.from_numpy(i)].numpy()
        zero, som = float((depth == 0).float().mean()), float(depth.std() / depth.mean())
        out[P + "zero_share"], out[P + "std_over_mean"] = np.array(zero), np.array(som)
        with torch.no_grad():
            ref = m(x)
            tw = [dt.rel_rms(m(x, twin=d), ref) for d in (torch.float16, torch.bfloat16)]
        out[P + "twin_err"] = np.array(tw)
        print(f"{name}: depth mean {float(depth.mean()):.3f}, exact zeros {zero:.4f}, std / mean {som:.3f}; dpt_torch vs library max |d| / rms "
              f"{float((ref - depth).abs().max() / depth.pow(2).mean().sqrt()):.2e}; twin rms error fp16 {tw[0]:.2e}, bf16 {tw[1]:.2e}")
        assert zero < 0.05, f"{name}: {zero:.3f} of the depth values are exactly zero — a degenerate fixture"
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print(f"wrote {OUT}: {size} bytes, {len(out)} arrays")
    assert size < (1 << 20), size


if __name__ == "__main__":
    main()
