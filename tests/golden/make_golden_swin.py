"""Generate tests/golden/swin_golden.npz: what ``transformers.SwinBackbone`` computes in fp32 on the CPU for two small configs.

    python tests/golden/make_golden_swin.py        (from the repository root; CPU only, a few seconds)

The weights are NOT stored: tests/swin_torch.py's ``seed_state`` regenerates them from the recorded seed (numpy's MT19937 stream on the
fp16 grid), and the per-key checksums pin that.  Two configs (``swin_torch.small_cfg``), under the prefixes ``w7.`` and ``w12.``:

    w7    90 x 118 input, window 7, embed 32, heads 1 / 2 / 4, depths 2 / 2 / 2: the patch embedding pads to 92 x 120 -> grid 23 x 30
          (windows pad it to 28 x 35); merging pads 23 -> 24 -> 12 x 15 (-> 14 x 21); -> 6 x 8, smaller than the window (-> 7 x 14)
    w12   104 x 152 input, window 12, embed 96, heads 3 / 6 (no power of two), depths 2 / 2: grid 26 x 38 (-> 36 x 48); 13 x 19 (-> 24 x 24)

Stored per config:
  cfg_seed, cfg_input_seed                   the seeds (the architecture and the input size are swin_torch.small_cfg(name))
  sd_keys, sum.<key>                         the state-dict keys and a float64 checksum per key
  input_q                                    the input [2, 3, H, W] as int8: pixel value = input_q / 8
  idx.<name>, <name>                         embeddings, stage1 .. stageN ([B, h w, C], before downsampling) at the tokens idx.<name>;
                                             map1 .. mapN (the normed NCHW feature maps) at the rows idx.<name>.y and columns idx.<name>.x
  twin_err                                   rms error / rms of swin_torch's fp16 and bf16 twins on the last feature map, for scale
  defect.<name>                              what each deliberate defect of swin_torch does to the last feature map (rms / rms)

SENSITIVITY.  Before the file is written the oracle is run, on the file's own inputs, with each defect of ``swin_torch.DEFECTS`` (the
shift mask dropped, the padded keys excluded, the roll reversed, the bias index's sign flipped, the merge order permuted), and each
must move the last feature map by at least 10 x the fp16 twin's figure.  That is a condition on the fixture (seed and weight scale),
not a tolerance of any test: a fixture that fails it is changed until the reference alone satisfies it."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import swin_torch as st  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "swin_golden.npz")
CONFIGS = {"w7": dict(seed=41, input_seed=9), "w12": dict(seed=42, input_seed=10)}
SENSITIVITY = 10.0


def pick(n, k):
    return np.unique(np.round(np.linspace(0, n - 1, min(n, k))).astype(np.int64))


def library_run(cfg, sd, x):
    from transformers import SwinBackbone
    hf = SwinBackbone(st.to_hf_config(cfg)).eval()
    assert list(hf.state_dict()) == list(sd)
    hf.load_state_dict(sd, strict=True)
    with torch.no_grad():
        o = hf(x, output_hidden_states=True)
    seqs = [h.flatten(2).transpose(1, 2) for h in o.hidden_states]            # stem, stage1 ..: NCHW -> [B, h w, C]
    return seqs, o.feature_maps


def main():
    torch.manual_seed(0)
    out = {}
    for name, c in CONFIGS.items():
        P = name + "."
        cfg = st.small_cfg(name)
        sd = st.seed_state(cfg, c["seed"])
        out[P + "cfg_seed"], out[P + "cfg_input_seed"] = np.array(c["seed"]), np.array(c["input_seed"])
        out[P + "sd_keys"] = np.array(list(sd))
        for k, v in sd.items():
            out[P + "sum." + k] = st.checksum(v)
        H, W = cfg["image"]
        xq = st.seeded_input(c["input_seed"], 2, H, W)
        out[P + "input_q"] = xq
        x = torch.from_numpy(xq.astype(np.float32) / 8.0)
        seqs, maps = library_run(cfg, sd, x)
        names = ["embeddings"] + [f"stage{i + 1}" for i in range(len(cfg["depths"]))]
        assert len(seqs) == len(names) and len(maps) == len(cfg["out_features"])
        for k, t in zip(names, seqs):
            i = pick(t.shape[1], 24)
            out[P + "idx." + k], out[P + k] = i, t[:, torch.from_numpy(i)].numpy()
        for n, t in enumerate(maps):
            iy, ix = pick(t.shape[2], 7), pick(t.shape[3], 7)
            out[P + f"idx.map{n + 1}.y"], out[P + f"idx.map{n + 1}.x"] = iy, ix
            out[P + f"map{n + 1}"] = t[:, :, torch.from_numpy(iy)][:, :, :, torch.from_numpy(ix)].numpy()
        with torch.no_grad():
            ref = st.forward(sd, cfg, x)
            last = ref["feature_maps"][-1]
            lib_d = max(float((a - b).abs().max() / b.pow(2).mean().sqrt()) for a, b in zip(ref["feature_maps"], maps))
            tw = [st.rel_rms(st.forward(sd, cfg, x, twin=d)["feature_maps"][-1], last) for d in (torch.float16, torch.bfloat16)]
            out[P + "twin_err"] = np.array(tw)
            print(f"{name}: grids {ref['grids']}; swin_torch vs library max |d| / rms {lib_d:.2e}; twin rms error fp16 {tw[0]:.2e}, bf16 {tw[1]:.2e}")
            assert lib_d < 1e-3, lib_d
            for d in st.DEFECTS:
                e = st.rel_rms(st.forward(sd, cfg, x, defect=d)["feature_maps"][-1], last)
                out[P + "defect." + d] = np.array(e)
                print(f"  defect {d}: moves the last feature map by {e:.3e} = {e / tw[0]:.0f} x the fp16 twin")
                assert e >= SENSITIVITY * tw[0], f"{name}: the fixture cannot tell '{d}' from rounding ({e:.3e} against {tw[0]:.3e}); change the seed or the scale"
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print(f"wrote {OUT}: {size} bytes, {len(out)} arrays")
    assert size < (1 << 19), size


if __name__ == "__main__":
    main()
