"""Generate tests/golden/bert.npz: what transformers' BertModel(add_pooling_layer=False) computes in fp32 on the CPU for two small configs
under the inputs GroundingDINO gives its text backbone (the [B, 1, T, T] phrase block mask and the per-phrase position ids of the
library's generate_masks_with_special_tokens_and_transfer_map).

    python tests/golden/make_golden_bert.py        (from the repository root; CPU only, about ten seconds)

The weights are NOT stored: tests/bert_torch.py's ``seed_state`` regenerates them from the recorded seed and the per-key checksums pin
that.  Two configs (``bert_torch.small_cfg``), under the prefixes ``a.`` and ``b.``:

    a   hidden 768, 12 heads, intermediate 3072, 2 layers, vocabulary 1100: the real Linear shapes of BERT-base
    b   hidden 192, 3 heads, intermediate 328 (a multiple of 8, not of 32), 3 layers, 300 positions

Config a's position table has 128 rows, not 64: its T = 70 input, the one beyond the module's first ``t_skinny`` at the real
widths, would be refused by the module on a 64-row table (T > max_position_embeddings), although no per-phrase position id comes near 64.

Per config and per padded length T (6, 23, 70; b also 256) one batch of three captions of different lengths, several phrases each
(closed by 1012 / 1029), right padded with [PAD]; T = 70 and 256 are beyond 64, the module's first ``t_skinny``.  Stored:
  cfg_seed, sd_keys, sum.<key>          the seed, the state-dict keys and a float64 checksum per key
  T<T>.input_ids / .token_type_ids / .attention_mask (uint8 [B, T, T]) / .position_ids / .lengths
  T<T>.idx.token, T<T>.idx.channel      the sampled positions
  T<T>.state<i>                         the library's state i (0: the embeddings' output, i: after layer i - 1) [B, tokens, channels]
  T<T>.oracle_err                       rms(oracle - library) / rms(library) per state over ALL positions: fp32 rounding
  T<T>.twin_err                         [2, states]: the same figure of bert_torch's fp16 and bf16 twins against the fp32 oracle
  T<T>.defect.<name>                    what each deliberate defect of bert_torch.DEFECTS does to the last state (rms / rms)

CONDITIONS, asserted before the file is written.  The oracle reproduces the library to fp32 rounding on every state (< 2e-5; the figures
found are 2e-7 .. 6e-7).  The masks and position ids equal the library's.  On every input each defect moves the last state by at least
10 x the fp16 twin's figure on that state — a condition on the fixture (seeds and weight scales), not a tolerance of any test.  No defect
of the list had to be taken off it."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import bert_torch as bt  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "bert.npz")
CONFIGS = {"a": dict(seed=71), "b": dict(seed=72)}
SENSITIVITY = 10.0


def pick(n, k):
    return np.unique(np.round(np.linspace(0, n - 1, min(n, k))).astype(np.int64))


def checksum(v: torch.Tensor) -> np.ndarray:
    return np.array(float((v.double() * torch.arange(1, v.numel() + 1, dtype=torch.float64).reshape(v.shape).remainder(7.0).add(1.0)).sum()))


def library_run(cfg, sd, inp):
    from transformers import BertConfig, BertModel
    from transformers.models.grounding_dino.modeling_grounding_dino import generate_masks_with_special_tokens_and_transfer_map
    m = BertModel(BertConfig(**bt.hf_config_dict(cfg)), add_pooling_layer=False).eval()
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all(k == "embeddings.position_ids" for k in missing), (missing, unexpected)
    mask, pos = generate_masks_with_special_tokens_and_transfer_map(inp["input_ids"])
    assert torch.equal(mask, inp["attention_mask"]) and torch.equal(pos, inp["position_ids"]), "bert_torch.text_masks differs from the library"
    with torch.no_grad():
        o = m(input_ids=inp["input_ids"], attention_mask=mask[:, None], token_type_ids=inp["token_type_ids"], position_ids=pos,
              output_hidden_states=True, return_dict=True)
    assert torch.equal(o.hidden_states[-1], o.last_hidden_state)
    return list(o.hidden_states)


def oracle(cfg, sd, inp, **kw):
    with torch.no_grad():
        return bt.forward(sd, cfg, inp["input_ids"], inp["attention_mask"], inp["token_type_ids"], inp["position_ids"], **kw)


def build():
    out = {}
    for name, c in CONFIGS.items():
        cfg = bt.small_cfg(name)
        sd = bt.seed_state(cfg, c["seed"])
        out[name + ".cfg_seed"] = np.array(c["seed"])
        out[name + ".sd_keys"] = np.array(list(sd))
        for k, v in sd.items():
            out[f"{name}.sum.{k}"] = checksum(v)
        for T in cfg["lengths"]:
            P = f"{name}.T{T}."
            inp = bt.seeded_ids(cfg, T, 1000 * c["seed"] + T)
            assert len(set(inp["lengths"])) == 3, inp["lengths"]
            assert int(inp["position_ids"].max()) < cfg["positions"] and T <= cfg["positions"]
            for k in ("input_ids", "token_type_ids", "position_ids"):
                out[P + k] = inp[k].numpy()
            out[P + "attention_mask"] = inp["attention_mask"].to(torch.uint8).numpy()
            out[P + "lengths"] = np.array(inp["lengths"])
            lib = library_run(cfg, sd, inp)
            assert len(lib) == cfg["layers"] + 1
            it, ic = pick(T, 8), pick(cfg["hidden"], 64)
            out[P + "idx.token"], out[P + "idx.channel"] = it, ic
            for i, s in enumerate(lib):
                out[P + f"state{i}"] = s[:, torch.from_numpy(it)][:, :, torch.from_numpy(ic)].numpy()
            ref = oracle(cfg, sd, inp)
            err = [bt.rel_rms(r, l) for r, l in zip(ref, lib)]
            print(f"{name} T={T} lengths {inp['lengths']}: oracle against the library, per state: " + " ".join(f"{e:.2e}" for e in err))
            assert max(err) < 2e-5, err
            out[P + "oracle_err"] = np.array(err)
            tw = []
            for dt in (torch.float16, torch.bfloat16):
                o = oracle(cfg, {k: v.to(dt).float() for k, v in sd.items()}, inp, twin=dt)
                tw.append([bt.rel_rms(a, b) for a, b in zip(o, ref)])
            out[P + "twin_err"] = np.array(tw)
            print(f"{name} T={T} twins on the last state: fp16 {tw[0][-1]:.3e}, bf16 {tw[1][-1]:.3e}")
            for d in bt.DEFECTS:
                dv = bt.rel_rms(oracle(cfg, sd, inp, defect=d)[-1], ref[-1])
                out[P + f"defect.{d}"] = np.array(dv)
                print(f"{name} T={T} {d:22s} {dv:.4f} ({dv / tw[0][-1]:.0f} x twin)")
                assert dv >= SENSITIVITY * tw[0][-1], f"config {name}, T = {T}: the fixture does not see defect '{d}'"
    return out


def main():
    torch.manual_seed(0)
    out = build()
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
