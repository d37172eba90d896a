"""omg_amd.BertTextEncoder on the HIP kernels (-m gpu) against tests/golden/bert.npz (the library's BertModel in fp32 on the CPU, under
GroundingDINO's phrase block mask and per-phrase position ids) and against tests/bert_torch.py, the plain-torch oracle that
tests/test_bert.py pins to the fixture.

The error figure is rms(error) / rms(fp32 oracle output).  The bound is 2 x the same figure of bert_torch's 16-bit twin on the same
input (FACTOR of tests/test_gdino_gpu.py and tests/test_swin_gpu.py, for the same reason: the twin rounds after every operation, the
kernels round once per fused pass and sum in another order; a factor of two covers the order, it does not cover a wrong layer — the
fixture's generator asserts that each of seven deliberate defects moves the last state by at least 10 x the fp16 twin's figure).  Every
recorded state (the embeddings' output and the state after every layer) is held to the rule against ITS twin figure; the fixture's
positions to 1.5 x that.

Measured on an MI355X (HIP figure / twin figure, the worst over all recorded states and the inputs T = 6, 23, 70 (b: and 256)):

    config  batch   fp16: skinny / gemm   bf16: skinny / gemm
    a       1       0.89 / 0.91           0.91 / 0.92
    a       3       0.89 / 0.90           0.91 / 0.92
    b       1       0.94 / 1.04           0.96 / 1.01
    b       3       0.89 / 0.94           0.92 / 0.95

("auto" is the skinny column: with T_SKINNY = 256, the largest T a call can have, it takes omg_gemm_skinny at every T; omg_gemm is reached
through linear="gemm" or an explicit t_skinny.  The twin's own figures on the last state: 1.2e-3 .. 1.5e-3 in fp16, 0.9e-2 .. 1.2e-2 in
bf16.)  The same table is in DESIGN.md section 5.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from omg_amd import bert as hip_bert
from tests import bert_torch as bt

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bert.npz")
DTYPES = [torch.float16, torch.bfloat16]
CONFIGS = ["a", "b"]
LINEARS = ["auto", "skinny", "gemm"]
FACTOR = 2.0
KEYS = ("input_ids", "attention_mask", "token_type_ids", "position_ids")


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLD)
    return {k: z[k] for k in z.files}


_CACHE = {}


def inputs_of(gold, name, T):
    P = f"{name}.T{T}."
    return dict(input_ids=torch.from_numpy(gold[P + "input_ids"]), token_type_ids=torch.from_numpy(gold[P + "token_type_ids"]),
                attention_mask=torch.from_numpy(gold[P + "attention_mask"]).bool(), position_ids=torch.from_numpy(gold[P + "position_ids"]))


def weights(gold, name):
    if name not in _CACHE:
        _CACHE[name] = bt.seed_state(bt.small_cfg(name), int(gold[name + ".cfg_seed"]))
    return _CACHE[name]


def oracle(gold, name, T):
    """(cfg, sd, the three captions of padded length T, {dtype: [twin figure per state]}, [fp32 oracle states]) — once per (config, T);
    the first B samples of a batch are the first B rows of every state, so B = 1 shares it."""
    if (name, T) not in _CACHE:
        cfg, sd, inp = bt.small_cfg(name), weights(gold, name), inputs_of(gold, name, T)
        with torch.no_grad():
            ref = bt.forward(sd, cfg, **inp)
            twins = {}
            for d in DTYPES:
                tw = bt.forward({k: v.to(d).float() for k, v in sd.items()}, cfg, twin=d, **inp)
                twins[d] = tw
        _CACHE[(name, T)] = (cfg, sd, inp, twins, ref)
    return _CACHE[(name, T)]


_MODELS = {}


def hip_model(gold, name, dtype, dev, linear="auto"):
    key = (name, dtype, linear)
    if key not in _MODELS:
        m = hip_bert.BertTextEncoder(bt.hf_config_dict(bt.small_cfg(name)), dtype=dtype, device=dev, linear=linear)
        m.load_state_dict(weights(gold, name), strict=True)
        _MODELS[key] = m
    return _MODELS[key]


def run_hip(m, inp, dev, sl=slice(None)):
    return m(*[inp[k][sl].to(dev) for k in KEYS])


def states_of(m, inp, dev, sl):
    last, states = m(*[inp[k][sl].to(dev) for k in KEYS], output_hidden_states=True)
    assert torch.equal(last, states[-1]) and len(states) == m.cfg["layers"] + 1
    return states


@pytest.mark.parametrize("linear", LINEARS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name", CONFIGS)
def test_against_fixture_and_oracle(dev, gold, name, B, dtype, linear):
    m = hip_model(gold, name, dtype, dev, linear)
    worst = 0.0
    for T in bt.small_cfg(name)["lengths"]:
        cfg, sd, inp, twins, ref = oracle(gold, name, T)
        assert m.uses_skinny(T) == (linear == "skinny" or linear == "auto" and T <= hip_bert.T_SKINNY)
        got_all = states_of(m, inp, dev, slice(0, B))
        P = f"{name}.T{T}."
        it, ic = torch.from_numpy(gold[P + "idx.token"]), torch.from_numpy(gold[P + "idx.channel"])
        for i, got in enumerate(got_all):
            got = got.float().cpu()
            assert got.shape == ref[i][:B].shape and torch.isfinite(got).all(), (T, i)
            twin = bt.rel_rms(twins[dtype][i][:B], ref[i][:B])
            e = bt.rel_rms(got, ref[i][:B])
            e_lib = bt.rel_rms(got[:, it][:, :, ic], torch.from_numpy(gold[P + f"state{i}"])[:B])
            worst = max(worst, e / twin)
            print(f"{name} B={B} {str(dtype)[6:]} {linear} T={T} state{i}: rms error / rms {e:.3e} (fixture positions {e_lib:.3e}), twin {twin:.3e}, "
                  f"ratio {e / twin:.2f}")
            assert e <= FACTOR * twin, (T, i, e, twin)
            assert e_lib <= FACTOR * 1.5 * twin, (T, i, e_lib, twin)
    print(f"{name} B={B} {str(dtype)[6:]} {linear}: worst ratio {worst:.2f}")


@pytest.mark.parametrize("linear", LINEARS)
@pytest.mark.parametrize("name", CONFIGS)
def test_batched_equals_single(dev, gold, name, linear):
    """A batched call is bitwise the single calls, per caption over its own tokens (and over its padding): M = 3 T against M = T on one
    kernel, since the kernel is chosen by T."""
    m = hip_model(gold, name, torch.float16, dev, linear)
    for T in bt.small_cfg(name)["lengths"]:
        _, _, inp, _, _ = oracle(gold, name, T)
        both = run_hip(m, inp, dev)
        for b, n in enumerate(int(x) for x in gold[f"{name}.T{T}.lengths"]):
            one = run_hip(m, inp, dev, slice(b, b + 1))
            assert torch.equal(both[b, :n], one[0, :n]), (T, b)
            assert torch.equal(both[b:b + 1], one), (T, b)


@pytest.mark.parametrize("t_skinny", [64, None])
def test_a_caption_is_the_same_alone_and_beside_a_longer_one(dev, gold, t_skinny):
    """Under "auto" the T = 23 caption padded to 70 is bitwise the same alone and beside the T = 70 caption: the kernel is chosen by T = 70
    for both calls, never by B T (70 and 140 rows).  With ``t_skinny=64``, the value the module started with, both calls take omg_gemm;
    with the measured default (T_SKINNY = 256) both take omg_gemm_skinny.  The T = 23 caption at its own length (omg_gemm_skinny either
    way) is NOT asked to equal itself padded to 70 across the two kernels: that is what "a function of T" allows.  It is asked to be the
    same alone and beside a second caption of T = 23 (23 and 46 rows)."""
    kw = {} if t_skinny is None else dict(t_skinny=t_skinny)
    m = hip_bert.BertTextEncoder(bt.hf_config_dict(bt.small_cfg("a")), dtype=torch.float16, device=dev, linear="auto", **kw)
    m.load_state_dict(weights(gold, "a"), strict=True)
    _, _, i23, _, _ = oracle(gold, "a", 23)
    _, _, i70, _, _ = oracle(gold, "a", 70)
    pad = lambda t: torch.nn.functional.pad(t, (0, 70 - 23))
    ids = torch.cat([pad(i23["input_ids"][:1]), i70["input_ids"][:1]])
    types = torch.cat([pad(i23["token_type_ids"][:1]), i70["token_type_ids"][:1]])
    from omg_amd.gdino_decoder import text_masks_from_input_ids
    mask, pos = text_masks_from_input_ids(ids)
    assert m.uses_skinny(23) and m.uses_skinny(70) == (t_skinny is None) and hip_bert.T_SKINNY >= 70
    both = m(ids.to(dev), mask.to(dev), types.to(dev), pos.to(dev))
    alone = m(ids[:1].to(dev), mask[:1].to(dev), types[:1].to(dev), pos[:1].to(dev))
    assert torch.equal(both[:1], alone)
    two = run_hip(m, i23, dev, slice(0, 2))
    one = run_hip(m, i23, dev, slice(0, 1))
    assert torch.equal(two[:1], one)
    # the caption's own tokens against the oracle, padded: padding tokens are seen by nobody under the block mask
    _, _, _, twins, ref = oracle(gold, "a", 23)
    assert bt.rel_rms(alone[0, :23].float().cpu(), ref[-1][0]) <= FACTOR * bt.rel_rms(twins[torch.float16][-1][0], ref[-1][0])


@pytest.mark.parametrize("linear,T", [("skinny", 23), ("gemm", 70), ("auto", 6)])
def test_graph_replay_equals_eager(dev, gold, linear, T):
    m = hip_model(gold, "a", torch.float16, dev, linear)
    _, _, inp, _, _ = oracle(gold, "a", T)
    d_inp = [inp[k].to(dev) for k in KEYS]
    eager = m(*d_inp)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m(*d_inp)                                    # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = m(*d_inp)
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(cap, eager)
