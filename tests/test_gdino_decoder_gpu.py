"""omg_amd.GroundingDinoDecoderHead on the HIP kernels (-m gpu) against tests/golden/gdino_decoder_golden.npz (the library's own modules in
fp32 on the CPU) and against tests/gdino_decoder_torch.py, the plain-torch oracle that tests/test_gdino_decoder.py pins to that fixture.

The error figure is rms(error) / rms(fp32 oracle output).  The bound is 2 x the same figure of the oracle's 16-bit twin on the same
input (tests/test_gdino_gpu.py's factor, for the same reason: the twin rounds after every operation, the kernels round once per fused
pass and sum in another order; a factor of two covers the order, it does not cover a wrong layer — the fixture's generator asserts that
every deliberate defect that applies moves pred_boxes, the last state or the logits by at least 10 x the fp16 twin's figure).  Every
layer's state and reference, the finite logits and pred_boxes of every level are held to the rule against THEIR twin figure; the -inf
pattern of the logits is exact.

With the module's own selection the selected SET must be the library's (the generator asserts that the gap at the cut is 20 x the
twin's error on the scores: fp16 on configs a and b, bf16 on config c, which is b with 6 queries).  The order inside the set is the
module's own and the outputs are held to the oracle on that order (see the test's docstring: the learned query embedding is indexed by
the query slot, so a permutation of the proposals is not a permutation of the outputs).

Measured on an MI355X (HIP figure / twin figure, the worst of states, references, pred_boxes, finite logits and initial references):

    config  batch   fp16                                           bf16
    a       1       1.23 (references; states 1.08, logits 1.10)    1.05
    a       2       1.20                                           1.03
    b       1       1.00                                           1.02
    b       2       1.00                                           1.00
    own selection, batch 2:  a 1.12, b 1.00, c 1.14 (fp16); c 1.00 (bf16);  a's weights on b's sizes: 1.02

(the twin's own figures: states 2e-3 .. 4e-3 in fp16 and 2e-2 .. 3e-2 in bf16, boxes 2e-4 .. 6e-4 and 2e-3 .. 5e-3).  The same table is
in DESIGN.md section 5.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from omg_amd import gdino_decoder as hip
from tests import gdino_decoder_torch as gd

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gdino_decoder_golden.npz")
DTYPES = [torch.float16, torch.bfloat16]
CONFIGS = ["a", "b"]
FACTOR = 2.0
KEYS = ("states", "references", "pred_boxes", "logits", "init_reference_points")


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLD)
    return {k: z[k] for k in z.files}


_CACHE = {}


def take(inp, B):
    return {k: (v if k == "spatial" else v[:B]) for k, v in inp.items()}


def run_oracle(cfg, sd, inp, **kw):
    with torch.no_grad():
        o = gd.forward(sd, cfg, inp["memory"], inp["text"], inp["mask_flatten"], inp["text_token_mask"], inp["spatial"], inp["valid_ratios"], **kw)
    return dict(states=torch.stack(o["states"], 1), references=torch.stack(o["references"], 1), pred_boxes=torch.stack(o["pred_boxes"], 1),
                logits=torch.stack(o["logits"], 1), init_reference_points=o["init_reference_points"], topk=o["topk_proposals"], scores=o["scores"])


def figure(got, ref):
    keep = torch.isfinite(ref)
    return gd.rel_rms(got[keep], ref[keep])


def oracle(gold, name, B):
    """(cfg, sd, inputs of the first B samples, the library's top-k, {dtype: {what: twin figure}}, {what: fp32 oracle}) — once per case."""
    key = (name, B)
    if key not in _CACHE:
        cfg = gd.small_cfg(name)
        sd = gd.seed_state(cfg, int(gold[name + ".seed"]))
        inp = take(gd.seeded_inputs(cfg, int(gold[name + ".input_seed"])), B)
        topk = torch.from_numpy(gold[name + ".topk"])[:B]
        ref = run_oracle(cfg, sd, inp, topk_proposals=topk)
        twins = {}
        for d in DTYPES:
            tw = run_oracle(cfg, {k: v.to(d).float() for k, v in sd.items()}, inp, topk_proposals=topk, twin=d)
            twins[d] = {k: figure(tw[k], ref[k]) for k in KEYS}
        _CACHE[key] = (cfg, sd, inp, topk, twins, ref)
    return _CACHE[key]


def hip_model(cfg, sd, dtype, dev):
    h = hip.GroundingDinoDecoderHead(cfg, dtype=dtype, device=dev)
    h.load_state_dict(sd, strict=True)
    return h


def enc_of(inp, dev, dtype):
    return type("Enc", (), dict(last_hidden_state_vision=inp["memory"].to(dev).to(dtype), last_hidden_state_text=inp["text"].to(dev).to(dtype),
                                spatial_shapes_list=list(inp["spatial"]), valid_ratios=inp["valid_ratios"].to(dev),
                                mask_flatten=inp["mask_flatten"].to(dev)))()


def run_hip(h, inp, dev, **kw):
    o = h(enc_of(inp, dev, h.dtype), inp["text_token_mask"].to(dev), output_hidden_states=True, **kw)
    return o, dict(states=o.intermediate_hidden_states.float().cpu(), references=o.intermediate_reference_points.cpu(),
                   pred_boxes=torch.stack(o.all_pred_boxes, 1).cpu(), logits=torch.stack(o.all_logits, 1).cpu(),
                   init_reference_points=o.init_reference_points.cpu(), topk=o.topk_proposals.cpu())


def held(tag, got, ref, twins):
    worst = 0.0
    for k in KEYS:
        assert got[k].shape == ref[k].shape, (k, got[k].shape, ref[k].shape)
        if k == "logits":
            assert got[k].dtype == torch.float32 and torch.equal(torch.isneginf(got[k]), torch.isneginf(ref[k])), "exact -inf pattern"
            assert not torch.isnan(got[k]).any() and not torch.isposinf(got[k]).any()
        else:
            assert torch.isfinite(got[k]).all(), k
        e = figure(got[k], ref[k])
        ratio = e / twins[k] if twins[k] > 0 else 0.0
        worst = max(worst, ratio)
        print(f"{tag} {k}: rms error / rms {e:.3e}, twin {twins[k]:.3e}, ratio {ratio:.2f}")
        assert e <= FACTOR * twins[k], (k, e, twins[k])
    print(f"{tag}: worst ratio {worst:.2f}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("name", CONFIGS)
def test_against_fixture_and_oracle(dev, gold, name, B, dtype):
    cfg, sd, inp, topk, twins, ref = oracle(gold, name, B)
    h = hip_model(cfg, sd, dtype, dev)
    o, got = run_hip(h, inp, dev, topk_proposals=topk.to(dev))
    held(f"{name} B={B} {str(dtype)[6:]}", got, ref, twins[dtype])
    # the fixture itself (the library), at its sampled queries, to 1.5 x the rule
    qs = torch.from_numpy(gold[name + ".q_s"])
    for k, g in (("states", got["states"][:, :, qs]), ("references", got["references"][:, :, qs]), ("pred_boxes", got["pred_boxes"]), ("logits", got["logits"])):
        lib = torch.from_numpy(gold[f"{name}.{k}"]).transpose(0, 1)[:B]
        e = figure(g, lib)
        assert e <= FACTOR * 1.5 * twins[dtype][k], (k, e)
    assert torch.equal(o.logits, o.all_logits[-1]) and torch.equal(o.pred_boxes, o.all_pred_boxes[-1])
    assert o.logits.shape == (B, cfg["num_queries"], 256) and o.pred_boxes.shape == (B, cfg["num_queries"], 4)
    assert float(o.pred_boxes.min()) >= 0.0 and float(o.pred_boxes.max()) <= 1.0
    # only the last level is computed unless all are asked for, and it is the same
    last = h(enc_of(inp, dev, dtype), inp["text_token_mask"].to(dev), topk_proposals=topk.to(dev))
    assert last.all_logits is None and torch.equal(last.logits, o.logits) and torch.equal(last.pred_boxes, o.pred_boxes)


@pytest.mark.parametrize("case", [("a", torch.float16), ("b", torch.float16), ("c", torch.float16), ("c", torch.bfloat16)],
                         ids=["a-fp16", "b-fp16", "c-fp16", "c-bf16"])
def test_own_selection_picks_the_librarys_set(dev, gold, case):
    """The selected set is the library's.  The ORDER inside the set is the module's own (descending by its own 16-bit-operand scores, ties
    — config a's 59 padded rows share one score — in torch.topk's order on the device), and it matters: query slot i pairs the learned
    query_position_embeddings row i with the i-th selected proposal, so the decoder is NOT equivariant under a permutation of the
    proposals.  The outputs are therefore held to the oracle run on the module's own order, with the twin of that run."""
    name, dtype = case
    cfg, sd, inp, topk, _, _ = oracle(gold, name, 2)
    h = hip_model(cfg, sd, dtype, dev)
    _, got = run_hip(h, inp, dev)
    assert torch.equal(got["topk"].sort(1)[0], topk.sort(1)[0]), "the selected set is the library's"
    ref = run_oracle(cfg, sd, inp, topk_proposals=got["topk"])
    tw = run_oracle(cfg, {k: v.to(dtype).float() for k, v in sd.items()}, inp, topk_proposals=got["topk"], twin=dtype)
    held(f"{name} own selection {str(dtype)[6:]}", got, ref, {k: figure(tw[k], ref[k]) for k in KEYS})
    if name == "a":          # sample 1 selects invalid proposals: box logit +inf, an initial reference of exactly 1
        assert bool((got["init_reference_points"][1] == 1.0).all(-1).any())


@pytest.mark.parametrize("name", CONFIGS)
def test_batched_equals_single(dev, gold, name):
    cfg, sd, inp, topk, _, _ = oracle(gold, name, 2)
    h = hip_model(cfg, sd, torch.float16, dev)
    _, both = run_hip(h, inp, dev)
    one_inp = {k: (v if k == "spatial" else v[1:]) for k, v in inp.items()}
    _, one = run_hip(h, one_inp, dev)
    for k in KEYS + ("topk",):
        assert torch.equal(both[k][1:], one[k]), k


def test_graph_replay_equals_the_eager_call(dev, gold):
    cfg, sd, inp, _, _, _ = oracle(gold, "a", 2)
    h = hip_model(cfg, sd, torch.float16, dev)
    enc, tm = enc_of(inp, dev, torch.float16), inp["text_token_mask"].to(dev)
    eager = h(enc, tm)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        h(enc, tm)                               # warm-up off the default stream: workspaces, packed weights
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = h(enc, tm)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(cap.logits, eager.logits) and torch.equal(cap.pred_boxes, eager.pred_boxes) and torch.equal(cap.topk_proposals, eager.topk_proposals)
    # new inputs in the captured buffers, replayed
    enc.last_hidden_state_vision.copy_(enc.last_hidden_state_vision.flip(0))
    enc.last_hidden_state_text.copy_(enc.last_hidden_state_text.flip(0))
    tm.copy_(tm.flip(0))
    enc.mask_flatten.copy_(enc.mask_flatten.flip(0))
    enc.valid_ratios.copy_(enc.valid_ratios.flip(0))
    g.replay()
    torch.cuda.synchronize()
    again = h(enc, tm)
    assert torch.equal(cap.logits, again.logits) and torch.equal(cap.pred_boxes, again.pred_boxes)
    assert torch.equal(again.pred_boxes, eager.pred_boxes.flip(0))


def test_a_second_input_size_through_the_same_module(dev, gold):
    """Config a's weights on config b's levels and text length (and back): nothing of the first call's shapes is kept."""
    cfg, sd, inp_a, topk_a, twins_a, ref_a = oracle(gold, "a", 2)
    h = hip_model(cfg, sd, torch.float16, dev)
    _, first = run_hip(h, inp_a, dev, topk_proposals=topk_a.to(dev))
    inp_b = gd.seeded_inputs(gd.small_cfg("b"), 7)
    ref_b = run_oracle(cfg, sd, inp_b)
    tw = run_oracle(cfg, {k: v.half().float() for k, v in sd.items()}, inp_b, topk_proposals=ref_b["topk"], twin=torch.float16)
    _, got = run_hip(h, inp_b, dev, topk_proposals=ref_b["topk"].to(dev))
    held("a's weights on b's sizes fp16", got, ref_b, {k: figure(tw[k], ref_b[k]) for k in KEYS})
    _, back = run_hip(h, inp_a, dev, topk_proposals=topk_a.to(dev))
    for k in KEYS:
        assert torch.equal(back[k], first[k]), k


def test_detect_on_the_modules_output(dev, gold):
    cfg, sd, inp, topk, _, ref = oracle(gold, "b", 2)
    h = hip_model(cfg, sd, torch.float16, dev)
    o, _ = run_hip(h, inp, dev, topk_proposals=topk.to(dev))
    res = hip.detect(o, box_threshold=0.3, text_threshold=0.25)
    assert len(res) == 2
    for b, (boxes, scores, masks) in enumerate(res):
        want = ref["logits"][b, -1].sigmoid().max(-1)[0] > 0.3
        near = (ref["logits"][b, -1].sigmoid().max(-1)[0] - 0.3).abs() < 0.02          # decided by rounding: either way
        keep = (o.logits[b].sigmoid().max(-1)[0] > 0.3).cpu()
        assert bool(((keep == want) | near).all())
        assert boxes.shape == (int(keep.sum()), 4) and scores.shape == (int(keep.sum()),) and masks.shape == (int(keep.sum()), 256)
        assert bool((scores > 0.3).all())
