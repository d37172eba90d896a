"""The general prompt-to-prompt cross edit folded into V (CPU, -m "not gpu"): with the controller's fp32 tables
    V'[w, :] = sum_n M[w, n] alpha[n] V[n, :],   V''[n, :] = (1 - alpha[n]) V[n, :]
``P_base V' + P_own V''`` must equal the oracle's edited probabilities times V — the algebra omg_transpose_v_mapped and the two
omg_attn_fwd launches of a "mixed" cross layer implement — in float64, at every step, for a word swap with per-word windows, for two
edits and for equal prompts with a cross-replace window.  Also: the host-side classification of every step, and the C ABI."""
import os
import re
import subprocess

import pytest
import torch

from omg_amd import controller as pc
from oracle import controller as oc

HEADS, NQ, NK, D = 2, 8, 77, 64
STEPS = 8
SWAP = ["a man on the road", "a woman on the road"]
WINDOWS = {"default_": 0.6, "road": (0.2, 0.9)}
CASES = {
    "word_swap": (SWAP, WINDOWS),
    "two_edits": (["a man on the road", "a woman on the road", "a dog on the road"], WINDOWS),
    "equal_half": (["a man on the road", "a man on the road"], 0.5),
}


def make(name):
    prompts, crs = CASES[name]
    crs_a = dict(crs) if isinstance(crs, dict) else crs
    crs_b = dict(crs) if isinstance(crs, dict) else crs
    ctl = pc.AttentionReplace(prompts, STEPS, crs_a, (0.0, 0.5), 4, 4, tokenizer=oc.PieceTokenizer(), dtype=torch.float16)
    ora = oc.AttentionReplaceOracle(prompts, STEPS, crs_b, (0.0, 0.5), 4, 4, tokenizer=oc.PieceTokenizer())
    return prompts, ctl, ora


@pytest.mark.parametrize("name", list(CASES))
def test_folded_edit_equals_the_oracles_edited_probabilities(name):
    prompts, ctl, ora = make(name)
    n = len(prompts)
    mapper, alpha, _ = ctl.edit_tables("cpu")
    assert mapper.dtype == torch.float32 and alpha.dtype == torch.float32
    assert tuple(mapper.shape) == (n - 1, NK, NK) and tuple(alpha.shape) == (STEPS + 1, n - 1, NK)
    # the protocol attributes keep the reference's dtype and shape
    assert ctl.mapper.dtype == torch.float16 and tuple(ctl.mapper.shape) == (n - 1, NK, NK)
    assert tuple(ctl.cross_replace_alpha.shape) == (STEPS + 1, n - 1, 1, 1, NK)
    g = torch.Generator().manual_seed(3)
    q = torch.randn(n, HEADS, NQ, D, generator=g, dtype=torch.float64)
    k = torch.randn(n, HEADS, NK, D, generator=g, dtype=torch.float64)
    v = torch.randn(n, HEADS, NK, D, generator=g, dtype=torch.float64)
    probs = torch.softmax(q @ k.transpose(-1, -2) * D ** -0.5, dim=-1)              # (prompts, heads, q, k): the conditional half
    M, A = mapper.double(), alpha.double()
    for step in range(STEPS + 1):
        ora.cur_step = step
        want = ora._edit(probs.reshape(n * HEADS, NQ, NK).clone(), True).reshape(n, HEADS, NQ, NK) @ v
        got = torch.empty_like(want)
        got[0] = probs[0] @ v[0]
        for e in range(n - 1):
            v1 = torch.einsum("wn,n,hnd->hwd", M[e], A[step, e], v[e + 1])
            v2 = (1 - A[step, e])[None, :, None] * v[e + 1]
            got[e + 1] = probs[0] @ v1 + probs[e + 1] @ v2
        assert (got - want).abs().max().item() < 1e-12, (name, step)


def test_kind_of_every_step():
    _, eq, _ = make("equal_half")
    lo = int(0.5 * (STEPS + 1))
    assert [eq.cross_kind(s) for s in range(STEPS + 1)] == ["borrow"] * lo + ["own"] * (STEPS + 1 - lo)
    assert not eq.is_pure_replacement
    _, sw, _ = make("word_swap")
    hi = int(0.9 * (STEPS + 1))                                                    # "road" keeps alpha = 1 until here
    assert [sw.cross_kind(s) for s in range(STEPS + 1)] == ["mixed"] * hi + ["own"] * (STEPS + 1 - hi)
    pure = pc.AttentionReplace(["a man", "a man"], STEPS, {"default_": 1.0}, 0.4, 4, 4)
    assert pure.is_pure_replacement and all(pure.cross_kind(s) == "borrow" for s in range(STEPS + 1))


def test_fused_edit_ticks_like_call_and_returns_the_row_plan():
    _, ctl, _ = make("two_edits")
    ctl.num_att_layers = 4
    ctl.cur_step = STEPS                                                           # last table row: every alpha is 0
    kind, src, edit_of = ctl.fused_edit(True, 16, 6, device="cpu")
    assert (kind, src, edit_of) == ("own", None, None) and ctl.cur_att_layer == 1
    ctl.reset()
    ctl._bound_step = (torch.zeros(1, dtype=torch.int32), 0)                       # a bound counter: nothing is written on the host side
    kind, src, edit_of = ctl.fused_edit(True, 16, 6, device="cpu", total_batch=14, images=2)
    assert kind == "mixed"
    assert src.tolist() == [0, 1, 2, 3, 3, 3, 6, 7, 8, 9, 9, 9, 12, 13]
    assert edit_of.tolist() == [-1, -1, -1, -1, 0, 1, -1, -1, -1, -1, 0, 1, -1, -1]
    kind, src, edit_of = ctl.fused_edit(False, 16, 6, device="cpu")               # self-attention inside the window: borrow Q, K
    assert kind == "borrow" and src.tolist() == [0, 1, 2, 3, 3, 3] and edit_of is None
    kind, src, _ = ctl.fused_edit(False, 17, 6, device="cpu")                     # a map larger than width * height is left alone
    assert kind == "own" and src is None
    ctl.fused_edit(True, 16, 6, device="cpu")
    assert (ctl.cur_step, ctl.cur_att_layer) == (1, 0)
    with pytest.raises(ValueError):
        ctl.fused_edit(True, 16, 4, device="cpu")
    # the entry points of the pure path keep their errors
    with pytest.raises(RuntimeError):
        ctl.fused_qk_src(True, 16, 6)
    with pytest.raises(RuntimeError):
        ctl.skip_layer()
    blend = pc.AttentionReplace(SWAP, STEPS, 0.6, 0.5, 4, 4, local_blend=object(), tokenizer=oc.PieceTokenizer())
    with pytest.raises(RuntimeError):
        blend.fused_edit(True, 16, 4, device="cpu")


def test_bound_counter_offsets_the_alpha_table():
    _, ctl, _ = make("word_swap")
    step = torch.zeros(1, dtype=torch.int32)
    ctl.bind_step_counter(step, 3)
    mapper, alpha, s = ctl.edit_tables("cpu")
    assert s is step and tuple(alpha.shape) == (STEPS + 1 - 3, 1, NK)
    assert torch.equal(alpha[0], ctl.edit_tables("cpu")[1][0]) and torch.equal(alpha[0], ctl._alpha_host[3])
    ctl.bind_step_counter(None)
    assert tuple(ctl.edit_tables("cpu")[1].shape) == (STEPS + 1, 1, NK)


def test_abi_has_the_mapped_transpose_and_is_still_6():
    from omg_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "omg_hip.h")).read(), flags=re.S)
    assert re.search(r"\bomg_transpose_v_mapped\s*\(", header)
    assert "omg_transpose_v_mapped" in _lib.SYMBOLS
    lib = _lib.lib()
    assert hasattr(lib, "omg_transpose_v_mapped")
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r"\bT omg_transpose_v_mapped\b", nm)
    assert lib.omg_abi_version() == 6
    # the ctypes mirror has the size the C compiler gives the struct
    import ctypes
    code = '#include <stdio.h>\n#include "omg_hip.h"\nint main(){printf("%zu\\n",sizeof(omg_vmap_args));return 0;}'
    exe = os.path.join(root, "tests", "_vmap_size.out")
    subprocess.run(["gcc", "-x", "c", "-I", os.path.join(root, "include"), "-o", exe, "-"], input=code.encode(), check=True)
    try:
        assert int(subprocess.check_output([exe], text=True)) == ctypes.sizeof(_lib.VMapArgs)
    finally:
        os.remove(exe)
