"""The CLIP text encoders on the causal flash kernel (-m gpu): one `omg_transpose_v` + one `omg_attn_fwd_causal` per layer whatever
the number of prompts and heads, parity with oracle/text_encoder.py at the existing tolerance, and the bitwise properties a causal
kernel with lane-local rows gives the whole encoder: a prompt's result does not depend on its batch, a position's not on later tokens."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from omg_amd import _lib as L
from omg_amd.text_encoder import ClipTextConfig, ClipTextEncoder
from oracle import text_encoder as ot
from tests.test_text_encoder_gpu import _pair

EOS_AT = [2, 4, 40, 70, 76]


def _ids5(seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(2, 298, (5, 77), generator=g)      # five different rows
    ids[:, 0] = 298
    for b, n in enumerate(EOS_AT):
        ids[b, n:] = 299
    return ids


class _CountingLib:
    """Stands in for the ctypes library object: every `omg_*` call is counted by name, then forwarded."""

    def __init__(self, lib):
        self._lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("omg_") or name == "omg_last_error":
            return fn

        def counted(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a)
        return counted


def _count(monkeypatch, enc, ids):
    enc(ids)                                   # packs the weights outside the count
    proxy = _CountingLib(L.lib())
    monkeypatch.setattr(L, "_lib", proxy)
    try:
        enc(ids)
    finally:
        monkeypatch.undo()
    return proxy.calls


def _encoder(heads, dev):
    """head_dim is fixed at 64, so the width follows the head count: 128 for 2 heads, 256 for 4."""
    cfg = ClipTextConfig(vocab_size=300, hidden_size=64 * heads, intermediate_size=256, num_hidden_layers=3, num_attention_heads=heads,
                         projection_dim=64, eos_token_id=299, with_projection=False)
    enc = ClipTextEncoder(cfg, dtype=torch.float16, device=dev)
    g = torch.Generator().manual_seed(heads)
    enc.load_state_dict({k: (0.05 * torch.randn(v.shape, generator=g)).to(torch.float16).to(dev) for k, v in enc.state_dict().items()})
    return enc


def test_the_number_of_library_calls_does_not_depend_on_prompts_or_heads(dev, monkeypatch):
    ids = _ids5(0).to(dev)
    enc2, enc4 = _encoder(2, dev), _encoder(4, dev)
    one, five = _count(monkeypatch, enc2, ids[:1]), _count(monkeypatch, enc2, ids)
    four_heads = _count(monkeypatch, enc4, ids)
    print(five)
    assert one == five == four_heads
    assert five["omg_attn_fwd_causal"] == 3 and five["omg_transpose_v"] == 3        # one of each per layer
    assert "omg_softmax_rows" not in five and "omg_add_inplace" not in five


@pytest.fixture(scope="module")
def encoded(dev):
    """(oracle config, fp32 state dict, encoder, ids, hidden, pooled) per (activation, dtype), computed once."""
    res = {}
    for act, proj in (("quick_gelu", False), ("gelu", True)):
        for dtype in (torch.float16, torch.bfloat16):
            ocfg, sd, enc = _pair(act, proj, dev, dtype, seed=10)
            ids = _ids5(11)
            h, p = enc(ids.to(dev))
            res[act, dtype] = (ocfg, sd, enc, ids, h, p)
    return res


@pytest.mark.parametrize("act", ["quick_gelu", "gelu"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_five_prompts_match_the_oracle(encoded, dtype, act):
    ocfg, sd, enc, ids, h, p = encoded[act, dtype]
    hidden, last, pooled = ot.text_model(sd, ocfg, ids)
    tol = 2e-2 if dtype == torch.float16 else 1e-1
    ref_h = hidden[-2]
    eh = ((h.float().cpu() - ref_h).abs().max() / ref_h.pow(2).mean().sqrt()).item()
    ep = ((p.float().cpu() - pooled).abs().max() / pooled.pow(2).mean().sqrt()).item()
    print(f"hidden {eh:.3e} pooled {ep:.3e} (bound {tol})")
    assert h.shape == ref_h.shape and p.shape == pooled.shape
    assert eh < tol and ep < tol


@pytest.mark.parametrize("act", ["quick_gelu", "gelu"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_a_prompt_encodes_to_the_same_bits_alone_and_in_a_batch(dev, encoded, dtype, act):
    _, _, enc, ids, h, p = encoded[act, dtype]
    for b in range(5):
        h1, p1 = enc(ids[b:b + 1].to(dev))
        assert torch.equal(h1[0], h[b]) and torch.equal(p1[0], p[b]), b


@pytest.mark.parametrize("act", ["quick_gelu", "gelu"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("pos", [1, 40, 76])
def test_a_later_token_does_not_reach_earlier_positions(dev, encoded, dtype, act, pos):
    _, _, enc, ids, h, _ = encoded[act, dtype]
    ids2 = ids.clone()
    ids2[:, pos] = torch.where(ids[:, pos] == 7, 8, 7)
    h2, _ = enc(ids2.to(dev))
    assert torch.equal(h2[:, :pos], h[:, :pos])
    assert not torch.equal(h2[:, pos:], h[:, pos:])
