"""Two CPU float64 references of softmax(q k^T * scale) v for the attention tests (tests/test_attention_conditioning_gpu.py,
tests/test_attn_model.py).  Both take the STORED 16-bit q (..., Nq, 64), k (..., Nkv, 64), v (..., Nkv, 64) — any leading
(sample, head) dimensions — and the softmax scale.

* :func:`truth`: the operation in float64.  The reference of record.
* :func:`model`: the same with the rounding points the kernels document (csrc/attn.hip, v2's comment) and nothing else of
  their structure — no tiles, no lazy reference maximum, no MFMA layouts or summation orders:
      Q' = round16(float32(q) * float32(scale * log2 e))      the pre-scaled query, stored in 16 bits
      S  = Q' k^T                                             exact (float64), in log2 units
      P  = round16(exp2(S - rowmax S))                        the probabilities the second MFMA consumes
      O  = (P v) / sum(P)                                     float64; the caller rounds it to the storage type
  It says how much error the DESIGN has on a given input; a kernel's error is another draw from the same distribution.
"""
import math

import torch

LOG2E_F32 = torch.tensor(1.4426950408889634, dtype=torch.float32)


def round16(x: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """float64 -> nearest value of the 16-bit storage type, returned as float64."""
    return x.to(dtype).double()


def ulp(dtype: torch.dtype) -> float:
    """Spacing of the storage type relative to a value at the bottom of its binade (2^-10 fp16, 2^-7 bf16)."""
    return 2.0 ** -10 if dtype == torch.float16 else 2.0 ** -7


def scaled_query(q: torch.Tensor, scale: float) -> torch.Tensor:
    """Q' exactly as the kernels form it: fp32 product with the fp32 constant scale * log2 e, rounded to q's type."""
    sl2e = torch.tensor(scale, dtype=torch.float32) * LOG2E_F32
    return (q.float() * sl2e).to(q.dtype)


def truth_probs(q, k, scale):
    s = (q.double() @ k.double().transpose(-1, -2)) * scale
    return torch.softmax(s, dim=-1)


def truth(q, k, v, scale):
    return truth_probs(q, k, scale) @ v.double()


def model_logits(q, k, scale):
    """The log2-unit scores of the model: Q' k^T in float64."""
    return scaled_query(q, scale).double() @ k.double().transpose(-1, -2)


def model(q, k, v, scale):
    """Unrounded O of the rounding model (float64): round it with :func:`round16`, after any out_scale / accumulate."""
    s = model_logits(q, k, scale)
    p = round16(torch.exp2(s - s.amax(dim=-1, keepdim=True)), q.dtype)
    return (p @ v.double()) / p.sum(dim=-1, keepdim=True)


def split_heads(t: torch.Tensor, heads: int) -> torch.Tensor:
    """(B, N, heads*64) -> (B, heads, N, 64)"""
    return t.reshape(t.shape[0], t.shape[1], heads, 64).permute(0, 2, 1, 3)


def merge_heads(t: torch.Tensor) -> torch.Tensor:
    """(B, heads, N, 64) -> (B, N, heads*64)"""
    return t.permute(0, 2, 1, 3).reshape(t.shape[0], t.shape[2], t.shape[1] * 64)


def rms(x: torch.Tensor) -> float:
    return math.sqrt(float((x.double() ** 2).mean()))


def evidence_input(dtype, nkv, in_scale, seed, nq=256):
    """The one-head input of the model-vs-truth pin: rows 0..2 = all-equal logits / a dominant early key / a dominant late
    key (as tests/test_kernels_gpu.py::test_attention), the rest of q and k N(0, in_scale^2), v N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    q = (torch.randn(nq, 64, generator=g) * in_scale).to(dtype)
    k = (torch.randn(nkv, 64, generator=g) * in_scale).to(dtype)
    v = torch.randn(nkv, 64, generator=g).to(dtype)
    q[0] = 0
    q[1] = k[min(5, nkv - 1)] * 4
    q[2] = k[nkv - 3] * 4
    return q, k, v
