"""The yardstick of tests/test_attention_conditioning_gpu.py pinned on the CPU: the float64 rounding model of the attention
kernels (tests/_attn_model.py) against the float64 truth on three fixed inputs.  The upper figures are the design's error as
it was measured when the GPU bounds were derived from the model (one head, 256 query rows, softmax scale 0.125; rows 0..2
all-equal / dominant-early / dominant-late); a model that errs more than that has grown a rounding point the kernels do
not have, one that errs less than half of it — or less than rounding the true output alone — has lost one, and either way
the GPU module's `C_MAX * max(e_m)` would silently mean something else."""
import pytest
import torch

from tests import _attn_model as M

# dtype, keys, input scale, seed, the design's max error on such inputs
PIN = [
    (torch.float16, 1000, 1.5, 2, 1.1e-3),
    (torch.float16, 130, 3.0, 1, 5.9e-3),      # 16-bit rounding of Q' dominates on large logits (pure output rounding: 9.8e-4)
    (torch.bfloat16, 1000, 1.5, 0, 1.0e-2),
]


@pytest.mark.parametrize("dtype,nkv,in_scale,seed,design_max", PIN)
def test_rounding_model_errs_what_the_design_errs(dtype, nkv, in_scale, seed, design_max):
    q, k, v = M.evidence_input(dtype, nkv, in_scale, seed)
    t = M.truth(q, k, v, 0.125)
    e_m = (M.round16(M.model(q, k, v, 0.125), dtype) - t).abs()
    e_r = (M.round16(t, dtype) - t).abs()
    print(f"{dtype} Nkv {nkv} x{in_scale}: model max {e_m.max():.3e} rms {M.rms(e_m):.3e}; output rounding max {e_r.max():.3e} rms {M.rms(e_r):.3e}")
    assert 0.5 * design_max <= float(e_m.max()) <= design_max
    assert M.rms(e_m) >= M.rms(e_r)


def test_model_is_the_truth_where_nothing_rounds():
    """q = 0 and a one-hot V: Q' = 0, P = 1 exactly, O = count / Nkv: model and truth agree to float64 rounding."""
    k = torch.randn(77, 64, generator=torch.Generator().manual_seed(0)).half()
    v = torch.zeros(77, 64).half()
    v[torch.arange(77), torch.arange(77) % 64] = 1
    q = torch.zeros(5, 64).half()
    t, m = M.truth(q, k, v, 0.125), M.model(q, k, v, 0.125)
    assert float((t - m).abs().max()) < 1e-15
    assert abs(float(t[0, 3]) - 2 / 77) < 1e-15 and abs(float(t[0, 20]) - 1 / 77) < 1e-15


def test_scaled_query_is_exact_at_scale_ln2():
    """The stress tests prescribe log2-unit logits exactly by using scale = ln 2: fp32(scale) * fp32(log2 e) is within an
    fp32 ulp of 1, so Q' = q bit for bit."""
    import math
    q = torch.randn(64, 64, generator=torch.Generator().manual_seed(1))
    for dt in (torch.float16, torch.bfloat16):
        assert torch.equal(M.scaled_query(q.to(dt) * 7, math.log(2.0)), q.to(dt) * 7)
