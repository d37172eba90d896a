"""omg_transpose_v_mapped and the "mixed" cross-attention layer built on it (-m gpu).

Kernel group: the two V^T images against exact answers (identity, alpha = 0, a permutation with alpha in {0, 1}: every output element
is one input element or zero, so the images must be bit-equal to the plain transpose of the gathered / masked V) and against a float64
evaluation within one ulp of the 16-bit format for fractional tables; padding, canaries, plain rows, the device step index, a NaN
behind zero coefficients, and the OMG_EINVAL cases.

Attention group: a tiny Attention module through RegionControlNet_AttnProcessor with a word-swap controller, against the reference
sequence (softmax -> controller edit -> probs V) in float64 on the module's own rounded q, k, v, at the project's kernel tolerance
(2e-3 relative + 2e-3 absolute in fp16, 1.6e-2 in bf16; the one extra rounding of V' is 2^-11 relative)."""
import numpy as np
import pytest
import torch

from omg_amd import _lib as L
from omg_amd import controller as pc
from omg_amd import ops
from omg_amd.attention import Attention, RegionControlNet_AttnProcessor
from oracle import controller as oc

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
NKVS = [1, 15, 16, 17, 63, 64, 65, 77, 128]
EDIT_OF = [-1, 0, -1, 1, 0]
B, E, STEPS, TW = 5, 2, 4, 128             # TW: width of the tables (ld of the mapper > Nkv for every Nkv but 128)
CANARY = 1234.0
GUARD = 64


def canary_out(heads, pad, dtype, dev):
    """An output image inside a larger canary-filled allocation: (whole buffer, the image view)."""
    n = B * heads * 64 * pad
    buf = torch.full((n + 2 * GUARD,), CANARY, dtype=dtype, device=dev)
    return buf, buf[GUARD: GUARD + n].view(B, heads, 64, pad)


def guards_intact(buf):
    return bool((buf[:GUARD] == CANARY).all()) and bool((buf[-GUARD:] == CANARY).all())


def run(v, heads, mapper, alpha, step, dev, edit_of=EDIT_OF):
    Nkv = v.shape[1]
    pad = (Nkv + 63) // 64 * 64
    bm, vm = canary_out(heads, pad, v.dtype, dev)
    bo, vo = canary_out(heads, pad, v.dtype, dev)
    eo = torch.tensor(edit_of, dtype=torch.int32, device=dev)
    st = None if step is None else torch.tensor([step], dtype=torch.int32, device=dev)
    ops.transpose_v_mapped(v, heads, eo, mapper.to(dev), alpha.to(dev), st, out=(vm, vo))
    torch.cuda.synchronize()
    assert guards_intact(bm) and guards_intact(bo)
    return vm, vo


def make_v(Nkv, heads, dtype, dev, seed=0):
    """V as the [k|v] projection holds it: the right half of a (B, Nkv, 2 * heads * 64) buffer."""
    g = torch.Generator().manual_seed(seed * 1000 + Nkv * 7 + heads)
    kv = torch.randn(B, Nkv, 2 * heads * 64, generator=g).to(dtype).to(dev)
    return kv[:, :, heads * 64:]


def tables(Nkv, kind, seed=0):
    """(mapper (E, TW, TW), alpha (STEPS, E, TW)) fp32 on the host; entries beyond Nkv hold garbage the kernel must not read into the result."""
    g = torch.Generator().manual_seed(seed * 77 + Nkv)
    mapper = torch.full((E, TW, TW), 7.0)
    alpha = torch.full((STEPS, E, TW), 0.5)
    for e in range(E):
        m = torch.zeros(Nkv, Nkv)
        if kind in ("identity", "zero_alpha"):
            m = torch.eye(Nkv)
        elif kind == "permutation":
            m[torch.arange(Nkv), torch.randperm(Nkv, generator=g)] = 1
        else:                                   # multi-piece words: rows spreading 1/2 or 1/3 over two or three keys
            for w in range(Nkv):
                cnt = min(Nkv, 2 + (w + e) % 2)
                cols = torch.randperm(Nkv, generator=g)[:cnt]
                m[w, cols] = 1.0 / cnt
        mapper[e, :Nkv, :Nkv] = m
    if kind == "identity":
        alpha[:, :, :Nkv] = 1
    elif kind == "zero_alpha":
        alpha[:, :, :Nkv] = 0
    elif kind == "permutation":
        alpha[:, :, :Nkv] = (torch.rand(STEPS, E, Nkv, generator=g) < 0.5).float()
    else:
        alpha[:, :, :Nkv] = torch.rand(STEPS, E, Nkv, generator=g)
    return mapper, alpha


def padding_is_zero(vt, Nkv):
    """Columns >= Nkv of the MFMA key order: positions whose key index is >= Nkv."""
    pad = vt.shape[3]
    idx = np.array([g * 16 + (r // 8) * 4 + (r % 4) + ((r % 8) // 4) * 8 for g in range(pad // 16) for r in range(16)])
    return bool((vt[..., torch.from_numpy(idx >= Nkv).to(vt.device)] == 0).all())


@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("Nkv", NKVS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_answer_tables(dev, dtype, Nkv, heads):
    v = make_v(Nkv, heads, dtype, dev)
    plain = ops.transpose_v(v, heads)
    zero = torch.zeros_like(plain)
    edited = torch.tensor(EDIT_OF) >= 0
    # M = I, alpha = 1: the mapped image is the plain transpose, the own image is zero
    vm, vo = run(v, heads, *tables(Nkv, "identity"), 1, dev)
    assert torch.equal(vm, plain) and torch.equal(vo, zero)
    # alpha = 0: the roles swap (on the edited rows; the others stay plain / zero)
    vm, vo = run(v, heads, *tables(Nkv, "zero_alpha"), 1, dev)
    assert torch.equal(vm[edited], zero[edited]) and torch.equal(vo[edited], plain[edited])
    assert torch.equal(vm[~edited], plain[~edited]) and torch.equal(vo[~edited], zero[~edited])
    # a permutation with alpha in {0, 1}: gather / mask, exactly
    mapper, alpha = tables(Nkv, "permutation")
    for step in (0, 2, STEPS - 1):              # the device step index alone selects the alpha row
        vm, vo = run(v, heads, mapper, alpha, step, dev)
        g1, g2 = v.clone(), torch.zeros_like(v)
        for b, e in enumerate(EDIT_OF):
            if e < 0:
                continue
            a = alpha[step, e, :Nkv].to(dev)
            src = mapper[e, :Nkv, :Nkv].argmax(dim=1).to(dev)
            g1[b] = (v[b].float() * a[:, None])[src].to(dtype)
            g2[b] = (v[b].float() * (1 - a)[:, None]).to(dtype)
        assert torch.equal(vm, ops.transpose_v(g1, heads)), step
        assert torch.equal(vo, ops.transpose_v(g2, heads)), step
        assert padding_is_zero(vm, Nkv) and padding_is_zero(vo, Nkv)
    vm0, vo0 = run(v, heads, mapper, alpha, None, dev)          # no step index: row 0
    vm1, vo1 = run(v, heads, mapper, alpha, 0, dev)
    assert torch.equal(vm0, vm1) and torch.equal(vo0, vo1)


def ulp(ref, dtype):
    """Spacing of ``dtype`` at |ref| (float64 tensor): 2^(floor(log2 |ref|) - mantissa bits), not below the smallest subnormal's."""
    mant, emin = (10, -14) if dtype == torch.float16 else (7, -126)
    ex = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** emin)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), ex - mant)


@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("Nkv", NKVS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_fractional_tables_within_one_ulp_of_float64(dev, dtype, Nkv, heads):
    v = make_v(Nkv, heads, dtype, dev, seed=1)
    mapper, alpha = tables(Nkv, "fractional", seed=1)
    step = 2
    vm, vo = run(v, heads, mapper, alpha, step, dev)
    assert padding_is_zero(vm, Nkv) and padding_is_zero(vo, Nkv)
    plain = ops.transpose_v(v, heads)
    v64 = v.double().cpu()
    r1, r2 = v64.clone(), torch.zeros_like(v64)
    for b, e in enumerate(EDIT_OF):
        if e < 0:
            continue
        a = alpha[step, e, :Nkv].double()
        r1[b] = (mapper[e, :Nkv, :Nkv].double() * a[None, :]) @ v64[b]
        r2[b] = (1 - alpha[step, e, :Nkv]).double()[:, None] * v64[b]          # 1 - alpha is formed in fp32, as the kernel forms it
    # the same layout through the plain transpose of a float32 image is not available on the device: index the outputs instead
    pad = vm.shape[3]
    pos = torch.tensor([g * 16 + (r // 8) * 4 + (r % 4) + ((r % 8) // 4) * 8 for g in range(pad // 16) for r in range(16)])
    keep = pos < Nkv
    for got, ref in ((vm, r1), (vo, r2)):
        got = got.double().cpu()[..., keep]                                    # (B, heads, 64, Nkv) in key order pos[keep]
        want = ref.view(B, Nkv, heads, 64).permute(0, 2, 3, 1)[..., pos[keep]]
        err = (got - want).abs()
        assert bool((err <= ulp(want, dtype)).all()), (err / ulp(want, dtype)).max().item()
    for b, e in enumerate(EDIT_OF):                                            # plain rows: bit-equal to omg_transpose_v, own image zero
        if e < 0:
            assert torch.equal(vm[b], plain[b]) and not bool(vo[b].any())


@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_behind_zero_coefficients_does_not_reach_the_output(dev, dtype):
    Nkv, heads = 77, 3
    v = make_v(Nkv, heads, dtype, dev, seed=2).clone()
    bad = 40
    v[1, bad] = float("nan")                   # sample 1 is edit 0
    v[3, bad] = float("inf")                   # sample 3 is edit 1
    mapper, alpha = tables(Nkv, "fractional", seed=2)
    mapper[:, :Nkv, bad] = 0                   # no output key draws on key `bad` ...
    alpha[:, :, bad] = 1                       # ... and 1 - alpha is exactly 0 there
    vm, vo = run(v, heads, mapper, alpha, 1, dev)
    assert bool(torch.isfinite(vm.float()).all()) and bool(torch.isfinite(vo.float()).all())
    alpha[:, :, bad] = 0                       # alpha = 0: the mapped coefficients M * alpha vanish, the own image carries the row
    mapper[:, :Nkv, bad] = 0.5
    vm, vo = run(v, heads, mapper, alpha, 1, dev)
    assert bool(torch.isfinite(vm.float()).all())
    assert bool(torch.isnan(vo[1].float()).any()) and bool(torch.isinf(vo[3].float()).any())


def test_bad_arguments_are_einval_and_write_nothing(dev):
    heads, dtype = 2, torch.float16
    eo = torch.tensor(EDIT_OF, dtype=torch.int32, device=dev)
    wide_m, wide_a = torch.zeros(E, 136, 136, device=dev), torch.zeros(STEPS, E, 136, device=dev)

    def refused(v, mapper, alpha, pad):
        bm, vm = canary_out(heads, pad, dtype, dev)
        bo, vo = canary_out(heads, pad, dtype, dev)
        with pytest.raises(L.OmgHipError, match="omg_transpose_v_mapped"):
            ops.transpose_v_mapped(v, heads, eo, mapper, alpha, None, nkv_pad=pad, out=(vm, vo))
        torch.cuda.synchronize()
        assert bool((bm == CANARY).all()) and bool((bo == CANARY).all())

    good = torch.randn(B, 77, heads * 64, device=dev).to(dtype)
    refused(torch.randn(B, 129, heads * 64, device=dev).to(dtype), wide_m, wide_a, 192)          # Nkv > 128
    refused(torch.randn(B, 77, heads * 64 + 2, device=dev).to(dtype)[:, :, :heads * 64], wide_m, wide_a, 128)      # ldv % 8 != 0
    refused(torch.randn(B, 77, heads * 64 + 8, device=dev).to(dtype)[:, :, 4:heads * 64 + 4], wide_m, wide_a, 128)  # V not 16-byte aligned
    refused(good, wide_m[:0], wide_a[:, :0], 128)                                                 # E = 0
    refused(good, wide_m, wide_a[:0], 128)                                                        # steps = 0
    a = L.VMapArgs()                                                                              # Nkv_pad not a multiple of 64, straight at the ABI
    bm, vm = canary_out(heads, 128, dtype, dev)
    a.dtype, a.B, a.heads, a.Nkv, a.Nkv_pad = 0, B, heads, 77, 96
    a.V, a.ldv, a.v_bstride = good.data_ptr(), good.stride(1), good.stride(0)
    a.edit_of, a.E, a.steps = eo.data_ptr(), E, STEPS
    a.mapper, a.ld_mapper, a.mapper_estride = wide_m.data_ptr(), 136, 136 * 136
    a.alpha, a.alpha_step_stride, a.alpha_estride = wide_a.data_ptr(), E * 136, 136
    a.Vt_mapped = a.Vt_own = vm.data_ptr()
    import ctypes
    assert L.lib().omg_transpose_v_mapped(ctypes.byref(a), None) != 0
    assert b"Nkv_pad" in L.lib().omg_last_error()
    torch.cuda.synchronize()
    assert bool((bm == CANARY).all())


# ------------------------------------------------------------------ attention level
PROMPTS = ["a man on the road", "a woman on the road"]
WINDOWS = {"default_": 0.6, "road": (0.2, 0.9)}
P2P_STEPS = 8
TOL = {torch.float16: 2e-3, torch.bfloat16: 1.6e-2}
C = 128                                      # 2 heads of 64


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


def _module(dtype, dev):
    """Cross-attention with an identity out-projection: the module's output IS the attention output, rounded once."""
    attn = Attention(C, C, 2, dtype=dtype, device=dev)
    g = torch.Generator().manual_seed(11)
    sd = {f"to_{n}.weight": (0.1 * torch.randn(C, C, generator=g)).to(dtype).to(dev) for n in "qkv"}
    sd["to_out.0.weight"] = torch.eye(C).to(dtype).to(dev)
    sd["to_out.0.bias"] = torch.zeros(C).to(dtype).to(dev)
    attn.load_state_dict(sd)
    return attn


def _reference(attn, x, ctx, images, step):
    """softmax -> AttentionReplaceOracle -> probs V in float64 on the module's own rounded q, k, v; per request block of four rows."""
    q, k, v = (t.double().cpu() for t in (attn.to_q(x), attn.to_k(ctx), attn.to_v(ctx)))
    octl = oc.AttentionReplaceOracle(PROMPTS, P2P_STEPS, dict(WINDOWS), (0.0, 0.5), 4, 4, tokenizer=oc.PieceTokenizer())
    octl.num_att_layers = 1 << 30
    N = q.shape[1]
    h2b = lambda t: t.reshape(4, t.shape[1], 2, 64).permute(0, 2, 1, 3).reshape(8, t.shape[1], 64)      # head_to_batch_dim of one block
    out = []
    for j in range(images):
        qb, kb, vb = (h2b(t[4 * j: 4 * j + 4]) for t in (q, k, v))
        probs = torch.softmax(qb @ kb.transpose(-1, -2) * 64 ** -0.5, dim=-1)                            # get_attention_scores
        octl.cur_step = step
        probs = octl(probs, True, "mid")                                                                 # the controller's in-place edit
        out.append((probs @ vb).reshape(4, 2, N, 64).permute(0, 2, 1, 3).reshape(4, N, C))               # bmm + batch_to_head_dim
    return torch.cat(out)


@pytest.mark.parametrize("images", [1, 3])
@pytest.mark.parametrize("Nq", [16, 100])
@pytest.mark.parametrize("dtype", DTYPES)
def test_mixed_cross_layer_matches_the_reference_sequence(dev, dtype, Nq, images, monkeypatch):
    attn = _module(dtype, dev)
    ctl = pc.AttentionReplace(PROMPTS, P2P_STEPS, dict(WINDOWS), (0.0, 0.5), 4, 4, tokenizer=oc.PieceTokenizer(), device=dev, dtype=dtype)
    ctl.num_att_layers = 1 << 30
    proc = RegionControlNet_AttnProcessor(controller=ctl, place_in_unet="mid")
    attn.set_processor(proc)
    g = torch.Generator().manual_seed(Nq + images)
    x = torch.randn(4 * images, Nq, C, generator=g).to(dtype).to(dev)
    ctx = torch.randn(4 * images, 77, C, generator=g).to(dtype).to(dev)
    kw = dict(omg_main_batch=4, omg_images=images)
    for step in (0, 6):                        # "road" not yet replaced / only "road" still replaced: both "mixed"
        ctl.cur_step = step
        assert ctl.cross_kind() == "mixed"
        ref = _reference(attn, x, ctx, images, step)
        attn(x, encoder_hidden_states=ctx, **kw)                               # fills the projection cache outside the count
        ctl.cur_step = step
        proxy, matmuls = _CountingLib(L.lib()), []
        real_matmul = torch.matmul
        monkeypatch.setattr(L, "_lib", proxy)
        monkeypatch.setattr(torch, "matmul", lambda *a, **k: (matmuls.append(1), real_matmul(*a, **k))[1])
        try:
            y = attn(x, encoder_hidden_states=ctx, **kw)
        finally:
            monkeypatch.undo()
        assert "omg_attn_probs" not in proxy.calls and "omg_attn_apply_probs" not in proxy.calls and not matmuls, proxy.calls
        assert proxy.calls["omg_transpose_v_mapped"] == 1 and proxy.calls["omg_attn_fwd"] == 2, proxy.calls
        err = (y.double().cpu() - ref).abs()
        bound = TOL[dtype] * (1 + ref.abs())
        print(f"{dtype} Nq={Nq} images={images} step={step}: max err {err.max().item():.3e}, max err/bound {(err / bound).max().item():.3f}")
        assert bool((err <= bound).all())
        # the check above must be able to tell the edit from no edit: somewhere in the edited row the unedited attention lies more
        # than twice the bound away from the reference, so a path that skipped the edit would miss the tolerance
        plain = (ref.view(images, 4, Nq, C)[:, 3] - _plain(attn, x, ctx).view(images, 4, Nq, C)[:, 3]).abs()
        assert bool((plain > 2 * bound.view(images, 4, Nq, C)[:, 3]).any()), "the edit must be visible in the edited row"
        if images == 1:                        # the explicit switch: the reference's literal sequence on materialised probabilities
            proc.force_protocol = True
            ctl.cur_step = step
            proxy = _CountingLib(L.lib())
            monkeypatch.setattr(L, "_lib", proxy)
            try:
                yp = attn(x, encoder_hidden_states=ctx, **kw)
            finally:
                monkeypatch.undo()
                proc.force_protocol = False
            assert proxy.calls.get("omg_attn_probs") == 1 and proxy.calls.get("omg_attn_apply_probs") == 1
            errp = (yp.double().cpu() - ref).abs()
            print(f"    force_protocol: max err {errp.max().item():.3e}, max err/bound {(errp / bound).max().item():.3f}")


def _plain(attn, x, ctx):
    q, k, v = (t.double().cpu() for t in (attn.to_q(x), attn.to_k(ctx), attn.to_v(ctx)))
    Bq, N, _ = q.shape
    h = lambda t: t.reshape(Bq, t.shape[1], 2, 64).permute(0, 2, 1, 3)
    o = torch.softmax(h(q) @ h(k).transpose(-1, -2) * 0.125, dim=-1) @ h(v)
    return o.permute(0, 2, 1, 3).reshape(Bq, N, C)


def test_borrow_and_own_steps_are_one_launch_and_batches_are_accepted(dev, monkeypatch):
    """Equal prompts with cross_replace_steps = 0.5: "borrow" steps are the pure path's single launch with qk_src, "own" steps a plain
    attention — for three requests at once (protocol mode refused more than one)."""
    dtype = torch.float16
    attn = _module(dtype, dev)
    ctl = pc.AttentionReplace([PROMPTS[0]] * 2, P2P_STEPS, 0.5, (0.0, 0.5), 4, 4, device=dev, dtype=dtype)
    ctl.num_att_layers = 1 << 30
    attn.set_processor(RegionControlNet_AttnProcessor(controller=ctl, place_in_unet="mid"))
    g = torch.Generator().manual_seed(5)
    x = torch.randn(12, 16, C, generator=g).to(dtype).to(dev)
    ctx = torch.randn(12, 77, C, generator=g).to(dtype).to(dev)
    q = attn.to_q(x)
    k, vt = attn.project_cross(ctx)
    src = ctl.qk_src_vector(4, dev, 12, 3)
    want = {0: ops.attention(q, k, vt, 2, attn.scale, qk_src=src), 7: ops.attention(q, k, vt, 2, attn.scale)}
    for step, kind in ((0, "borrow"), (7, "own")):
        ctl.cur_step = step
        assert ctl.cross_kind() == kind
        proxy = _CountingLib(L.lib())
        monkeypatch.setattr(L, "_lib", proxy)
        try:
            y = attn(x, encoder_hidden_states=ctx, omg_main_batch=4, omg_images=3)
        finally:
            monkeypatch.undo()
        assert proxy.calls["omg_attn_fwd"] == 1 and "omg_transpose_v_mapped" not in proxy.calls and "omg_attn_probs" not in proxy.calls
        assert torch.equal(y, want[step])
