"""The yardstick of tests/test_gemm_tiles_gpu.py, CPU only: float64 references of ``ops.gemm`` and ``ops.conv2d`` that use no project
kernel, the cases at which each GEMM tile can go wrong, and the two ways a result is judged.

*Exact cases.*  ``x`` and ``w`` hold -1 / 0 / 1 (``w`` sparse), ``bias`` / ``group_bias`` / ``residual`` integers in [-4, 4], ``out_scale``
is 1, 0.5 or 2: every product and every partial sum is a small integer (or half of one), exact in fp32 in ANY summation order, and the
result is exactly representable in fp16 and bf16 — the generator asserts it.  A kernel is right on such a case iff it returns the
reference bit for bit; a wrong tap, channel offset, tile edge or operand stride moves some output by at least 1/2.

*Random cases.*  Linear epilogues only.  The contract of csrc/gemm_epilogue.h is fp32 accumulation that starts at the bias, then
``fma(v, out_scale, residual)`` and ONE rounding at the store, so

    |out - ref64| <= 0.5 ulp_dtype(|ref64|) + (K + K2 + 4) 2^-23 S,
    S = |out_scale| (|A| |W|^T + |A2| |W2|^T + |bias| + |group_bias|) + |residual|         (float64)

The first term is the rounding at the store, the second the bound of K + K2 + 4 fp32 operations in any order with truncating adds
(each errs at most 2^-23 of a partial result that is at most S).  Both are derived, neither is measured.  tests/test_gemm_oracle.py
shows that the bound accepts the once-rounded reference and rejects one that is rounded before the residual is added — except on
``BLIND``, where the second term alone is already larger than the rounding too many.
"""
import functools

import torch
import torch.nn.functional as F

DTYPES = [torch.float16, torch.bfloat16]
VARIANTS = [1, 13, 14, 15, 24, 25, 28]       # csrc/gemm.hip g_variant: 128x128 | v6 256x256, 256x128 | v7 256x256, 128x320 | v12 256x256 | v13 256x320
SETTINGS = VARIANTS + [0]                    # 0 = the heuristic
FMT = {torch.float16: (10, -14), torch.bfloat16: (7, -126)}      # stored mantissa bits p, smallest normal exponent e_min
# The extra rounding of a twice-rounded result errs at most half an ulp of the value it rounds.  Where (K + 4) 2^-23 S is at least that
# on every output, no bound of this form can refuse it: the two fp16 convolutions with K = 1152 and K = 1728.  There the bound still
# holds the kernel to fp32 accumulation, it just cannot tell one rounding from two.
BLIND = {("concat", torch.float16), ("up", torch.float16)}
COUT = 328                                   # one whole 320 tile + 8 | 256 + 72 | 2 x 128 + 72


def round16(x64: torch.Tensor, dtype) -> torch.Tensor:
    return x64.to(dtype).double()


def ulp(x64: torch.Tensor, dtype) -> torch.Tensor:
    """2^(max(floor(log2 |x|), e_min) - p): the spacing of ``dtype`` at |x| (subnormal spacing below 2^e_min and at 0)."""
    p, e_min = FMT[dtype]
    ax = x64.abs().double()
    _, e = torch.frexp(ax)                                  # ax = m 2^e, m in [0.5, 1): floor(log2 ax) = e - 1
    fl = torch.where(ax == 0, torch.full_like(e, e_min), e - 1).clamp_min(e_min)
    return torch.ldexp(torch.ones_like(ax), fl - p)


def bound(ref64: torch.Tensor, S: torch.Tensor, K: int, K2: int, dtype) -> torch.Tensor:
    return 0.5 * ulp(ref64, dtype) + (K + K2 + 4) * 2.0 ** -23 * S


# ------------------------------------------------------------------------------------------------ float64 references
def _epilogue(acc, act, out_scale, residual):
    if act == "silu":
        acc = acc * torch.sigmoid(acc)
    elif act == "geglu":
        # packed row p of W (ops.geglu_row_perm): block p // 64; j = p % 64 < 32 is value column 32 block + j, else the gate of column 32 block + j - 32
        M, N = acc.shape
        h = acc.view(M, N // 64, 2, 32)
        acc = (h[:, :, 0] * F.gelu(h[:, :, 1])).reshape(M, N // 2)
    else:
        assert act == "none"
    out = acc * out_scale
    return out if residual is None else out + residual.double()


def gemm_ref64(a, w, *, bias=None, group_bias=None, groups=1, out_scale=1.0, residual=None, act="none", adapter=None, out_init=None,
               a2=None, w2=None):
    """``ops.gemm`` on the operands the kernel gets, in float64.  ``w`` 3-D: weight slots, ``adapter[g]`` picks group g's and -1 leaves
    the group's rows at ``out_init``.  ``a2`` / ``w2``: the second K-segment, added for the groups whose adapter is >= 0.  ``act``:
    "none" | "silu" | "geglu" (``w`` / ``bias`` in the packed row order)."""
    a = a.double()
    M = a.shape[0]
    rows = M // groups
    assert rows * groups == M
    N = w.shape[-2]
    acc = torch.zeros(M, N, dtype=torch.float64)
    skipped = torch.zeros(M, dtype=torch.bool)
    for g in range(groups):
        sl = slice(g * rows, (g + 1) * rows)
        slot = 0 if adapter is None else int(adapter[g])
        if w.dim() == 3 and slot < 0:
            skipped[sl] = True
            continue
        acc[sl] = a[sl] @ (w[slot] if w.dim() == 3 else w).double().T
        if a2 is not None and slot >= 0:
            acc[sl] += a2[sl].double() @ (w2[slot] if w2.dim() == 3 else w2).double().T
        if group_bias is not None:
            acc[sl] += group_bias[g].double()
    if bias is not None:
        acc = acc + bias.double()
    out = _epilogue(acc, act, out_scale, residual)
    if skipped.any():
        out[skipped] = out_init.double()[skipped] if torch.is_tensor(out_init) else float(out_init)
    return out


def unpack_conv_weight(w_packed, ksize):
    """[Cout, ksize * ksize * C] with K = (tap row, tap column, channel) -> OIHW."""
    co, K = w_packed.shape
    return w_packed.view(co, ksize, ksize, K // (ksize * ksize)).permute(0, 3, 1, 2)


def conv_acc64(x1, w_packed, ksize, *, stride=1, upsample=False, x2=None):
    """The convolution alone (no bias), NHWC in, NHWC float64 out: nearest 2x upsample, then the channel concat x1 | x2, then
    F.conv2d in double on NCHW with padding ksize // 2."""
    x = (x1 if x2 is None else torch.cat([x1, x2], dim=-1)).double().permute(0, 3, 1, 2)
    if upsample:
        x = x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    y = F.conv2d(x, unpack_conv_weight(w_packed.double(), ksize), None, stride=stride, padding=ksize // 2)
    return y.permute(0, 2, 3, 1).contiguous()


def conv_epilogue64(acc, *, bias=None, group_bias=None, out_scale=1.0, residual=None, act="none"):
    B, H, W, Co = acc.shape
    if bias is not None:
        acc = acc + bias.double()
    if group_bias is not None:
        acc = acc + group_bias.double()[:, None, None, :]
    return _epilogue(acc.reshape(-1, Co), act, out_scale, None if residual is None else residual.reshape(-1, Co)).view(B, H, W, Co)


def conv2d_ref64(x1, w_packed, ksize, *, stride=1, upsample=False, x2=None, **epi):
    return conv_epilogue64(conv_acc64(x1, w_packed, ksize, stride=stride, upsample=upsample, x2=x2), **epi)


# ------------------------------------------------------------------------------------------------ data
def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * ord(c) for i, c in enumerate("/".join(map(str, key)))) % (2 ** 31))


def tern(g, *shape, density=None):
    """-1 / 0 / 1 as float64: uniform, or (``density``) +-1 at that fraction of the places."""
    if density is None:
        return torch.randint(-1, 2, shape, generator=g).double()
    return (torch.randint(0, 2, shape, generator=g).double() * 2 - 1) * (torch.rand(shape, generator=g) < density) + 0.0       # + 0.0: no negative zeros


def ints(g, *shape):
    return torch.randint(-4, 5, shape, generator=g).double()


def rnd(g, *shape, dtype, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def density(K, sigma=8.0):
    """Weight density at which a sum of K products of a uniform -1 / 0 / 1 with a +-1 has standard deviation ``sigma``: large enough
    that few outputs are 0, small enough that the largest of 10^5 outputs (4.5 sigma) stays far below bf16's 256."""
    return min(0.75, sigma * sigma / (K * 2.0 / 3.0))


def assert_exact_case(ref64, what):
    """An exact case is usable iff its reference is representable in both dtypes and is no degenerate (small or mostly-zero) matrix."""
    for dt in DTYPES:
        bad = (round16(ref64, dt) != ref64).nonzero()
        assert bad.numel() == 0, f"{what}: the reference is not representable in {dt} at {bad[0].tolist()}: {ref64[tuple(bad[0])].item()}"
    assert float(ref64.abs().max()) >= 8, f"{what}: max |ref| {float(ref64.abs().max())} < 8"
    zeros = float((ref64 == 0).double().mean())
    assert zeros < 0.25, f"{what}: {zeros:.0%} of the outputs are zero"


# ------------------------------------------------------------------------------------------------ convolution cases
# B = 3 and a 13 x 11 output: M = 429 = one 256-row tile + 173 = three 128-row tiles + 45; the sample boundaries (rows 143, 286) fall
# inside a tile and image edges in every wave.  "folded": rows per sample % 256 == 0, the group bias starts the accumulator.
CONV_CASES = {
    "s1": dict(B=3, H=13, W=11, C1=64, C2=0, k=3, s=1, up=False),
    "concat": dict(B=3, H=13, W=11, C1=128, C2=64, k=3, s=1, up=False),
    "s2_odd": dict(B=3, H=25, W=21, C1=64, C2=0, k=3, s=2, up=False),
    "s2_even": dict(B=3, H=26, W=22, C1=64, C2=0, k=3, s=2, up=False),
    "up": dict(B=3, H=7, W=5, C1=64, C2=64, k=3, s=1, up=True),
    "1x1_concat": dict(B=3, H=13, W=11, C1=64, C2=64, k=1, s=1, up=False),       # K = 128: two stages
    "1x1_one_stage": dict(B=3, H=13, W=11, C1=64, C2=0, k=1, s=1, up=False),     # K = 64
    "1x1_s2": dict(B=3, H=25, W=21, C1=64, C2=0, k=1, s=2, up=False),
    "1x1_up": dict(B=3, H=7, W=5, C1=64, C2=0, k=1, s=1, up=True),
    "folded": dict(B=2, H=16, W=16, C1=64, C2=0, k=3, s=1, up=False),
}
# epilogue -> (group bias, residual, out_scale, act); "silu" runs on random data only
CONV_EPILOGUES = {"bias": (False, False, 1.0, "none"), "group_bias": (True, False, 2.0, "none"), "residual": (False, True, 0.5, "none"),
                  "silu": (True, False, 1.0, "silu")}
LINEAR_EPILOGUES = ["bias", "group_bias", "residual"]


def conv_out_hw(c):
    Hl, Wl = (2 * c["H"], 2 * c["W"]) if c["up"] else (c["H"], c["W"])
    pad = c["k"] // 2
    return (Hl + 2 * pad - c["k"]) // c["s"] + 1, (Wl + 2 * pad - c["k"]) // c["s"] + 1


@functools.lru_cache(maxsize=None)
def conv_case(name, kind, dtype=None):
    """Operands (CPU; float64 integers for kind "int", ``dtype`` for "rnd"), the float64 accumulator and — "rnd" — the accumulator of
    the absolute values.  Computed once and shared by every variant; nobody writes to it."""
    c = CONV_CASES[name]
    g = _gen("conv", name, kind, dtype)
    Ct, K = c["C1"] + c["C2"], c["k"] ** 2 * (c["C1"] + c["C2"])
    Ho, Wo = conv_out_hw(c)
    shp = lambda C: (c["B"], c["H"], c["W"], C)
    if kind == "int":
        d = dict(x1=tern(g, *shp(c["C1"])), x2=tern(g, *shp(c["C2"])) if c["C2"] else None, w=tern(g, COUT, K, density=density(K)),
                 bias=ints(g, COUT), group_bias=ints(g, c["B"], COUT), residual=ints(g, c["B"], Ho, Wo, COUT))
    else:
        d = dict(x1=rnd(g, *shp(c["C1"]), dtype=dtype), x2=rnd(g, *shp(c["C2"]), dtype=dtype) if c["C2"] else None,
                 w=rnd(g, COUT, K, dtype=dtype, scale=K ** -0.5), bias=rnd(g, COUT, dtype=dtype), group_bias=rnd(g, c["B"], COUT, dtype=dtype),
                 residual=rnd(g, c["B"], Ho, Wo, COUT, dtype=dtype))
    geo = dict(stride=c["s"], upsample=c["up"])
    d.update(geo=geo, K=K, ksize=c["k"], out_shape=(c["B"], Ho, Wo, COUT))
    d["acc"] = conv_acc64(d["x1"], d["w"], c["k"], x2=d["x2"], **geo)
    if kind == "rnd":
        d["acc_abs"] = conv_acc64(d["x1"].abs(), d["w"].abs(), c["k"], x2=None if d["x2"] is None else d["x2"].abs(), **geo)
    return d


def conv_epi_args(d, epi):
    gb, res, scale, act = CONV_EPILOGUES[epi]
    return dict(bias=d["bias"], group_bias=d["group_bias"] if gb else None, residual=d["residual"] if res else None, out_scale=scale, act=act)


@functools.lru_cache(maxsize=None)
def conv_expected(name, kind, dtype, epi):
    """(ref64, S): S is None on the exact cases (no tolerance) and under SiLU (judged by the suite's TOL)."""
    d = conv_case(name, kind, dtype)
    e = conv_epi_args(d, epi)
    ref = conv_epilogue64(d["acc"], **e)
    if kind == "int":
        assert_exact_case(ref, f"conv {name} / {epi}")
        return ref, None
    if e["act"] != "none":
        return ref, None
    ab = {k: (v.abs() if torch.is_tensor(v) else v) for k, v in e.items()}
    return ref, conv_epilogue64(d["acc_abs"], **ab)


def conv_twice_rounded(name, dtype):
    """The "residual" epilogue of a random case with a rounding too many: the scaled accumulator rounded to ``dtype``, then the residual
    -> (the scaled accumulator before its rounding, the twice-rounded result)."""
    d = conv_case(name, "rnd", dtype)
    e = conv_epi_args(d, "residual")
    pre = conv_epilogue64(d["acc"], **{**e, "residual": None})
    return pre, round16(round16(pre, dtype) + d["residual"].double(), dtype)


# ------------------------------------------------------------------------------------------------ plain GEMM cases
# name -> M, N, K, groups and what is special.  "layouts": every operand a column slice of a wider buffer (the GPU test builds them).
GEMM_CASES = {
    "tiny": dict(M=4, N=8, K=64, epis=("bias", "residual")),                                  # far below any tile
    "layouts": dict(M=429, N=328, K=192, epis=("residual",), layouts=True),
    "k72": dict(M=429, N=328, K=72, epis=("bias", "residual")),                               # K % 64 != 0: every variant falls through to 128x128
    "slots5": dict(M=385, N=328, K=128, groups=5, epis=("bias",), slots=[1, -1, 0, 0, 1]),    # 77 rows per group, group 1 skipped
    "gb5": dict(M=385, N=328, K=128, groups=5, epis=("group_bias",)),                         # per-row group bias (77 rows: not folded)
    "slots2": dict(M=512, N=328, K=128, groups=2, epis=("bias",), slots=[-1, 1]),
    "gb2": dict(M=512, N=328, K=128, groups=2, epis=("group_bias",)),                         # 256 rows per group: folded
    "lora8": dict(M=429, N=328, K=128, groups=3, epis=("bias",), K2=8, lora=[1, -1, 0]),      # forced variants fall through to 128x128
    "lora64": dict(M=429, N=328, K=128, groups=3, epis=("bias",), K2=64, lora=[1, -1, 0]),
}
GEGLU_CASE = dict(M=429, N=128, K=192)                                                        # random data only
GEMM_EPILOGUES = {"bias": (False, False, 1.0), "group_bias": (True, False, 2.0), "residual": (False, True, 0.5)}
OUT_INIT = 7.0                                                                                # what a skipped group's rows hold before and after


@functools.lru_cache(maxsize=None)
def gemm_case(name, kind, dtype=None):
    """Operands of a plain-GEMM case (CPU).  LoRA cases: ``down`` [2, K2, K] and ``up`` [2, N, K2]; the test runs the down-projection
    (a slot GEMM, adapter -1 skipped) and feeds its result to the second K-segment."""
    c = GEMM_CASES[name]
    g = _gen("gemm", name, kind, dtype)
    M, N, K, G = c["M"], c["N"], c["K"], c.get("groups", 1)
    wshape = (2, N, K) if "slots" in c else (N, K)
    if kind == "int":
        d = dict(a=tern(g, M, K), w=tern(g, *wshape, density=density(K)), bias=ints(g, N), group_bias=ints(g, G, N), residual=ints(g, M, N))
        if "lora" in c:
            # the down-projection stays small (sigma 1.5), so that the second segment's sums of K2 products of it do too
            d["down"] = tern(g, 2, c["K2"], K, density=density(K, 1.5))
            d["up"] = tern(g, 2, N, c["K2"], density=min(0.75, 48.0 / (c["K2"] * 2.25)))
    else:
        d = dict(a=rnd(g, M, K, dtype=dtype), w=rnd(g, *wshape, dtype=dtype, scale=K ** -0.5), bias=rnd(g, N, dtype=dtype),
                 group_bias=rnd(g, G, N, dtype=dtype), residual=rnd(g, M, N, dtype=dtype))
        if "lora" in c:
            d["down"] = rnd(g, 2, c["K2"], K, dtype=dtype, scale=K ** -0.5)
            d["up"] = rnd(g, 2, N, c["K2"], dtype=dtype, scale=0.1)
    adapter = c.get("slots", c.get("lora"))
    d.update(groups=G, K=K, K2=c.get("K2", 0), adapter=None if adapter is None else torch.tensor(adapter, dtype=torch.int32),
             slots="slots" in c, layouts=c.get("layouts", False), epis=c["epis"])
    return d


def gemm_epi_args(d, epi):
    gb, res, scale = GEMM_EPILOGUES[epi]
    return dict(bias=d["bias"], group_bias=d["group_bias"] if gb else None, residual=d["residual"] if res else None, out_scale=scale,
                groups=d["groups"], adapter=d["adapter"], out_init=OUT_INIT)


def lora_down_ref64(d):
    """The down-projection launch of a LoRA case: slot GEMM into zeros, adapter -1 untouched -> (ref64, S)."""
    kw = dict(groups=d["groups"], adapter=d["adapter"], out_init=0.0)
    return gemm_ref64(d["a"], d["down"], **kw), gemm_ref64(d["a"].abs(), d["down"].abs(), **kw)


def gemm_expected(name, kind, dtype, epi, a2=None):
    """(ref64, S) of one epilogue of a case.  LoRA: ``a2`` is the down-projection the second segment reads — kind "int": the exact one
    (default); kind "rnd": the 16-bit tensor the kernel under test produced, i.e. rounded once to the storage dtype."""
    d = gemm_case(name, kind, dtype)
    e = gemm_epi_args(d, epi)
    seg = {}
    if d["K2"]:
        if a2 is None:
            assert kind == "int"
            a2 = lora_down_ref64(d)[0]
            assert all(torch.equal(round16(a2, dt), a2) for dt in DTYPES) and float((a2 != 0).double().mean()) > 0.25, f"gemm {name}: down-projection"
        seg = dict(a2=a2, w2=d["up"])
    ref = gemm_ref64(d["a"], d["w"], **e, **seg)
    if kind == "int":
        assert_exact_case(ref, f"gemm {name} / {epi}")
        return ref, None
    ab = {k: (v.abs() if torch.is_tensor(v) and v.dtype != torch.int32 else v) for k, v in e.items()}
    sega = {k: v.abs() for k, v in seg.items()}
    return ref, gemm_ref64(d["a"].abs(), d["w"].abs(), **ab, **sega)


def gemm_twice_rounded(name, dtype):
    d = gemm_case(name, "rnd", dtype)
    e = gemm_epi_args(d, "residual")
    pre = gemm_ref64(d["a"], d["w"], **{**e, "residual": None})
    return pre, round16(round16(pre, dtype) + d["residual"].double(), dtype)


@functools.lru_cache(maxsize=None)
def geglu_case(dtype):
    """Plain ``w`` / ``bias`` (value rows, then gate rows) of the GEGLU case; the kernel gets them in ops.geglu_row_perm order."""
    c = GEGLU_CASE
    g = _gen("geglu", dtype)
    return dict(a=rnd(g, c["M"], c["K"], dtype=dtype), w=rnd(g, c["N"], c["K"], dtype=dtype, scale=c["K"] ** -0.5), bias=rnd(g, c["N"], dtype=dtype))
