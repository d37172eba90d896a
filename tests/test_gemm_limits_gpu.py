"""The 16-bit GEMM family and its MX-fp8 siblings at the edge of their 32-bit buffer offsets (-m gpu; the last test needs no GPU).

The large-tile kernels reach every operand through a buffer descriptor and a 32-bit byte offset; ``omg_debug_gemm_offset_limit()``
(csrc/gemm_epilogue.h ``GEMM_OFFSET_LIMIT``) is the operand extent from which the 16-bit entries hand a call to the 128x128 kernel's 64-bit
pointers and the MX-fp8 entries refuse it.  Every case here puts ONE operand's addresses at that edge and keeps the arithmetic trivial:

* the operand is a 64 ... 320 column slice of a buffer with a wide leading dimension, allocated at its full extent (``torch.empty``: every
  address a kernel may form is memory the test owns); only the viewed columns, their neighbours and the row behind the last are filled;
* row i of it is row i mod P of a small integer table, P = 1009 a prime that divides no tile size, so the float64 reference is a
  P-row product and the WHOLE output is compared on the device against that table: a dropped, zeroed or wrapped row anywhere fails;
* all values are small integers (the generator asserts |x| <= 256): exact in fp16, bf16 and in any summation order, compared bit for bit;
* the extents: the last row ending within one row of the limit ("under"), between the limit and 0x7fff0000, where the gates stood
  before the limit was derived from the descriptors' clamp ("window": the large tiles dropped the stores beyond the clamp there),
  2^31 and 2^32 plus a few rows (an unsigned wrap in the 64-bit kernel);
* SiLU and GEGLU are not exact: the first P rows must be bitwise the same call on a P-row problem (batch invariance), every later row
  bitwise periodic, and the P-row result is held to the tolerance tests/test_gemm_tiles_gpu.py holds these epilogues to.
"""
import ctypes
import functools
import os
import re

import pytest
import torch

from omg_amd import _lib as L
from omg_amd import ops
from tests import _gemm_oracle as O

gpu = pytest.mark.gpu

P = 1009                         # period of the rows; prime, divides no tile size
K = 64
N = 320                          # one 320-wide tile | 256 + 64 | 2 x 128 + 64
NG = 128                         # packed GEGLU rows -> 64 output columns
LD = 8192                        # elements per row of a wide buffer (16 KiB)
COL = 8                          # first viewed column of a wide buffer
CANARY = 1000.0                  # representable in both dtypes, larger than any |reference|
FILLER = 3.0                     # next to a read operand's columns: reading it moves an exact sum by a multiple of 3
OLD_GATE = 0x7fff0000            # where the launch gates stood before: the upper end of the "window" extents
EXTENTS = ["under", "window", "2^31", "2^32"]
DID = lambda dt: str(dt)[6:]
VID = lambda v: "heuristic" if v == 0 else f"v{v}"
both_dtypes = pytest.mark.parametrize("dtype", O.DTYPES, ids=DID)


def limit():
    return int(L.lib().omg_debug_gemm_offset_limit())


def rows_ld(extent, row_mult=3, elt=2):
    """(M, ld): M rows of ld elements whose byte extent M * ld * elt — what the launch gates compute — lies where ``extent`` says.
    M is a multiple of ``row_mult`` (the groups of the per-sample forms) and no multiple of P."""
    lim = limit()
    up = lambda m: (m + row_mult - 1) // row_mult * row_mult
    if extent == "under":        # the widest M with M * ld * elt < lim; the leading dimension is searched so that M suits
        for ld in range(LD, LD + 8 * 4096, 8):
            M = (lim - 1) // (ld * elt)
            if M % row_mult == 0 and M % P != 0:
                assert M * ld * elt < lim <= (M + 1) * ld * elt
                return M, ld
        raise AssertionError("no leading dimension found")
    if extent == "window":
        M = up(-(-((lim + OLD_GATE) // 2) // (LD * elt)))
        assert lim + LD * elt * 8 <= M * LD * elt < OLD_GATE, "the window between the limit and the old gate is too narrow for this case"
    else:
        M = up(-(-{"2^31": 2 ** 31, "2^32": 2 ** 32}[extent] // (LD * elt)) + 3)
    if M % P == 0:
        M += row_mult
    return M, LD


def sample_rows(M, ld, elt=2):
    """First and last rows and both sides of the rows in which the byte offset crosses the limit, 2^31 and 2^32."""
    rows = {0, 1, M - 2, M - 1}
    for x in (limit(), 2 ** 31, 2 ** 32):
        r = x // (ld * elt)
        rows.update(q for q in (r - 1, r, r + 1) if 0 <= q < M)
    return sorted(rows)


@functools.lru_cache(maxsize=None)
def tables():
    """The P distinct rows of every operand (CPU float64 integers) and the float64 references of the four epilogue forms."""
    g = O._gen("gemm limits")
    d = dict(a=O.tern(g, P, K), w=O.tern(g, N, K, density=O.density(K)), bias=O.ints(g, N), gb=O.ints(g, 3, N), res=O.ints(g, P, N),
             wg=O.tern(g, NG, K, density=O.density(K, 2.0)), bg=O.ints(g, NG))
    acc = d["a"] @ d["w"].T + d["bias"]
    d["ref_bias"] = acc
    d["ref_residual"] = 2.0 * acc + d["res"]
    for name in ("ref_bias", "ref_residual"):
        O.assert_exact_case(d[name], name)
    for v in list(d.values()) + [acc + d["gb"][i] for i in range(3)]:
        assert float(v.abs().max()) <= 256 and torch.equal(v, v.round())
    return d


def on_dev(dtype, dev, *names):
    t = tables()
    return [t[n].to(dtype).to(dev) for n in names]


def bits(x):
    return x.view(torch.int16)


def periodic(tab, M):
    """[P, n] -> [M, n], row i = tab[i mod P] (a new contiguous tensor)."""
    return tab[torch.arange(M, device=tab.device) % P]


def assert_periodic(out, tab, what):
    """Every row i of ``out`` [M, n] (any row stride) is bitwise ``tab[i mod P]``; compared whole, on the device."""
    M, n = out.shape
    full = M // P * P
    if bool((bits(out[:full]).view(-1, P, n) == bits(tab)).all()) and bool((bits(out[full:]) == bits(tab[:M - full])).all()):
        return
    bad = (bits(out) != bits(periodic(tab, M))).any(dim=1).nonzero().flatten()
    r = int(bad[0])
    c = int((bits(out[r]) != bits(tab[r % P])).nonzero()[0])
    pytest.fail(f"{what}: {bad.numel()} of {M} rows wrong, rows {r}..{int(bad[-1])} (byte offsets {r * out.stride(0) * 2:#x}..); "
                f"first at (row {r}, column {c}): got {out[r, c].item()}, want {tab[r % P, c].item()}")


def assert_rows_match_cpu(out, ref64, rows, what):
    got = out[torch.tensor(rows, device=out.device)].double().cpu()
    want = ref64[torch.tensor(rows) % P]
    assert torch.equal(got, want), f"{what}: sampled rows {[r for r, ok in zip(rows, (got == want).all(dim=1).tolist()) if not ok]} differ from the float64 reference"


class Wide:
    """An output of M rows behind a wide leading dimension: [M + 1, ld] ``torch.empty``; ``arm(n)`` gives the view [:M, COL:COL + n] after
    filling columns 0 .. COL + n + 8 of every row, the row behind the last included, with the canary."""

    def __init__(self, M, ld, dtype, dev):
        self.buf = torch.empty((M + 1) * ld, dtype=dtype, device=dev)
        self.rows = self.buf.view(M + 1, ld)
        self.M, self.n = M, 0

    def arm(self, n):
        self.n = n
        self.rows[:, :COL + n + 8].fill_(CANARY)
        return self.rows[:self.M, COL:COL + n]

    def assert_guards(self, what):
        c = torch.tensor(CANARY, dtype=self.buf.dtype, device=self.buf.device)
        ok = bool((self.rows[:, :COL] == c).all()) and bool((self.rows[:, COL + self.n:COL + self.n + 8] == c).all()) and \
            bool((self.rows[self.M, :COL + self.n + 8] == c).all())
        assert ok, f"{what}: wrote outside the output's column slice or behind its last row"


def wide_input(tab, M, ld, fill=FILLER):
    """``tab``'s rows, periodic, as the column slice [COL, COL + n) of a [M, ld] ``torch.empty`` buffer; the 8 columns on either side hold ``fill``."""
    n = tab.shape[1]
    buf = torch.empty(M * ld, dtype=tab.dtype, device=tab.device)
    rows = buf.view(M, ld)
    rows[:, :COL + n + 8].fill_(fill)
    view = rows[:, COL:COL + n]
    view.copy_(periodic(tab, M))
    return buf, view


@pytest.fixture
def release():
    yield
    torch.cuda.empty_cache()         # one large operand at a time


def forced(v):
    from tests.test_gemm_tiles_gpu import forced as f
    return f(v)


def tol_check(out_small, ref64, dtype, scale):
    from tests.test_gemm_tiles_gpu import assert_tol
    assert_tol(out_small, ref64, dtype, scale=scale)


# ------------------------------------------------------------------------------------------------ omg_gemm: C
@gpu
@both_dtypes
@pytest.mark.parametrize("extent", EXTENTS)
def test_gemm_output_at_the_offset_limit(dev, release, extent, dtype):
    """C behind a wide ldc, every tile kernel, four epilogue forms.  In the "window" the forced large tiles must fall back: before the
    gate was lowered to the limit they ran there and the rows whose bytes lie beyond the descriptors' clamp kept the canary."""
    t = tables()
    M, ld = rows_ld(extent)
    a_tab, w, bias, gb, r_tab, wg, bg = on_dev(dtype, dev, "a", "w", "bias", "gb", "res", "wg", "bg")
    perm = ops.geglu_row_perm(NG).to(dev)
    wg, bg = wg[perm].contiguous(), bg[perm].contiguous()
    a = periodic(a_tab, M)
    res = periodic(r_tab, M)
    rows = sample_rows(M, ld)
    # the non-linear forms on a P-row problem: what the first P rows of the big one must be, bit for bit
    small_silu = ops.gemm(a_tab, w, bias=bias, group_bias=gb[:1], act=L.ACT_SILU)
    small_geglu = ops.gemm(a_tab, wg, bias=bg, act=L.ACT_GEGLU)
    tol_check(small_silu, O.gemm_ref64(t["a"], t["w"], bias=t["bias"], group_bias=t["gb"][:1], act="silu"), dtype, 1.0)
    tol_check(small_geglu, O.gemm_ref64(t["a"], wg.cpu(), bias=bg.cpu(), act="geglu"), dtype, 2.0)
    ref_bias, ref_res = t["ref_bias"].to(dtype).to(dev), t["ref_residual"].to(dtype).to(dev)
    wide = Wide(M, ld, dtype, dev)
    rpg = M // 3
    for variant in O.SETTINGS:
        for form in ("bias", "residual", "gb_silu", "geglu"):
            what = f"C {extent} (M {M}, ldc {ld}) / {form} {DID(dtype)} {VID(variant)}"
            out = wide.arm(NG // 2 if form == "geglu" else N)
            with forced(variant):
                if form == "bias":
                    ops.gemm(a, w, bias=bias, out=out)
                elif form == "residual":
                    ops.gemm(a, w, bias=bias, residual=res, out_scale=2.0, out=out)
                elif form == "gb_silu":
                    ops.gemm(a, w, bias=bias, group_bias=gb, groups=3, act=L.ACT_SILU, out=out)
                else:
                    ops.gemm(a, wg, bias=bg, act=L.ACT_GEGLU, out=out)
            wide.assert_guards(what)
            if form == "bias":
                assert_periodic(out, ref_bias, what)
                assert_rows_match_cpu(out, t["ref_bias"], rows, what)
            elif form == "residual":
                assert_periodic(out, ref_res, what)
                assert_rows_match_cpu(out, t["ref_residual"], rows, what)
            elif form == "geglu":
                assert torch.equal(bits(out[:P]), bits(small_geglu)), f"{what}: the first {P} rows are not the bits of the {P}-row call"
                assert_periodic(out, small_geglu, what)
            else:
                # group 0's rows are the P-row call's; groups 1 and 2 (other per-sample bias) must be periodic in themselves, and their first period
                # is held to the same call with that group's bias
                assert torch.equal(bits(out[:P]), bits(small_silu)), f"{what}: the first {P} rows are not the bits of the {P}-row call"
                for g in range(3):
                    o = out[g * rpg:(g + 1) * rpg]
                    shift = (g * rpg) % P
                    tab_g = ops.gemm(a_tab, w, bias=bias, group_bias=gb[g:g + 1], act=L.ACT_SILU).roll(-shift, 0) if g else small_silu
                    assert_periodic(o, tab_g.contiguous(), f"{what}, group {g}")
    del wide, out


# ------------------------------------------------------------------------------------------------ omg_gemm: residual, A, W
@gpu
@both_dtypes
@pytest.mark.parametrize("extent", EXTENTS)
def test_gemm_residual_at_the_offset_limit(dev, release, extent, dtype):
    """The residual behind a wide ldr: staged through LDS (the 256x256 four-wave tile, 25 and the heuristic) and by register loads (the rest)."""
    t = tables()
    M, ld = rows_ld(extent)
    a_tab, w, bias, r_tab = on_dev(dtype, dev, "a", "w", "bias", "res")
    a = periodic(a_tab, M)
    buf, res = wide_input(r_tab, M, ld, fill=CANARY)
    assert res.stride(0) == ld
    ref = t["ref_residual"].to(dtype).to(dev)
    out = torch.empty(M, N, dtype=dtype, device=dev)
    for variant in O.SETTINGS:
        what = f"residual {extent} (M {M}, ldr {ld}) {DID(dtype)} {VID(variant)}"
        out.fill_(CANARY)
        with forced(variant):
            ops.gemm(a, w, bias=bias, residual=res, out_scale=2.0, out=out)
        assert_periodic(out, ref, what)
        assert_rows_match_cpu(out, t["ref_residual"], sample_rows(M, ld), what)
    del buf, res


@gpu
@both_dtypes
@pytest.mark.parametrize("extent", EXTENTS)
def test_gemm_a_operand_at_the_offset_limit(dev, release, extent, dtype):
    t = tables()
    M, ld = rows_ld(extent)
    a_tab, w, bias = on_dev(dtype, dev, "a", "w", "bias")
    buf, a = wide_input(a_tab, M, ld)
    assert a.stride(0) == ld
    ref = t["ref_bias"].to(dtype).to(dev)
    out = torch.empty(M, N, dtype=dtype, device=dev)
    for variant in O.SETTINGS:
        what = f"A {extent} (M {M}, lda {ld}) {DID(dtype)} {VID(variant)}"
        out.fill_(CANARY)
        with forced(variant):
            ops.gemm(a, w, bias=bias, out=out)
        assert_periodic(out, ref, what)
        assert_rows_match_cpu(out, t["ref_bias"], sample_rows(M, ld), what)
    del buf, a


@gpu
@both_dtypes
@pytest.mark.parametrize("extent", EXTENTS)
def test_gemm_w_operand_at_the_offset_limit(dev, release, extent, dtype):
    """N = 64 weight rows behind a stride of (extent / 64) bytes; M = P rows, so the output is the reference table itself."""
    t = tables()
    lim = limit()
    n = 64
    target = {"under": lim - 1, "window": (lim + OLD_GATE) // 2, "2^31": 2 ** 31 + n * 2 * 64, "2^32": 2 ** 32 + n * 2 * 64}[extent]
    ldw = target // (n * 2) // 8 * 8
    if extent == "under":
        assert n * ldw * 2 < lim <= n * (ldw + 8) * 2
    elif extent == "window":
        assert lim <= n * ldw * 2 < OLD_GATE
    else:
        assert n * ldw * 2 >= 2 ** int(extent[2:])
    a, w_tab, bias = on_dev(dtype, dev, "a", "w", "bias")
    buf = torch.empty(n * ldw, dtype=dtype, device=dev)
    rows = buf.view(n, ldw)
    rows[:, :COL + K + 8].fill_(FILLER)
    w = rows[:, COL:COL + K]
    w.copy_(w_tab[:n])
    assert w.stride(0) == ldw
    ref64 = t["ref_bias"][:, :n]
    for variant in O.SETTINGS:
        what = f"W {extent} (ldw {ldw}) {DID(dtype)} {VID(variant)}"
        out = torch.full((P, n), CANARY, dtype=dtype, device=dev)
        with forced(variant):
            ops.gemm(a, w, bias=bias[:n], out=out)
        got = out.double().cpu()
        assert torch.equal(got, ref64), f"{what}: {int((got != ref64).sum())} outputs differ from the float64 reference"
    del buf, rows, w


@gpu
@both_dtypes
def test_lora_segment_and_weight_slots_beyond_2_gib(dev, release, dtype):
    """A beyond 2^31 bytes with per-sample weight slots (one skipped group) on the down-projection and the K2 = 8 segment on the main GEMM:
    the launches the large tiles never take."""
    t = tables()
    M, ld = rows_ld("2^31")
    rpg = M // 3
    g = O._gen("gemm limits lora")
    down64 = O.tern(g, 2, 8, K, density=O.density(K, 1.5))
    up64 = O.tern(g, 2, N, 8, density=0.75)
    adapter = [1, -1, 0]
    a_tab, w, bias = on_dev(dtype, dev, "a", "w", "bias")
    buf, a = wide_input(a_tab, M, ld)
    down_w, up_w = down64.to(dtype).to(dev), up64.to(dtype).to(dev)
    ad = torch.tensor(adapter, dtype=torch.int32, device=dev)
    for variant in (0, 1, 25):
        what = f"LoRA K2 = 8, A 2^31 (M {M}, lda {ld}) {DID(dtype)} {VID(variant)}"
        down = torch.zeros(M, 8, dtype=dtype, device=dev)
        out = torch.full((M, N), CANARY, dtype=dtype, device=dev)
        with forced(variant):
            ops.gemm(a, down_w, out=down, groups=3, w_group_adapter=ad)
            ops.gemm(a, w, bias=bias, lora=ops.LoraSpec(down, up_w, ad), groups=3, out=out)
        for gi, slot in enumerate(adapter):
            shift = (gi * rpg) % P
            d64 = t["a"] @ down64[slot].T if slot >= 0 else torch.zeros(P, 8, dtype=torch.float64)
            o64 = t["ref_bias"] + (d64 @ up64[slot].T if slot >= 0 else 0.0)
            assert float(o64.abs().max()) <= 256
            assert_periodic(down[gi * rpg:(gi + 1) * rpg], d64.roll(-shift, 0).to(dtype).to(dev), what + f", down-projection of group {gi}")
            assert_periodic(out[gi * rpg:(gi + 1) * rpg], o64.roll(-shift, 0).to(dtype).to(dev), what + f", group {gi}")
    del buf, a


# ------------------------------------------------------------------------------------------------ omg_conv2d
H = W = 64                       # one image: 4096 pixels; C1 = 64 channels -> 512 KiB, about 2^12 images per 2 GiB


def images_for(extent, bytes_per_image):
    lim = limit()
    if extent == "under":
        B = (lim - 1) // bytes_per_image
        assert B * bytes_per_image < lim <= (B + 1) * bytes_per_image
    elif extent == "window":
        B = -(-((lim + OLD_GATE) // 2) // bytes_per_image)
        assert lim <= B * bytes_per_image < OLD_GATE
    else:
        B = -(-2 ** 31 // bytes_per_image) + 2
    return B


@functools.lru_cache(maxsize=None)
def conv_image(c1, c2, cout, ksize, taps=None):
    g = O._gen("conv limits", c1, c2, cout, ksize)
    Kc = (taps or ksize * ksize) * (c1 + c2)
    return dict(x1=O.tern(g, 1, H, W, c1), x2=O.tern(g, 1, H, W, c2) if c2 else None, w=O.tern(g, cout, Kc, density=O.density(Kc)),
                bias=O.ints(g, cout))


def assert_images_equal_first(y, ref64, what):
    """All images of ``y`` are copies of one: image 0 against the float64 reference, every other against image 0 on the device."""
    got = y[0].double().cpu()
    assert torch.equal(got, ref64), f"{what}: image 0 differs from the float64 reference at {int((got != ref64).sum())} outputs"
    same = (bits(y[1:]) == bits(y[:1])).flatten(1).all(dim=1)
    if not bool(same.all()):
        bad = (~same).nonzero().flatten() + 1
        pytest.fail(f"{what}: {bad.numel()} of {y.shape[0]} images differ from image 0, images {int(bad[0])}..{int(bad[-1])}")


@gpu
@both_dtypes
@pytest.mark.parametrize("extent", ["under", "window", "2^31"])
def test_conv_x1_at_the_offset_limit(dev, release, extent, dtype):
    """X1 of C1 = 64 channels and about 2^24 pixels, Cout = 8: 3x3 at stride 1, stride 2 and on the 2x-upsampled input."""
    d = conv_image(64, 0, 8, 3)
    B = images_for(extent, H * W * 64 * 2)
    x = d["x1"].to(dtype).to(dev).expand(B, H, W, 64).contiguous()
    w, bias = d["w"].to(dtype).to(dev), d["bias"].to(dtype).to(dev)
    for geo in (dict(stride=1), dict(stride=2), dict(upsample=True)):
        ref = O.conv2d_ref64(d["x1"], d["w"], 3, bias=d["bias"], **geo)[0]
        assert float(ref.abs().max()) <= 256
        for variant in O.SETTINGS:
            with forced(variant):
                y = ops.conv2d(x, w, 3, bias=bias, **geo)
            assert_images_equal_first(y, ref, f"conv X1 {extent} (B {B}) {geo} {DID(dtype)} {VID(variant)}")
            del y
    del x


@gpu
@both_dtypes
def test_conv_x2_beyond_2_gib(dev, release, dtype):
    d = conv_image(64, 64, 8, 3)
    B = images_for("2^31", H * W * 64 * 2)
    x1 = d["x1"].to(dtype).to(dev).expand(B, H, W, 64).contiguous()
    x2 = d["x2"].to(dtype).to(dev).expand(B, H, W, 64).contiguous()
    w, bias = d["w"].to(dtype).to(dev), d["bias"].to(dtype).to(dev)
    ref = O.conv2d_ref64(d["x1"], d["w"], 3, x2=d["x2"], bias=d["bias"])[0]
    assert float(ref.abs().max()) <= 256
    for variant in O.SETTINGS:
        with forced(variant):
            y = ops.conv2d(x1, w, 3, x2=x2, bias=bias)
        assert_images_equal_first(y, ref, f"conv X2 2^31 (B {B}) {DID(dtype)} {VID(variant)}")
        del y
    del x1, x2


@gpu
@both_dtypes
@pytest.mark.parametrize("extent", ["under", "window", "2^31"])
def test_conv_y_at_the_offset_limit(dev, release, extent, dtype):
    """Y of a 1x1 convolution with Cout = 64 on the 2x-upsampled input: four times X1's extent, so Y alone is at the edge."""
    d = conv_image(64, 0, 64, 1)
    B = images_for(extent, 4 * H * W * 64 * 2)
    x = d["x1"].to(dtype).to(dev).expand(B, H, W, 64).contiguous()
    w, bias = d["w"].to(dtype).to(dev), d["bias"].to(dtype).to(dev)
    ref = O.conv2d_ref64(d["x1"], d["w"], 1, upsample=True, bias=d["bias"])[0]
    n = B * 4 * H * W * 64
    flat = torch.empty(n + 2 * W * 64, dtype=dtype, device=dev)
    y = flat[:n].view(B, 2 * H, 2 * W, 64)
    for variant in O.SETTINGS:
        what = f"conv Y {extent} (B {B}) {DID(dtype)} {VID(variant)}"
        flat.fill_(CANARY)
        with forced(variant):
            ops.conv2d(x, w, 1, upsample=True, bias=bias, out=y)
        assert bool((flat[n:] == CANARY).all()), f"{what}: wrote behind the output"
        assert_images_equal_first(y, ref, what)
    del flat, y, x


@gpu
@both_dtypes
def test_conv_phase_form_y_beyond_2_gib(dev, release, dtype):
    """upsample == 2: the four phase launches scatter their rows over an output beyond 2^31 bytes (gemm_phase_kernel)."""
    g = O._gen("conv limits phase")
    x64 = O.tern(g, 1, H, W, 64)
    w_oihw = O.tern(g, 64, 64, 3, 3, density=0.2)          # sums of up to four of them stay small integers
    bias64 = O.ints(g, 64)
    B = images_for("2^31", 4 * H * W * 64 * 2)
    x = x64.to(dtype).to(dev).expand(B, H, W, 64).contiguous()
    wp = ops.pack_conv_weight_phase(w_oihw.to(dtype)).to(dev)
    ref = O.conv2d_ref64(x64, ops.pack_conv_weight(w_oihw), 3, upsample=True, bias=bias64)[0]
    assert float(ref.abs().max()) <= 256
    n = B * 4 * H * W * 64
    flat = torch.empty(n + 2 * W * 64, dtype=dtype, device=dev)
    y = flat[:n].view(B, 2 * H, 2 * W, 64)
    for variant in (0, 1, 28):
        what = f"conv phase Y 2^31 (B {B}) {DID(dtype)} {VID(variant)}"
        flat.fill_(CANARY)
        with forced(variant):
            ops.conv2d(x, wp, 3, upsample=2, bias=bias64.to(dtype).to(dev), out=y)
        assert bool((flat[n:] == CANARY).all()), f"{what}: wrote behind the output"
        assert_images_equal_first(y, ref, what)
    del flat, y, x


@gpu
@both_dtypes
@pytest.mark.parametrize("big", ["x1", "y"])
def test_conv_slots_with_segment_beyond_2_gib(dev, release, big, dtype):
    """omg_conv2d_slots in segment mode (a weight slot per sample, slot -1 skipped, K2 = 8 added for the others) with X1, or Y, beyond 2^31
    bytes: the CSEG form of the 128x128 kernel."""
    if big == "x1":
        cout, ksize, geo, per_image = 8, 3, dict(), H * W * 64 * 2
    else:
        cout, ksize, geo, per_image = 64, 1, dict(upsample=True), 4 * H * W * 64 * 2
    B = images_for("2^31", per_image)
    g = O._gen("conv limits slots", big)
    Kc = ksize * ksize * 64
    x64 = O.tern(g, 1, H, W, 64)
    w64 = O.tern(g, 2, cout, Kc, density=O.density(Kc))
    bias64 = O.ints(g, cout)
    Ho, Wo = (2 * H, 2 * W) if big == "y" else (H, W)
    a2_64 = O.tern(g, 1, Ho, Wo, 8)
    w2_64 = O.tern(g, 2, cout, 8)
    # what an image holds afterwards, by slot: 0, 1, and -1 (index 2): skipped, the canary stays
    refs = []
    for s in range(2):
        r = O.conv2d_ref64(x64, w64[s], ksize, bias=bias64, **geo)[0] + a2_64[0] @ w2_64[s].T
        assert float(r.abs().max()) <= 256
        refs.append(r)
    refs.append(torch.full_like(refs[0], CANARY))
    refs_dev = torch.stack(refs).to(dtype).to(dev)
    slot = torch.tensor([0, 1, -1], dtype=torch.int32).repeat(-(-B // 3))[:B]
    kind = (slot.long() % 3).to(dev)                         # -1 -> 2
    x = x64.to(dtype).to(dev).expand(B, H, W, 64).contiguous()
    a2 = a2_64.to(dtype).to(dev).expand(B, Ho, Wo, 8).contiguous()
    w, w2, bias, ad = w64.to(dtype).to(dev), w2_64.to(dtype).to(dev), bias64.to(dtype).to(dev), slot.to(dev)
    y = torch.full((B, Ho, Wo, cout), CANARY, dtype=dtype, device=dev)
    ops.conv2d(x, w, ksize, bias=bias, w_group_adapter=ad, lora=ops.LoraSpec(a2, w2, ad), out=y, **geo)
    first = y[:3].double().cpu()
    assert torch.equal(first, torch.stack(refs)), f"conv slots {big} {DID(dtype)}: images 0..2 differ from the float64 reference"
    ok = torch.ones(B, dtype=torch.bool, device=dev)
    for k in range(3):                                       # by slot, so that no second copy of the output is built
        idx = (kind == k).nonzero().flatten()
        for part in idx.split(256):
            ok[part] = (bits(y[part]) == bits(refs_dev[k])).flatten(1).all(dim=1)
    bad = (~ok).nonzero().flatten()
    assert bad.numel() == 0, f"conv slots {big} 2^31 (B {B}) {DID(dtype)}: {bad.numel()} images wrong, images {int(bad[0])}..{int(bad[-1])}"
    del x, a2, y


# ------------------------------------------------------------------------------------------------ MX-fp8: refused, not dropped
def mx8_gemm_case(dev, dtype, extent):
    """omg_gemm_mx8 with C behind a wide ldc; operands -1 / 0 / 1 (exact in e4m3 under any power-of-two scale), K = 128."""
    g = O._gen("mx8 limits")
    a64, w64 = O.tern(g, P, 128), O.tern(g, 64, 128, density=O.density(128))
    ref64 = a64 @ w64.T
    assert float(ref64.abs().max()) <= 256
    M, ld = rows_ld(extent, row_mult=1)
    ta = ops.quant_mx8(periodic(a64.to(dtype).to(dev), M))
    tw = ops.quant_mx8(w64.to(dtype).to(dev))
    wide = Wide(M, ld, dtype, dev)
    return M, ld, ta, tw, wide, ref64


@gpu
@both_dtypes
def test_gemm_mx8_output_just_under_the_limit(dev, release, dtype):
    M, ld, ta, tw, wide, ref64 = mx8_gemm_case(dev, dtype, "under")
    out = wide.arm(64)
    ops.gemm_mx8(ta, tw, out=out)
    what = f"mx8 C under (M {M}, ldc {ld}) {DID(dtype)}"
    wide.assert_guards(what)
    assert_periodic(out, ref64.to(dtype).to(dev), what)
    assert_rows_match_cpu(out, ref64, sample_rows(M, ld), what)
    del wide, out


@gpu
@both_dtypes
def test_gemm_mx8_output_in_the_window_is_refused(dev, release, dtype):
    """No 64-bit kernel stands behind the MX-fp8 entries: an output the descriptors cannot cover is OMG_EINVAL and nothing is written."""
    M, ld, ta, tw, wide, _ = mx8_gemm_case(dev, dtype, "window")
    out = wide.arm(64)
    with pytest.raises(L.OmgHipError, match=r"rc=-1"):
        ops.gemm_mx8(ta, tw, out=out)
    torch.cuda.synchronize()
    c = torch.tensor(CANARY, dtype=dtype, device=dev)
    assert bool((wide.rows[:, :COL + 64 + 8] == c).all()), "a refused call wrote to its output"
    del wide, out


def mx8_conv_case(dev, dtype, extent):
    """omg_conv2d_mx8 with Cin = 128, Cout = 128: Y is twice X's extent, so Y alone is at the edge.  All images are copies of one."""
    g = O._gen("mx8 conv limits")
    cin = cout = 128
    x64 = O.tern(g, 1, H, W, cin)
    w64 = O.tern(g, cout, 9 * cin, density=O.density(9 * cin))
    ref64 = O.conv2d_ref64(x64, w64, 3)[0]
    assert float(ref64.abs().max()) <= 256
    B = images_for(extent, H * W * cout * 2)
    tx = ops.quant_mx8(x64.view(H * W, cin).to(dtype).to(dev))
    xq = tx.q.view(1, H, W, cin).expand(B, H, W, cin).contiguous()
    xs = tx.scales[:, :H * W].repeat(1, B).contiguous()
    tw = ops.quant_mx8(w64.to(dtype).to(dev))
    n = B * H * W * cout
    flat = torch.full((n + W * cout,), CANARY, dtype=dtype, device=dev)
    a = L.Conv2dMx8Args()
    a.dtype = ops._DT[dtype]
    a.B, a.H, a.W, a.Cin, a.Cout = B, H, W, cin, cout
    a.X, a.x_scale, a.Wq, a.w_scale = xq.data_ptr(), xs.data_ptr(), tw.q.data_ptr(), tw.scales.data_ptr()
    a.sw_ld, a.act, a.out_scale, a.Y = tw.scales.stride(0), L.ACT_NONE, 1.0, flat.data_ptr()
    rc = L.lib().omg_conv2d_mx8(ctypes.byref(a), ops._stream())
    torch.cuda.synchronize()
    del xq, xs
    return rc, flat, flat[:n].view(B, H, W, cout), ref64


@gpu
@both_dtypes
def test_conv_mx8_output_just_under_the_limit(dev, release, dtype):
    rc, flat, y, ref64 = mx8_conv_case(dev, dtype, "under")
    assert rc == 0, L.lib().omg_last_error()
    assert bool((flat[y.numel():] == CANARY).all()), "wrote behind the output"
    assert_images_equal_first(y, ref64, f"mx8 conv Y under (B {y.shape[0]}) {DID(dtype)}")
    del flat, y


@gpu
@both_dtypes
def test_conv_mx8_output_in_the_window_is_refused(dev, release, dtype):
    rc, flat, y, _ = mx8_conv_case(dev, dtype, "window")
    assert rc == -1, f"omg_conv2d_mx8 returned {rc} for an output its descriptors cannot cover"
    assert bool((flat == CANARY).all()), "a refused call wrote to its output"
    del flat, y


# ------------------------------------------------------------------------------------------------ the constant (no GPU)
def test_offset_limit_respects_the_descriptor_clamp_and_the_sentinel():
    """The limit admits no epilogue operand larger than the descriptors' num_records clamp (beyond it stores vanish), and the clamp leaves
    the out-of-range sentinel out of range: EPI_OOB, alone or with any admitted offset added in 32 bits, lies at or beyond num_records."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "omg_amd", "csrc", "gemm_epilogue.h")
    src = open(path).read()
    const = lambda name: int(re.search(r"constexpr\s+(?:int|long)\s+" + name + r"\s*=\s*(0x[0-9a-fA-F]+)L?;", src).group(1), 16)
    clamp, oob = const("EPI_CLAMP"), const("EPI_OOB")
    lim = limit()
    assert 0 < lim <= clamp, "the gate admits an operand its descriptor cannot cover"
    assert clamp <= oob, "the sentinel is a valid offset of a clamped descriptor"
    assert oob + lim <= 2 ** 32 - 1, "sentinel + an admitted offset wraps round into range"
    assert lim < 2 ** 31, "an admitted offset does not fit the kernels' int arithmetic"
    gates = [l for l in open(os.path.join(os.path.dirname(path), "gemm.hip")) if re.search(r"\blim\b", l)]
    assert gates and not any("0x7fff0000" in l for l in gates), "a launch gate of gemm.hip carries its own copy of the limit"
