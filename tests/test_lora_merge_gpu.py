"""omg_lora_merge and omg_lora_rownorm (-m gpu) against the float64 model and the derived bound of tests/_lycoris_oracle.py: every term kind,
ranks that are odd and beyond one MFMA pair, shapes smaller than a tile, with a partial column tile, of many tiles and of nine taps, one to
four mixed terms with and without gains; exact-answer inputs, a canary-framed stack, a row alone, and the equivalences between the kinds."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from omg_amd import _lib as L
from omg_amd import ops
from omg_amd.lora import LoraTerm
from tests import _lycoris_oracle as O

DTYPES = [torch.float16, torch.bfloat16]
# (N, K, taps): less than a tile; partial row and column tiles; many tiles; a 3x3 convolution of 64 channels
SHAPES = [(8, 8, 1), (72, 200, 1), (320, 2048, 1), (64, 576, 9)]
RANKS = [1, 4, 5, 33]
SPLITS = [(1, 1), (4, 8), (8, 1)]


def kron_dense(w1, w2):
    """[a, b] x [c, taps, d] -> [a c, taps b d], tap by tap with torch.kron (column = tap * (b d) + ib * d + id)."""
    return torch.cat([torch.kron(w1, w2[:, t, :]) for t in range(w2.shape[1])], dim=1)


def make_term(kind, N, K, g, dev, r=4, split=(1, 1), taps=1, s=0.8, gain=False, amp=1.0):
    """The term as ops.lora_merge takes it, plus the oracle's delta, absolute-product sum and rank."""
    rn = lambda *shape: torch.randn(*shape, generator=g) * amp
    if kind == "plain":
        f = [rn(N, r) * r ** -0.5, rn(r, K)]
        d, a, rr = f[0].double() @ f[1].double(), f[0].double().abs() @ f[1].double().abs(), r
    elif kind == "hada":
        f = [rn(N, r) * r ** -0.5, rn(r, K), rn(N, r + 1) * (r + 1) ** -0.5, rn(r + 1, K)]          # the two products of different ranks
        f64 = [t.double() for t in f]
        d = (f64[0] @ f64[1]) * (f64[2] @ f64[3])
        a = (f64[0].abs() @ f64[1].abs()) * (f64[2].abs() @ f64[3].abs())
        rr = r + 1
    else:
        a_, b_ = split
        f = [rn(a_, b_), rn(N // a_, taps, K // taps // b_)]
        d = kron_dense(f[0].double(), f[1].double())
        a, rr = d.abs(), 1
    t = {"kind": kind, "f": tuple(x.to(dev).contiguous() for x in f), "s": s}
    gv = None
    if gain:
        gv = (torch.rand(N, generator=g) + 0.5).to(dev)
        t["gain"] = gv
    return t, {"d": d, "a": a, "s": s, "gain": gv, "r": rr}


def base_weight(N, K, g, dtype, dev):
    return (torch.randn(N, K, generator=g) * 0.5).to(dtype).to(dev)


def term_sets(N, K, taps, g, dev):
    """(name, terms, oracle terms): every kind alone at every rank and split, then two, three and four mixed terms with and without gains."""
    cin = K // taps
    splits = [sp for sp in SPLITS if N % sp[0] == 0 and cin % sp[1] == 0]
    assert splits == SPLITS
    out = []
    for r in RANKS:
        for kind in ("plain", "hada"):
            for gain in (False, True):
                t, o = make_term(kind, N, K, g, dev, r=r, gain=gain)
                out.append((f"{kind} r={r} gain={gain}", [t], [o]))
    for sp in splits:
        for gain in (False, True):
            t, o = make_term("kron", N, K, g, dev, split=sp, taps=taps, gain=gain)
            out.append((f"kron {sp} taps={taps} gain={gain}", [t], [o]))
    mixes = [[("plain", 5, False), ("kron", splits[1], True)],
             [("hada", 4, True), ("plain", 33, False), ("kron", splits[2], False)],
             [("plain", 4, True), ("hada", 5, False), ("kron", splits[1], True), ("kron", splits[0], False)],
             [("hada", 1, True), ("hada", 33, True), ("plain", 1, True), ("plain", 5, True)]]
    for mix in mixes:
        ts, os_ = [], []
        for i, (kind, arg, gain) in enumerate(mix):
            kw = dict(split=arg, taps=taps) if kind == "kron" else dict(r=arg)
            t, o = make_term(kind, N, K, g, dev, s=0.8 - 0.15 * i, gain=gain, **kw)
            ts.append(t); os_.append(o)
        out.append((" + ".join(f"{k}{'*' if gn else ''}" for k, _, gn in mix), ts, os_))
    return out


# ------------------------------------------------------------------ both kernels within the bound
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{n}x{k}" for n, k, _ in SHAPES])
def test_merge_and_rownorm_stay_within_the_derived_bound(dev, dtype, shape):
    N, K, taps = shape
    g = torch.Generator().manual_seed(N * 7 + K)
    w = base_weight(N, K, g, dtype, dev)
    worst = 0.0
    for name, terms, oterms in term_sets(N, K, taps, g, dev):
        out = torch.empty_like(w)
        ops.lora_merge(w, terms, out)
        exact, S, r = O.merge_exact(w.cpu(), oterms)
        ok, ratio = O.held(out, exact, S, r)
        worst = max(worst, ratio)
        assert ok, f"merge {name}: largest |error| / bound = {ratio:.3f}"
        if len(terms) == 1:
            o = oterms[0]
            norm = ops.lora_rownorm(w, terms[0]).double().cpu()
            want, nb = O.rownorm_exact(w.cpu(), o["d"], o["a"], o["s"], o["r"])
            assert bool(((norm - want).abs() <= nb).all()), f"rownorm {name}: {((norm - want).abs() / nb).max().item():.3f} bounds"
    print(f"lora_merge {dtype} {N}x{K}: largest |error| / bound = {worst:.3f}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_no_terms_copies_the_base(dev, dtype):
    w = base_weight(72, 200, torch.Generator().manual_seed(1), dtype, dev)
    out = torch.zeros_like(w)
    ops.lora_merge(w, [], out)
    assert torch.equal(out, w)


# ------------------------------------------------------------------ exact answers
@pytest.mark.parametrize("dtype", DTYPES)
def test_small_integers_give_the_rounded_exact_result(dev, dtype):
    """Integer factors of at most 2, ranks up to 32, integer W of at most 8, scalings and gains that are powers of two: every product and every
    sum is an integer (or a quarter of one) far below 2^24, so fp32 holds them all exactly and the only rounding is the store's."""
    g = torch.Generator().manual_seed(4)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).float()
    for N, K, taps in ((8, 8, 1), (72, 200, 1), (64, 576, 9)):
        w = ri(-8, 8, N, K).to(dtype).to(dev)
        cin = K // taps
        up, down = ri(-2, 2, N, 5), ri(-2, 2, 5, K)
        h = [ri(-2, 2, N, 12), ri(-2, 2, 12, K), ri(-1, 1, N, 32), ri(-1, 1, 32, K)]      # ranks that are multiples of four take the 16-byte operand path
        w1, w2 = ri(-2, 2, 4, 8), ri(-2, 2, N // 4, taps, cin // 8)
        gains = [torch.tensor([1.0, 2.0, 0.5, 1.5])[torch.randint(0, 4, (N,), generator=g)] for _ in range(2)]
        terms = [{"kind": "plain", "f": (up.to(dev), down.to(dev)), "s": 2.0, "gain": gains[0].to(dev)},
                 {"kind": "hada", "f": tuple(t.to(dev) for t in h), "s": 0.5},
                 {"kind": "kron", "f": (w1.to(dev), w2.to(dev)), "s": -1.0, "gain": gains[1].to(dev)}]
        out = torch.empty_like(w)
        ops.lora_merge(w, terms, out)
        g0, g1 = gains[0].double()[:, None], gains[1].double()[:, None]
        exact = w.cpu().double() * (1 + (g0 - 1) + (g1 - 1)) + g0 * 2.0 * (up.double() @ down.double()) \
            + 0.5 * (h[0].double() @ h[1].double()) * (h[2].double() @ h[3].double()) - g1 * kron_dense(w1.double(), w2.double())
        assert float(exact.abs().max()) < 2 ** 24
        assert torch.equal(out.cpu(), exact.float().to(dtype)), (N, K)
        n = ops.lora_rownorm(w, terms[0])
        v = w.cpu().double() + 2.0 * (up.double() @ down.double())
        want = v.pow(2).sum(1).sqrt()                                                  # integer squares: the fp32 sum is exact, the root is within an ulp
        assert bool(((n.double().cpu() - want).abs() <= want * 2.0 ** -23).all()), (N, K)


# ------------------------------------------------------------------ nothing but the addressed slot is written
@pytest.mark.parametrize("dtype", DTYPES)
def test_only_the_addressed_slot_of_a_canary_framed_stack_changes(dev, dtype):
    g = torch.Generator().manual_seed(6)
    for N, K in ((8, 8), (72, 200), (33, 136)):
        w = base_weight(N, K, g, dtype, dev)
        frame = 4096
        buf = torch.full((frame + 3 * N * K + frame,), 7.0, dtype=dtype, device=dev)
        stack = buf[frame: frame + 3 * N * K].view(3, N, K)
        terms = [make_term("plain", N, K, g, dev, r=5)[0], make_term("hada", N, K, g, dev, r=4, gain=True)[0], make_term("kron", N, K, g, dev)[0]]
        ops.lora_merge(w, terms, stack[1])
        alone = torch.empty_like(w)
        ops.lora_merge(w, terms, alone)
        assert torch.equal(stack[1], alone) and not bool((alone == 7.0).all())
        assert bool((buf[:frame] == 7.0).all()) and bool((buf[frame + 3 * N * K:] == 7.0).all())
        assert bool((stack[0] == 7.0).all()) and bool((stack[2] == 7.0).all())


# ------------------------------------------------------------------ an element depends on its own row and column only
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_row_alone_is_bitwise_the_row_among_others(dev, dtype):
    g = torch.Generator().manual_seed(8)
    N, K = 72, 200
    w = base_weight(N, K, g, dtype, dev)
    tp = make_term("plain", N, K, g, dev, r=5, gain=True)[0]
    th = make_term("hada", N, K, g, dev, r=33)[0]
    tk = make_term("kron", N, K, g, dev, split=(4, 8), gain=True)[0]
    full = torch.empty_like(w)
    ops.lora_merge(w, [tp, th, tk], full)
    norms = [ops.lora_rownorm(w, t) for t in (tp, th, tk)]
    c = N // 4
    for n in (0, 31, 32, 71):
        row = lambda t, i: t[i:i + 1].contiguous()
        one = [{"kind": "plain", "f": (row(tp["f"][0], n), tp["f"][1]), "s": tp["s"], "gain": row(tp["gain"], n)},
               {"kind": "hada", "f": (row(th["f"][0], n), th["f"][1], row(th["f"][2], n), th["f"][3]), "s": th["s"]},
               {"kind": "kron", "f": (row(tk["f"][0], n // c), row(tk["f"][1], n % c)), "s": tk["s"], "gain": row(tk["gain"], n)}]
        out = torch.empty(1, K, dtype=dtype, device=dev)
        ops.lora_merge(row(w, n), one, out)
        assert torch.equal(out[0], full[n]), n
        for t1, nn in zip(one, norms):
            assert torch.equal(ops.lora_rownorm(row(w, n), t1)[0], nn[n]), (n, t1["kind"])


# ------------------------------------------------------------------ equivalences between the kinds
@pytest.mark.parametrize("dtype", DTYPES)
def test_equivalent_forms_agree_within_the_bound(dev, dtype):
    g = torch.Generator().manual_seed(10)
    N, K, r = 72, 200, 5
    w = base_weight(N, K, g, dtype, dev)
    tp, op_ = make_term("plain", N, K, g, dev, r=r)
    up, down = tp["f"]
    exact, S, _ = O.merge_exact(w.cpu(), [op_])

    # LoKr with a 1x1 w1 and a factored w2 (multiplied out in fp32 when the term is fitted to the layer) is the plain pair
    lokr = LoraTerm("kron", {"lokr_w1": torch.ones(1, 1), "lokr_w2_a": up.cpu(), "lokr_w2_b": down.cpu()})
    kind, f = lokr.kernel_term(N, K, 1, dev)
    assert kind == "kron"
    out = torch.empty_like(w)
    ops.lora_merge(w, [{"kind": kind, "f": f, "s": 0.8}], out)
    assert O.held(out, exact, S, r)[0]

    # LoHa whose second product is all ones is the plain pair
    ones = {"kind": "hada", "f": (up, down, torch.ones(N, 1, device=dev), torch.ones(1, K, device=dev)), "s": 0.8}
    ops.lora_merge(w, [ones], out)
    assert O.held(out, exact, S, r)[0]
    plain = torch.empty_like(w)
    ops.lora_merge(w, [tp], plain)
    assert O.held(plain, exact, S, r)[0]
    assert torch.equal(out, plain)                        # x * 1.0 is exact: the same fmaf chain, the same bits

    # a magnitude equal to the float64 norm is no magnitude: the gain is 1 to the norm kernel's own bound, and the slot is within the
    # bound of the float64 merge under that very gain
    want_n, nb = O.rownorm_exact(w.cpu(), op_["d"], op_["a"], 0.8, r)
    gain = (want_n.float().to(dev) / ops.lora_rownorm(w, tp)).contiguous()
    assert bool(((gain.double().cpu() - 1).abs() <= nb / want_n + 2 * O.U32).all())
    ops.lora_merge(w, [dict(tp, gain=gain)], out)
    e2, S2, _ = O.merge_exact(w.cpu(), [dict(op_, gain=gain)])
    assert O.held(out, e2, S2, r)[0]
    got = out.double().cpu()
    assert bool(((got - exact).abs() <= O.bound(got, exact, S, r, dtype) + (nb / want_n + 2 * O.U32)[:, None] * S).all())


# ------------------------------------------------------------------ refusals, without a launch
def test_bad_arguments_are_refused_and_write_nothing(dev):
    lib = L.lib()
    N, K = 16, 64
    w = torch.ones(N, K, dtype=torch.float16, device=dev)
    out = torch.full((N, K), 7.0, dtype=torch.float16, device=dev)
    up, down = torch.ones(N, 4, device=dev), torch.ones(4, K, device=dev)
    w1, w2 = torch.ones(4, 8, device=dev), torch.ones(4, 1, 8, device=dev)
    norm = torch.full((N,), 7.0, device=dev)

    def args(**kw):
        a = L.LoraMergeArgs()
        a.dtype, a.N, a.K, a.n_terms, a.W, a.out = L.OMG_F16, N, K, 1, w.data_ptr(), out.data_ptr()
        t = a.terms[0]
        t.kind, t.r, t.s, t.f0, t.f1 = L.LORA_PLAIN, 4, 1.0, up.data_ptr(), down.data_ptr()
        for k, v in kw.items():
            setattr(a.terms[0] if k.startswith("t_") else a, k[2:] if k.startswith("t_") else k, v)
        return a

    assert lib.omg_lora_merge(C.byref(args()), None) == 0
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())
    out.fill_(7.0)
    kron = dict(t_kind=L.LORA_KRON, t_a=4, t_b=8, t_c=4, t_d=8, t_taps=1, t_f0=w1.data_ptr(), t_f1=w2.data_ptr())
    assert lib.omg_lora_merge(C.byref(args(**kron)), None) == 0
    torch.cuda.synchronize()
    out.fill_(7.0)
    cases = {"K % 8": args(K=60), "K < 8": args(K=0), "N < 1": args(N=0), "dtype": args(dtype=L.OMG_F32), "null W": args(W=None), "null out": args(out=None),
             "five terms": args(n_terms=5), "negative terms": args(n_terms=-1), "kind": args(t_kind=3), "r < 1": args(t_r=0), "null factor": args(t_f1=None),
             "hada r2": args(t_kind=L.LORA_HADA, t_f2=up.data_ptr(), t_f3=down.data_ptr(), t_r2=0),
             "hada factors": args(t_kind=L.LORA_HADA, t_r2=4), "kron rows": args(**dict(kron, t_c=3)), "kron columns": args(**dict(kron, t_d=4)),
             "kron taps": args(**dict(kron, t_taps=2)), "kron zero": args(**dict(kron, t_b=0)), "misaligned W": args(W=w.data_ptr() + 2)}
    assert lib.omg_lora_merge(None, None) != 0 and lib.omg_last_error()
    for name, a in cases.items():
        assert lib.omg_lora_merge(C.byref(a), None) != 0 and lib.omg_last_error(), name
    good = args().terms[0]
    assert lib.omg_lora_rownorm(L.OMG_F16, N, K, w.data_ptr(), C.byref(good), norm.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert bool((norm == (K * 25.0) ** 0.5).all())
    norm.fill_(7.0)
    for name, rc in {"K % 8": lib.omg_lora_rownorm(L.OMG_F16, N, 60, w.data_ptr(), C.byref(good), norm.data_ptr(), None),
                     "null term": lib.omg_lora_rownorm(L.OMG_F16, N, K, w.data_ptr(), None, norm.data_ptr(), None),
                     "null norm": lib.omg_lora_rownorm(L.OMG_F16, N, K, w.data_ptr(), C.byref(good), None, None),
                     "dtype": lib.omg_lora_rownorm(L.OMG_F32, N, K, w.data_ptr(), C.byref(good), norm.data_ptr(), None),
                     "kron": lib.omg_lora_rownorm(L.OMG_F16, N, K, w.data_ptr(), C.byref(args(**dict(kron, t_c=3)).terms[0]), norm.data_ptr(), None)}.items():
        assert rc != 0 and lib.omg_last_error(), name
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((norm == 7.0).all()), "a refused call wrote to its output"
    # the wrapper's own checks: shapes that would make the kernel read outside a factor, a zero-width stack, five terms
    t = {"kind": "plain", "f": (up, down), "s": 1.0}
    for bad in ({"kind": "plain", "f": (up[:8].contiguous(), down), "s": 1.0}, {"kind": "plain", "f": (up[:, :0].contiguous(), down[:0].contiguous()), "s": 1.0},
                {"kind": "kron", "f": (w1, torch.ones(4, 1, 4, device=dev)), "s": 1.0}, dict(t, gain=torch.ones(N - 1, device=dev)),
                {"kind": "plain", "f": (up.half(), down), "s": 1.0}):
        with pytest.raises(L.OmgHipError):
            ops.lora_merge(w, [bad], out)
    with pytest.raises(L.OmgHipError, match="at most 4"):
        ops.lora_merge(w, [t] * 5, out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
