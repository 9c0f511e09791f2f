"""The classifier head (csrc/skinny.hip, training section) and the two loss kernels beside it (gtl_kernel, cross_entropy_kernel of
csrc/layer.hip) through every entry point of their C ABI, against the float64 restatement of tests/head_reference.py.

Exact family: integer operands, so y, dx, dW and db must equal the reference BIT FOR BIT whatever the split, slice, wave or atomic
order, and the forms of one product agree among themselves.  Rounding family: real operands with |logit| <= 8, within the derived
bound (n + 8) 2^-24 sum |a||b| per element; loss and dlogits under the project's 2e-5 max |ref| gate (the fused loss with the
header's fixed-point term), their error printed as a multiple of an f32 restatement's.  Every output is a view into a larger
sentinel-filled buffer whose guards must stay untouched; OVERWRITTEN outputs start from the sentinel, the atomically accumulated
dx from zero.  tests/test_host_head_reference.py shows on the CPU that these verdicts reject the defects they are meant to reject."""
import math

import numpy as np
import pytest
import torch

import head_abi as abi
import head_reference as hr
from mobgt_amd import _lib, forms, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = hr.SENT
ALPHA = 0.2
PAD = 64                                                # guard elements on either side (keeps the view 16-byte aligned)


class Guarded:
    """A contiguous destination of `shape` inside a sentinel-filled buffer (these entries take no leading dimension: the guards are
    the PAD elements in front of the first row and behind the last)."""

    def __init__(self, shape, init=SENT, dtype=torch.float32):
        self.shape, self.n = shape, math.prod(shape)
        self.big = torch.full((self.n + 2 * PAD,), SENT, dtype=dtype, device=DEV)
        self.view = self.big[PAD:PAD + self.n].view(shape)
        if init != SENT:
            self.view.fill_(init)

    def result(self):
        """The destination on the host (numpy); asserts that nothing outside it was written."""
        big = self.big.cpu()
        assert bool((big[:PAD] == SENT).all()) and bool((big[PAD + self.n:] == SENT).all()), "a guard element was written"
        return big[PAD:PAD + self.n].view(self.shape).numpy()


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.asarray(a, dtype=np.float32).view(np.int32)


def same_bits(a, b):
    return bool(np.array_equal(bits(a), bits(b)))


# ------------------------------------------------------------------------------------------------ the four products, every form
@pytest.mark.parametrize("family", ["exact", "round"])
@pytest.mark.parametrize("shape", hr.PRODUCT_SHAPES, ids=lambda s: "G%d-K%d-V%d" % s)
def test_products(shape, family):
    G, K, V = shape
    i = hr.PRODUCT_SHAPES.index(shape)
    case = hr.build_case(G, K, V, family, bias=i % 3 != 1)
    x, w, b, dy = (dev(case[k]) for k in ("x", "w", "b", "dy"))
    has = hr.forms_for(K)
    out = {}                                            # (form, product) -> Guarded
    out["fwd", "y"] = Guarded((G, V))
    assert abi.fwd(x, w, b, out["fwd", "y"].view, G, K, V) == 0
    if "fwd_mfma" in has:
        out["fwd_mfma", "y"] = Guarded((G, V))
        assert abi.fwd_mfma(x, w, b, out["fwd_mfma", "y"].view, G, K, V) == 0
        out["gtl", "y"], dl, loss = Guarded((G, V)), Guarded((G, V)), Guarded((1,))
        t = torch.zeros(G, dtype=torch.int64, device=DEV)
        assert abi.gtl(x, w, b, t, 0, out["gtl", "y"].view, dl.view, loss.view, G, K, V, ALPHA) == 0
    # legacy backward: all three OVERWRITTEN; then dx = NULL and db = NULL, which must leave dW as it was
    for p, s in (("dx", (G, K)), ("dW", (V, K)), ("db", (V,))):
        out["bwd", p] = Guarded(s)
    assert abi.bwd(dy, x, w, out["bwd", "dx"].view, out["bwd", "dW"].view, out["bwd", "db"].view, G, K, V) == 0
    dw_alone = Guarded((V, K))
    assert abi.bwd(dy, x, w, None, dw_alone.view, None, G, K, V) == 0
    if "dx" in has:
        out["dx", "dx"] = Guarded((G, K), init=0.0)
        assert abi.dx(dy, w, out["dx", "dx"].view, G, K, V) == 0
        out["bwd_both", "dx"], out["bwd_both", "dW"] = Guarded((G, K), init=0.0), Guarded((V, K))
        db = out["bwd_both", "db"] = Guarded((V,))
        with_db = i % 2 == 0                             # (db == NULL: a head without bias)
        assert abi.bwd_both(dy, x, w, out["bwd_both", "dx"].view, out["bwd_both", "dW"].view, db.view if with_db else None, G, K, V) == 0
    torch.cuda.synchronize()
    got = {k: g.result() for k, g in out.items()}
    if "fwd_mfma" in has:
        dl.result(), loss.result()                       # (their guards)
    if "dx" in has and not with_db:
        assert bool((got.pop(("bwd_both", "db")) == SENT).all())
    worst = {}
    for (form, p), a in got.items():
        ok, ratio = hr.product_verdict(case, p, a)
        worst[p] = max(worst.get(p, 0.0), ratio)
        assert ok, (form, p, shape, family, ratio)
    assert same_bits(dw_alone.result(), got["bwd", "dW"])
    if "fwd_mfma" in has:                                # one kernel, with and without the loss: the same logit bits in either family
        assert same_bits(got["fwd_mfma", "y"], got["gtl", "y"])
    if family == "exact":                                # (equal to one reference, hence to each other: said once more by name)
        for p in ("y", "dx", "dW", "db"):
            same = [a for (_, q), a in got.items() if q == p]
            assert all(same_bits(same[0], a) for a in same[1:]), p
    else:
        print("head-ratio products G%d-K%d-V%d " % shape + " ".join(f"{p}={r:.4f}" for p, r in sorted(worst.items())))


# ------------------------------------------------------------------------------------------------ the fused loss and the loss alone
def run_gtl(x, w, b, t, off, G, K, V, store=True):
    z, dl, loss = (Guarded((G, V)) if store else None), Guarded((G, V)), Guarded((1,))
    assert abi.gtl(x, w, b, t, off, z.view if store else None, dl.view, loss.view, G, K, V, ALPHA) == 0
    torch.cuda.synchronize()
    return (z.result() if store else None), dl.result(), loss.result()[0]


@pytest.mark.parametrize("off", [0, -1])
@pytest.mark.parametrize("shape", hr.GTL_SHAPES, ids=lambda s: "G%d-K%d-V%d" % s)
def test_fused_loss_and_loss_alone(shape, off):
    G, K, V = shape
    case = hr.build_case(G, K, V, "round", bias=hr.GTL_SHAPES.index(shape) % 3 != 1)
    x, w, b = (dev(case[k]) for k in ("x", "w", "b"))
    tn = hr.targets_for(G, V, off)
    t = dev(tn)
    z, dl, loss = run_gtl(x, w, b, t, off, G, K, V)
    ok, ratio = hr.product_verdict(case, "y", z)
    assert ok, ("logits", ratio)
    # both losses on the SAME logits (the kernel's own, as stored), against the formulas in float64 on those logits
    ref_loss, ref_dz = hr.gtl(z, tn, off, ALPHA)
    l32, d32 = hr.gtl(z, tn, off, ALPHA, np.float32)
    assert np.isfinite(d32).all() and np.isfinite(ref_dz).all()
    s_dz = float(np.abs(ref_dz).max())
    e32_loss, e32_dz = abs(float(l32) - ref_loss), float(np.abs(d32.astype(np.float64) - ref_dz).max())
    dl2, loss2 = Guarded((G, V)), Guarded((1,))
    assert abi.gradient_tail_loss(dev(z), t, off, dl2.view, loss2.view, G, V, ALPHA) == 0
    torch.cuda.synchronize()
    dl2, loss2 = dl2.result(), loss2.result()[0]
    for name, lo, dz_, fixed in (("fused", loss, dl, hr.gtl_fixed_point(G, V)), ("alone", loss2, dl2, 0.0)):
        ok, e_loss, e_dz = hr.loss_verdict(lo, dz_, ref_loss, ref_dz, fixed)
        r_loss, r_dz = hr.f32_ratio(e_loss, e32_loss, ref_loss), hr.f32_ratio(e_dz, e32_dz, s_dz)
        print(f"head-ratio gtl-{name} G{G}-K{K}-V{V} off={off} loss_err={e_loss / ref_loss:.2e} dz_err={e_dz / s_dz:.2e} "
              f"f32_loss_err={e32_loss / ref_loss:.2e} f32_dz_err={e32_dz / s_dz:.2e} loss/f32={r_loss:.2f} dz/f32={r_dz:.2f}")
        assert ok, (name, e_loss, e_dz, float(ref_loss), s_dz)
        assert r_loss <= 16 and r_dz <= 16, (name, r_loss, r_dz)
    assert abs(float(loss) - float(loss2)) <= hr.GATE * ref_loss + hr.gtl_fixed_point(G, V)
    assert float(np.abs(dl.astype(np.float64) - dl2).max()) <= hr.GATE * s_dz
    # logits == NULL: the same loss and dlogits bits; the same call again: the same loss bits (the fixed-order sum)
    _, dl3, loss3 = run_gtl(x, w, b, t, off, G, K, V, store=False)
    assert same_bits(loss3, loss) and same_bits(dl3, dl)
    for _ in range(2):
        assert same_bits(run_gtl(x, w, b, t, off, G, K, V)[2], loss)


# ------------------------------------------------------------------------------------------------ a diverged step, then a clean one
@pytest.mark.parametrize("V", [200, 257, 32769], ids=lambda v: "V%d" % v)            # 7, 9 and 1024 workgroups
def test_fused_loss_after_a_poisoned_call(V):
    """A call whose loss is not finite by arithmetic alone returns +inf and leaves the nine cells and the flag re-armed: the next
    clean call returns the bits it returned before."""
    G, K, off = 16, 128, -1
    case = hr.build_case(G, K, V, "round")
    x, w, b = (dev(case[k]) for k in ("x", "w", "b"))
    tn = hr.targets_for(G, V, off)
    t = dev(tn)
    _, dl0, loss0 = run_gtl(x, w, b, t, off, G, K, V)
    assert np.isfinite(loss0) and np.isfinite(dl0).all()
    classes = set((tn + off).tolist())
    for c in (3, V // 2 + 1, V - 2):                     # a bias of 100 on a column that is no row's class: p = 1, log(1 - p) = -inf
        assert c not in classes
        b2 = b.clone()
        b2[c] = 100.0
        assert run_gtl(x, w, b2, t, off, G, K, V)[2] == np.inf
        _, dl1, loss1 = run_gtl(x, w, b, t, off, G, K, V)
        assert same_bits(loss1, loss0) and same_bits(dl1, dl0), c
    x2 = x.clone()
    x2[0, 0] = float("nan")                              # a whole row of nan logits: +inf, not nan
    assert run_gtl(x2, w, b, t, off, G, K, V)[2] == np.inf
    b2 = b.clone()
    b2[5] = 100.0
    assert run_gtl(x2, w, b2, t, off, G, K, V)[2] == np.inf
    for _ in range(2):
        _, dl1, loss1 = run_gtl(x, w, b, t, off, G, K, V)
        assert same_bits(loss1, loss0) and same_bits(dl1, dl0)


def run_ce(z, t, ignore, G, V, want_dz=True):
    dz, loss = (Guarded((G, V)) if want_dz else None), Guarded((1,))
    assert abi.cross_entropy(z, t, ignore, dz.view if want_dz else None, loss.view, G, V) == 0
    torch.cuda.synchronize()
    return loss.result()[0], (dz.result() if want_dz else None)


def ce_inputs(G, V):
    rng = np.random.default_rng(G * 100003 + V)
    ignore = 0 if V > 2 else -100
    # logits of a few units, as test_cross_entropy_in_one_launch draws them; with two columns and one live row that makes
    # softmax - one_hot a difference of nearly equal numbers everywhere (|gradient| <= 4e-4 at 2^-24 absolute: the gate, relative to
    # the largest gradient, then measures float32 itself -- the f32 restatement misses it by the same 3e-8), so V <= 2 draws
    # logits half a unit apart and keeps a gradient of the order of 1 / rows
    z = (rng.standard_normal((G, V)) * (3 if V > 2 else 0.5)).astype(np.float32)
    t = rng.integers(1 if ignore == 0 else 0, V, size=G).astype(np.int64)
    if G >= 3:
        t[::3] = ignore
        t[1] = -5                                        # outside [0, V): in the divisor, no term, a zero gradient row
    if G >= 5:
        t[4] = V + 3
    return z, t, ignore


@pytest.mark.parametrize("G", [16, 257])
def test_cross_entropy_after_a_poisoned_call(G):
    V = 1000
    zn, tn, ignore = ce_inputs(G, V)
    z, t = dev(zn), dev(tn)
    loss0, dz0 = run_ce(z, t, ignore, G, V)
    assert np.isfinite(loss0)
    g = 2                                                # a live row
    assert tn[g] != ignore and 0 <= tn[g] < V
    c = (int(tn[g]) + 7) % V
    big, nan, both = z.clone(), z.clone(), z.clone()
    big[g, c] = 1.0e5                                    # -log softmax = 1e5 - z[t] >= 2^16: the header's +inf
    nan[g, c] = float("nan")
    both[g, c], both[g + 5, c] = 1.0e5, float("nan")     # (row g + 5 is live too) nan wins
    assert tn[g + 5] != ignore and 0 <= tn[g + 5] < V
    for poisoned, want in ((big, np.inf), (nan, np.nan), (both, np.nan)):
        got = run_ce(poisoned, t, ignore, G, V)[0]
        assert np.isnan(got) if np.isnan(want) else got == want
        loss1, dz1 = run_ce(z, t, ignore, G, V)
        assert same_bits(loss1, loss0) and same_bits(dz1, dz0)


# ------------------------------------------------------------------------------------------------ cross entropy
@pytest.mark.parametrize("shape", hr.CE_SHAPES, ids=lambda s: "G%d-V%d" % s)
def test_cross_entropy_matrix(shape):
    G, V = shape
    zn, tn, ignore = ce_inputs(G, V)
    z = dev(zn)
    for kind, tt in (("mixed", tn), ("all ignored", np.full(G, ignore, dtype=np.int64))):
        t = dev(tt)
        loss, dz = run_ce(z, t, ignore, G, V)
        ref_loss, ref_dz = hr.cross_entropy(zn, tt, ignore)
        assert same_bits(run_ce(z, t, ignore, G, V, want_dz=False)[0], loss)
        if kind == "all ignored":
            assert np.isnan(loss) and np.isnan(ref_loss) and not dz.any()
            continue
        l32, d32 = hr.cross_entropy(zn, tt, ignore, np.float32)
        e_loss, e_dz = abs(float(loss) - ref_loss), float(np.abs(dz.astype(np.float64) - ref_dz).max())
        s_dz = float(np.abs(ref_dz).max())
        print(f"head-ratio ce G{G}-V{V} loss_err={e_loss:.2e} dz_err={e_dz:.2e} "
              f"loss/f32={hr.f32_ratio(e_loss, abs(float(l32) - ref_loss), abs(ref_loss)):.2f} "
              f"dz/f32={hr.f32_ratio(e_dz, float(np.abs(d32 - ref_dz).max()), s_dz):.2f}")
        assert e_loss <= 2e-6 * abs(ref_loss) + 1e-6, (e_loss, ref_loss)
        assert e_dz <= 2e-6 * s_dz + 1e-9, (e_dz, s_dz)
        for g in np.nonzero((tt != ignore) & ((tt < 0) | (tt >= V)))[0]:
            assert not dz[g].any()


# ------------------------------------------------------------------------------------------------ refusals: status codes only
class Refusal:
    """Small valid operands whose destinations hold the sentinel; every refused call must leave them untouched."""
    G, K, V = 4, 64, 40

    def __init__(self):
        G, K, V = self.G, self.K, self.V
        one = lambda *s: torch.ones(*s, device=DEV)                          # noqa: E731
        self.x, self.w, self.b, self.dy = one(G + 1, K), one(V + 1, K), one(V), one(G, V)
        self.t = torch.zeros(G, dtype=torch.int64, device=DEV)
        self.y, self.dl, self.loss = Guarded((G, V)), Guarded((G, V)), Guarded((1,))
        self.dx, self.dw, self.db = Guarded((G, K)), Guarded((V, K)), Guarded((V,))
        self.z = one(16, 64)                                                  # cross entropy's logits
        self.tz = torch.zeros(4096, dtype=torch.int64, device=DEV)
        self.outs = (self.y, self.dl, self.loss, self.dx, self.dw, self.db)

    def dims(self, **kw):
        return (kw.get("G", self.G), kw.get("K", self.K), kw.get("V", self.V))

    def fwd(self, x=None, w=None, **kw):
        return abi.fwd(self.x if x is None else x, self.w if w is None else w, self.b, self.y.view, *self.dims(**kw))

    def bwd(self, dw=True, **kw):
        return abi.bwd(self.dy, self.x, self.w, self.dx.view, self.dw.view if dw else None, self.db.view, *self.dims(**kw))

    def dxo(self, w=None, dx=True, **kw):
        return abi.dx(self.dy, self.w if w is None else w, self.dx.view if dx else None, *self.dims(**kw))

    def both(self, w=None, dx=True, dw=True, **kw):
        return abi.bwd_both(self.dy, self.x, self.w if w is None else w, self.dx.view if dx else None, self.dw.view if dw else None,
                            self.db.view, *self.dims(**kw))

    def mfma(self, x=None, w=None, y=True, **kw):
        return abi.fwd_mfma(self.x if x is None else x, self.w if w is None else w, self.b, self.y.view if y else None, *self.dims(**kw))

    def gtl(self, x=None, w=None, t=True, dl=True, loss=True, **kw):
        return abi.gtl(self.x if x is None else x, self.w if w is None else w, self.b, self.t if t else None, 0, self.y.view,
                       self.dl.view if dl else None, self.loss.view if loss else None, *self.dims(**kw), ALPHA)

    def loss_alone(self, G=4, V=40):
        return abi.gradient_tail_loss(self.dy, self.t, 0, self.dl.view, self.loss.view, G, V, ALPHA)

    def ce(self, G=4, V=40, loss=True):
        return abi.cross_entropy(self.z, self.tz, 0, self.dl.view, self.loss.view if loss else None, G, V)


REFUSALS = {}
for _e in ("fwd", "bwd", "dxo", "both", "mfma", "gtl"):
    for _k, _v in (("G", 0), ("G", 17), ("K", 0), ("K", 6), ("K", 516), ("V", 0)):
        REFUSALS[f"{_e}-{_k}{_v}"] = (lambda c, e=_e, k=_k, v=_v: getattr(c, e)(**{k: v}), abi.EBADDIM)
REFUSALS.update({
    "fwd-x-off-4-bytes": (lambda c: c.fwd(x=c.x.data_ptr() + 4), abi.EALIGN),
    "fwd-w-off-4-bytes": (lambda c: c.fwd(w=c.w.data_ptr() + 4), abi.EALIGN),
    "bwd-db-without-dw": (lambda c: c.bwd(dw=False), abi.EBADDIM),
    "dx-K40": (lambda c: c.dxo(K=40), abi.EBADDIM), "both-K40": (lambda c: c.both(K=40), abi.EBADDIM),
    "dx-w-off-4-bytes": (lambda c: c.dxo(w=c.w.data_ptr() + 4), abi.EALIGN),
    "both-w-off-4-bytes": (lambda c: c.both(w=c.w.data_ptr() + 4), abi.EALIGN),
    "dx-null-dx": (lambda c: c.dxo(dx=False), abi.EBADDIM), "both-null-dx": (lambda c: c.both(dx=False), abi.EBADDIM),
    "both-null-dw": (lambda c: c.both(dw=False), abi.EBADDIM),
    "mfma-K512": (lambda c: c.mfma(K=512), abi.EBADDIM), "mfma-K96": (lambda c: c.mfma(K=96), abi.EBADDIM),
    "gtl-K512": (lambda c: c.gtl(K=512), abi.EBADDIM), "gtl-K96": (lambda c: c.gtl(K=96), abi.EBADDIM),
    "mfma-null-y": (lambda c: c.mfma(y=False), abi.EBADDIM), "gtl-null-dlogits": (lambda c: c.gtl(dl=False), abi.EBADDIM),
    "gtl-null-loss": (lambda c: c.gtl(loss=False), abi.EBADDIM), "gtl-null-targets": (lambda c: c.gtl(t=False), abi.EBADDIM),
    "mfma-x-off-4-bytes": (lambda c: c.mfma(x=c.x.data_ptr() + 4), abi.EALIGN),
    "mfma-w-off-4-bytes": (lambda c: c.mfma(w=c.w.data_ptr() + 4), abi.EALIGN),
    "gtl-x-off-4-bytes": (lambda c: c.gtl(x=c.x.data_ptr() + 4), abi.EALIGN),
    "gtl-w-off-4-bytes": (lambda c: c.gtl(w=c.w.data_ptr() + 4), abi.EALIGN),
    "loss-G0": (lambda c: c.loss_alone(G=0), abi.EBADDIM), "loss-V0": (lambda c: c.loss_alone(V=0), abi.EBADDIM),
    "ce-G0": (lambda c: c.ce(G=0), abi.EBADDIM), "ce-G4096": (lambda c: c.ce(G=4096), abi.EBADDIM),
    "ce-V0": (lambda c: c.ce(V=0), abi.EBADDIM), "ce-V10241": (lambda c: c.ce(V=10241), abi.EBADDIM),
    "ce-null-loss": (lambda c: c.ce(loss=False), abi.EBADDIM),
})


@pytest.fixture(scope="module")
def refusal():
    return Refusal()


@pytest.mark.parametrize("name", list(REFUSALS), ids=list(REFUSALS))
def test_refusal(refusal, name):
    """Host-side checks: the status code comes back, no kernel runs, no destination changes."""
    fn, code = REFUSALS[name]
    assert fn(refusal) == code
    torch.cuda.synchronize()
    for o in refusal.outs:
        assert bool((o.result() == SENT).all())


# ------------------------------------------------------------------------------------------------ the ops dispatch around them
def recorded(fn):
    """fn()'s result and the skinny entries it asked of the kernel library, in order (the spy tests/test_gpu_heads.py records a
    step's calls with: `_lib.call` goes through `_lib.lib`)."""
    real, seen = _lib.lib, []

    class _Spy:
        def __getattr__(self, entry):
            seen.append(entry)
            return getattr(real(), entry)

    _lib.lib = lambda: _Spy()
    try:
        out = fn()
    finally:
        _lib.lib = real
    return out, [e.replace("mobgt_skinny_linear_", "") for e in seen if e.startswith("mobgt_skinny_linear")]


def expected_entries(K, all_hip, fused, need_x, need_wb):
    if fused:
        fwd, all_hip = ["gtl"], False                    # (the fused forward has no legacy form)
    else:
        fwd = ["fwd"] if all_hip else (["fwd_mfma"] if K % 64 == 0 and K <= 448 else [])
    dx_mfma = need_x and not all_hip and K % 16 == 0
    return fwd + (["bwd_both"] if dx_mfma and need_wb else ["dx", "bwd"] if dx_mfma else ["bwd"])


WANTS = {"x": (True, False, False), "w": (False, True, False), "x+w+b": (True, True, True), "x+b": (True, False, True)}


@pytest.mark.parametrize("all_hip", [False, True], ids=["default", "skinny_all"])
@pytest.mark.parametrize("K", [64, 80, 100, 512])
def test_ops_skinny_linear_dispatch(K, all_hip):
    G, V = 5, 1024
    for bias in (True, False):
        case = hr.build_case(G, K, V, "round", bias=bias, seed=int(all_hip))
        for want, (nx, nw, nb) in WANTS.items():
            nb = nb and bias
            x, w, b = (dev(case[k]) for k in ("x", "w", "b"))
            x.requires_grad_(nx), w.requires_grad_(nw)
            if bias:
                b.requires_grad_(nb)
            assert ops.skinny_linear_ok(x, w)

            def step():
                with forms.using(skinny_all=all_hip):
                    y = ops.skinny_linear(x, w, b)
                    y.backward(dev(case["dy"]))
                return y
            y, seen = recorded(step)
            torch.cuda.synchronize()
            assert seen == expected_entries(K, all_hip, False, nx, nw or nb), (want, bias, seen)
            got = dict(y=y.detach(), dx=x.grad, dW=w.grad, db=b.grad if bias else None)
            for p, wanted in (("y", True), ("dx", nx), ("dW", nw), ("db", nb)):
                if not wanted:
                    assert got[p] is None, (p, want, bias)
                    continue
                ok, ratio = hr.product_verdict(case, p, got[p].cpu().numpy())
                assert ok, (p, want, bias, ratio)


@pytest.mark.parametrize("all_hip", [False, True], ids=["default", "skinny_all"])
@pytest.mark.parametrize("K", [64, 80, 100, 512])
def test_ops_skinny_linear_gtl_dispatch(K, all_hip):
    """ops.skinny_linear_gtl against float64 autograd of F.linear + GradientTailLoss, its backward fed with the unit gradient, with
    autograd's own ones and with the 3 of `3 * loss`; a K the fused kernel does not take is an error, not another path."""
    from mobgt_amd.model_fqandtoyo import GradientTailLoss
    G, V, off = 5, 1024, -1
    for bias in (True, False):
        case = hr.build_case(G, K, V, "round", bias=bias, seed=2 + int(all_hip))
        tn = hr.targets_for(G, V, off)
        xr, wr = (torch.tensor(case[k], dtype=torch.float64, requires_grad=True) for k in ("x", "w"))
        br = torch.tensor(case["b"], dtype=torch.float64, requires_grad=True) if bias else None
        # GradientTailLoss scatters its one-hot, which a class outside [0, V) cannot enter: the rows whose class is a column go
        # through it, the others are rows of negatives (the second term of its formula alone); each mean is over its own rows
        zr = torch.nn.functional.linear(xr, wr, br)
        inside = [g for g in range(G) if 0 <= tn[g] + off < V]
        outside = [g for g in range(G) if g not in inside]
        p_out = torch.sigmoid(zr[outside])
        ref = GradientTailLoss(zr[inside], torch.tensor(tn + off)[inside], alpha=ALPHA) * len(inside) / G \
            - (p_out * torch.log(1 - p_out)).sum() / (G * V)
        assert abs(float(ref.detach()) - float(hr.gtl(zr.detach().numpy(), tn, off, ALPHA)[0])) <= 1e-12
        ref.backward()
        ref = ref.detach()
        for want, (nx, nw, nb) in WANTS.items():
            nb = nb and bias
            for scale in ("unit", "ones", 3.0):
                x, w, b = (dev(case[k]) for k in ("x", "w", "b"))
                x.requires_grad_(nx), w.requires_grad_(nw)
                if bias:
                    b.requires_grad_(nb)
                if not ops.skinny_linear_gtl_ok(x, w):
                    assert K != 64
                    with pytest.raises(_lib.MobgtError):
                        ops.skinny_linear_gtl(x, w, b, dev(tn), ALPHA, target_offset=off)
                    continue
                assert K == 64

                def step():
                    with forms.using(skinny_all=all_hip):
                        loss = ops.skinny_linear_gtl(x, w, b, dev(tn), ALPHA, target_offset=off)
                        if scale == "unit":
                            loss.backward(gradient=ops.unit_grad(loss.device))
                        elif scale == "ones":
                            loss.backward()
                        else:
                            (scale * loss).backward()
                    return loss.detach()
                loss, seen = recorded(step)
                torch.cuda.synchronize()
                assert seen == expected_entries(K, all_hip, True, nx, nw or nb), (want, bias, scale, seen)
                f = scale if isinstance(scale, float) else 1.0
                assert abs(float(loss) - float(ref)) <= hr.GATE * float(ref) + hr.gtl_fixed_point(G, V)
                for name, got, r, wanted in (("dx", x.grad, xr.grad, nx), ("dW", w.grad, wr.grad, nw),
                                             ("db", b.grad if bias else None, br.grad if bias else None, nb)):
                    if not wanted:
                        assert got is None, (name, want, bias)
                        continue
                    err, sc = float((got.cpu().double() - f * r).abs().max()), f * float(r.abs().max())
                    assert err <= hr.GATE * sc, (name, want, bias, scale, err, sc)


def test_coverage_summary():
    """What the cases above launch, worked out from their shapes (quoted by docs/NOTEBOOK.md): every KT of the fused kernel, both
    dx slice counts, all nine cells of the loss sum, the workgroup counts around eight and at the cap."""
    kt, slices, cells, blocks = set(), set(), set(), set()
    for _, K, V in hr.PRODUCT_SHAPES + hr.GTL_SHAPES + [(16, 128, v) for v in (200, 257, 32769)]:
        if "gtl" in hr.forms_for(K):
            nb = hr.gtl_blocks(V)
            kt.add(K // 64), blocks.add(nb)
            cells |= set(range(min(nb, 8))) | {8}
        if "dx" in hr.forms_for(K):
            slices.add(hr.dx_slices(V))
    print("head-coverage KT=%s dx-slices=%s loss-cells=%s workgroups=%s" % tuple(sorted(v) for v in (kt, slices, cells, blocks)))
    assert kt == set(range(1, 8)) and slices == {8, 32} and cells == set(range(9)) and blocks >= {1, 2, 7, 8, 9, 1024}
