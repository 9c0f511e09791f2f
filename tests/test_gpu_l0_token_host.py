"""The hosting form of the encoder input's backward (csrc/tokbwd_body.h, libmobgt_tokhost: mobgt_tokhost_token_bwd_chain; forms "l0_token_host"): the
launch that also finishes the FIRST encoder layer's backward -- its input gradient dx0 = dx1 + dqkv Wqkv and its four weight
gradients -- against the two launches it replaces, mobgt_layer_backward_tail followed by mobgt_token_bwd_chain.

Kernel level, on the same random inputs.  The hosted product sums K in the order of mobgt_layer_backward_tail's GEMM (eight partial
sums over the k-steps i, i + 8, i + 16, added in order, then dx1) and the passengers run that launch's tiles, splits and sums, so
  * dx0, d_nf, d_add, dx4, d_pt, the four dW and the two db are asserted BIT-IDENTICAL (torch.equal) to the two-launch form;
  * d_token is a sum over the graphs -- by f32 atomics in whatever order they land in the old form, in float64 rounded once (up to
    16 graphs) in the hosted one: |hosted - old| <= the spread of two runs of the old form; where that spread cannot tell (the old
    form's atomics land in one order twice), the rule for one f32 sum split differently applies: against the float64 column sums
    of the token rows' d (the finished rows times the replayed dropout masks, as the kernel forms them), the hosted error is at
    most twice the old form's.  (It is in fact never larger: a correctly rounded sum is the f32 nearest to the exact one.)
  * a call without a tail equals today's kernel on every written output, with and without passengers;
  * a second launch on the same buffers (inputs put back) repeats every written output bit for bit.

Step level: TrainStep on an S-FSQ batch, 2 layers, with the form on and off from one restored state."""
import pytest
import torch

import token_abi as tabi
import wgrad_abi as wabi
from chain_abi import pack
from mobgt_amd import _lib, _tokhost
from mobgt_amd.ops import _stream

pytestmark = pytest.mark.gpu
DEV = "cuda"
C, W2, F = 192, 160, 1024
SHAPES = ((1, 1), (1, 15), (1, 16), (3, 11), (2, 16), (16, 37))
SEED = 0x5EED1234
HOST = "mobgt_tokhost_token_bwd_chain"


def _inputs(G, N):
    g = torch.Generator(device="cpu").manual_seed(1000 * G + N)
    rn = lambda *s, k=1.0: (torch.randn(*s, generator=g) * k).to(DEV)          # noqa: E731
    T, Rn = N + 1, G * N
    R = G * T
    bf = lambda t: t.to(torch.bfloat16)                                          # noqa: E731
    i = dict(dx1=rn(R, C), dqkv=bf(rn(R, 3 * C, k=0.3)), wqkv=bf(rn(3 * C, C, k=0.08)),
             real=(torch.rand(Rn, generator=g) > 0.2).float().to(DEV), y4=rn(Rn, C), x4=rn(Rn, C), w4=rn(C, C, k=0.07), w2=rn(W2, W2, k=0.08))
    i["wqt"] = pack(i["wqkv"], transposed=True)
    # the layer's four problems (g, x, db?): dW2 = df^T h, dW1 = du^T z (+ db1), dWo = dy^T a, dWqkv = dqkv^T xa (+ dbqkv)
    i["items"] = [(bf(rn(R, C, k=0.2)), bf(rn(R, F)), False), (bf(rn(R, F, k=0.2)), bf(rn(R, C)), True),
                  (bf(rn(R, C, k=0.2)), bf(rn(R, C)), False), (i["dqkv"], bf(rn(R, C)), True)]
    return i


def _outputs(i, G, N, items):
    Rn = G * N
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=DEV)               # noqa: E731
    e = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=DEV)   # noqa: E731
    return dict(dout=i["dx1"].clone(), d_nf=e(Rn, C), d_add=e(Rn, C), dx4=e(Rn, C), d_pt=e(Rn, W2), d_token=z(C),
                dw=[z(g_.shape[1], x_.shape[1]) for g_, x_, _ in items], db=[z(g_.shape[1]) if b_ else None for g_, _, b_ in items])


def _token_args(i, o, G, N, p):
    return (tabi.ptr(o["dout"]), tabi.ptr(i["real"]), tabi.ptr(i["y4"]), tabi.ptr(i["x4"]), C, tabi.ptr(i["w4"]), tabi.ptr(i["w2"]),
            tabi.ptr(o["d_nf"]), tabi.ptr(o["d_add"]), tabi.ptr(o["dx4"]), C, tabi.ptr(o["d_pt"]), tabi.ptr(o["d_token"]), G, N, C, W2,
            0.2, 0.2, float(p), float(p), SEED, tabi.ptr(None), *tabi.SALTS)


def _group(items, o):
    n = len(items)
    return (n, wabi._ptrs([t[0] for t in items]), wabi._ints([t[0].stride(0) for t in items], wabi.I64), wabi._ptrs([t[1] for t in items]),
            wabi._ints([t[1].stride(0) for t in items], wabi.I64), wabi._ptrs(o["dw"]), wabi._ints([d.stride(0) for d in o["dw"]], wabi.I64),
            wabi._ptrs(o["db"]), wabi._ints([t[0].shape[1] for t in items]), wabi._ints([t[1].shape[1] for t in items]))


def _run_old(i, G, N, p, tail, items):
    """The two launches: [mobgt_layer_backward_tail | mobgt_linear_wgrad_group | nothing], then mobgt_token_bwd_chain."""
    o = _outputs(i, G, N, items)
    R = G * (N + 1)
    lib = _lib.lib()
    if items:
        grp = _group(items, o)
        head = grp[:8] + (R,) + grp[8:] + (wabi.BF16,)
        if tail:
            _lib.check(lib.mobgt_layer_backward_tail(*head, tabi.ptr(i["dqkv"]), 3 * C, tabi.ptr(i["wqkv"]), C, tabi.ptr(o["dout"]), C,
                                                     R, C, 3 * C, _stream()), "mobgt_layer_backward_tail")
        else:
            _lib.check(lib.mobgt_linear_wgrad_group(*head, _stream()), "mobgt_linear_wgrad_group")
    elif tail:                                     # (the launch takes at least one problem: a throw-away 2 x 2 one beside the tail)
        g2 = torch.zeros(R, 2, dtype=torch.bfloat16, device=DEV)
        dw2 = torch.zeros(2, 2, dtype=torch.float32, device=DEV)
        _lib.check(lib.mobgt_layer_backward_tail(1, wabi._ptrs([g2]), wabi._ints([2], wabi.I64), wabi._ptrs([g2]), wabi._ints([2], wabi.I64),
                                                 wabi._ptrs([dw2]), wabi._ints([2], wabi.I64), None, R, wabi._ints([2]), wabi._ints([2]),
                                                 wabi.BF16, tabi.ptr(i["dqkv"]), 3 * C, tabi.ptr(i["wqkv"]), C, tabi.ptr(o["dout"]), C,
                                                 R, C, 3 * C, _stream()), "mobgt_layer_backward_tail")
    _lib.check(lib.mobgt_token_bwd_chain(*_token_args(i, o, G, N, p), _stream()), "mobgt_token_bwd_chain")
    torch.cuda.synchronize()
    return o


def _launch_host(i, o, G, N, p, tail, items):
    grp = _group(items, o) if items else (0,) + (None,) * 9
    t = (tabi.ptr(i["dqkv"]), tabi.ptr(i["wqt"]), tabi.ptr(o["dout"])) if tail else (tabi.ptr(None),) * 3
    return _tokhost.lib().mobgt_tokhost_token_bwd_chain(*_token_args(i, o, G, N, p), *t, *grp, _stream())


def _run_host(i, G, N, p, tail, items):
    o = _outputs(i, G, N, items)
    _tokhost.LIBRARY.check(_launch_host(i, o, G, N, p, tail, items), HOST)
    torch.cuda.synchronize()
    return o


def _token_rows_f64(i, dx0, G, N, p):
    """float64 column sums of the graph-token rows' d = dx0[g T] * masks, the products formed in f32 as the kernel forms them."""
    from mobgt_amd import ops
    T = N + 1
    rows = dx0.view(G, T, C)[:, 0].cpu()
    scale = torch.ones(G, C)
    if p:
        one = torch.ones((), dtype=torch.float32)                    # (1 / keep in f32, as the launcher forms it)
        ik = one / (one - torch.tensor(float(int(p * 65536.0 + 0.5)), dtype=torch.float32) / 65536.0)
        scale = torch.from_numpy(ops.dropout_site_mask(SEED, tabi.SALTS[1], G, C, p)).float() * ik
        keep_in = torch.from_numpy(ops.dropout_site_mask(SEED, tabi.SALTS[2], G * T, C, p)).view(G, T, C)[:, 0]
        scale = scale * (keep_in.float() * ik)
    return (rows * scale).double().sum(0)


WRITTEN = ("dout", "d_nf", "d_add", "dx4", "d_pt")


def _assert_equal(a, b, what, names=WRITTEN):
    for k in names:
        assert torch.equal(a[k], b[k]), (what, k, float((a[k] - b[k]).abs().max()))


@pytest.mark.parametrize("p", (0.0, 0.1), ids=("no_dropout", "dropout"))
@pytest.mark.parametrize("G,N", SHAPES, ids=[f"G{g}_N{n}" for g, n in SHAPES])
def test_hosted_launch_against_the_two_launches(G, N, p):
    i = _inputs(G, N)
    for tail in (False, True):
        for items in ([], i["items"]):
            what = f"G={G} N={N} p={p} tail={tail} n_wg={len(items)}"
            old, old2 = _run_old(i, G, N, p, tail, items), _run_old(i, G, N, p, tail, items)
            got = _run_host(i, G, N, p, tail, items)
            if tail:
                assert not torch.equal(got["dout"], i["dx1"]), what           # the product really landed
            else:
                assert torch.equal(got["dout"], i["dx1"]), what               # no tail: dout is only read
            _assert_equal(got, old, what)
            _assert_equal(old2, old, what + " (two runs of the old form)")
            for k in range(len(items)):
                for name, a, b, b2 in (("dw", got["dw"][k], old["dw"][k], old2["dw"][k]), ("db", got["db"][k], old["db"][k], old2["db"][k])):
                    if a is None:
                        continue
                    spread = float((b - b2).abs().max())
                    diff = float((a - b).abs().max())
                    print(f"{what} {name}[{k}]: |hosted - old| {diff:.3e}  spread of the old form {spread:.3e}")
                    assert diff <= spread, (what, name, k, diff, spread)
            # d_token: atomics over the graphs
            spread = float((old["d_token"] - old2["d_token"]).abs().max())
            diff = float((got["d_token"] - old["d_token"]).abs().max())
            ref = _token_rows_f64(i, old["dout"], G, N, p)
            e_got = float((got["d_token"].double().cpu() - ref).abs().max())
            e_old = max(float((o_["d_token"].double().cpu() - ref).abs().max()) for o_ in (old, old2))
            print(f"{what} d_token: |hosted - old| {diff:.3e}  spread {spread:.3e}  |. - f64| hosted {e_got:.3e} old {e_old:.3e}")
            assert diff <= spread or e_got <= 2 * e_old, (what, diff, spread, e_got, e_old)
            # the launch again on the same buffers, inputs put back: every written output repeats
            again = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in got.items()}
            got["dout"].copy_(i["dx1"])
            got["d_token"].zero_()
            for t in got["dw"] + [b for b in got["db"] if b is not None]:
                t.zero_()
            _tokhost.LIBRARY.check(_launch_host(i, got, G, N, p, tail, items), HOST)
            torch.cuda.synchronize()
            _assert_equal(got, again, what + " (second launch)")


def test_refusals_of_the_hosting_entry():
    G, N = 2, 5
    i = _inputs(G, N)
    o = _outputs(i, G, N, i["items"])
    bad = _tokhost.EBADDIM
    host = _tokhost.lib().mobgt_tokhost_token_bwd_chain
    base = _token_args(i, o, G, N, 0.0)
    grp = _group(i["items"], o)
    none = (0,) + (None,) * 9
    null = tabi.ptr(None)
    # half a tail; a tail whose dx1 is not dout; too many problems; problems without their arrays; misaligned tail operands
    assert host(*base, tabi.ptr(i["dqkv"]), null, tabi.ptr(o["dout"]), *none, _stream()) == bad
    assert host(*base, null, tabi.ptr(i["wqt"]), tabi.ptr(o["dout"]), *none, _stream()) == bad
    assert host(*base, tabi.ptr(i["dqkv"]), tabi.ptr(i["wqt"]), tabi.ptr(i["dx1"]), *none, _stream()) == bad
    assert host(*base, null, null, null, 5, *grp[1:], _stream()) == bad
    assert host(*base, null, null, null, 4, *(None,) * 9, _stream()) == bad
    assert host(*base, tabi.ptr(i["dqkv"].data_ptr() + 2), tabi.ptr(i["wqt"]), tabi.ptr(o["dout"]), *none,
                                          _stream()) == _tokhost.EALIGN
    # more token rows than the launch it reproduces serves
    Gb, Nb = 16, 64
    assert Gb * (Nb + 1) > _tokhost.MAX_ROWS
    ib = _inputs(Gb, Nb)
    ob = _outputs(ib, Gb, Nb, [])
    assert _launch_host(ib, ob, Gb, Nb, 0.0, True, []) == bad
    torch.cuda.synchronize()
    assert torch.equal(o["dout"], i["dx1"]) and torch.equal(ob["dout"], ib["dx1"])          # nothing was launched


# ------------------------------------------------------------------------------------------------------------------ step level
def _fsq(seed=1):
    from mobgt_amd import workloads
    uni, model, coll = workloads.build("fsq", DEV, seed=seed, model_overrides=dict(n_layers=2))
    batches = [coll(t) for t in workloads.make_pool("fsq", 1, 16, uni)]
    return model, batches


def _state_of(ts):
    return (ts.flat_params.tensor.detach().clone(), ts.exp_avg.clone(), ts.exp_avg_sq.clone(), ts.seed_dev.clone())


def _restore(ts, state):
    with torch.no_grad():
        ts.flat_params.tensor.copy_(state[0]); ts.exp_avg.copy_(state[1]); ts.exp_avg_sq.copy_(state[2]); ts.seed_dev.copy_(state[3])
        ts.sync_shadows()


def _step_from(ts, state):
    _restore(ts, state)
    loss = float(ts.step(0))
    torch.cuda.synchronize()
    return loss, ts.flat.flat.detach().clone()


class _Spy:
    """Stands in for both libraries' handles (`_lib.lib`, `_tokhost.LIBRARY.lib`) and counts the calls of the entries:
    (name, tail given, problems)."""

    def __init__(self):
        self.calls, self.real, self.real_host = [], _lib.lib(), _tokhost.lib()

    def install(self, monkeypatch):
        monkeypatch.setattr(_lib, "lib", lambda: self)
        monkeypatch.setattr(_tokhost.LIBRARY, "lib", lambda: self)
        return self

    def __getattr__(self, name):
        fn = getattr(self.real_host if name.startswith("mobgt_tokhost_") else self.real, name)
        if name == "mobgt_token_bwd_chain":
            self.calls.append((name, False, 0))
        elif name == HOST:
            def call(*a):
                self.calls.append((name, bool(a[26].value), int(a[29])))
                return fn(*a)
            return call
        elif name == "mobgt_layer_backward_tail":
            self.calls.append((name, True, 4))
        return fn


def _per_parameter(ts, flat):
    names = {id(p): n for n, p in ts.model.named_parameters()}
    out, base = {}, ts.flat.flat.data_ptr()
    for p, v in zip(ts.flat.params, ts.flat.views):
        o = (v.data_ptr() - base) // 4                        # (the slices are aligned: not back to back)
        assert v.is_contiguous() and 0 <= o and o + v.numel() <= flat.numel()
        out[names[id(p)]] = flat[o:o + v.numel()]
    return out


# Runs of the OLD form that measure its run-to-run spread.  Its gradients come in a few discrete variants per parameter (f32 atomics
# upstream land in one of a few orders, and whole groups of parameters switch together: 2-4 distinct values in 8 runs, measured), so
# a handful of runs often misses a variant that a later run -- of either form -- then shows; a step takes a millisecond.
OLD_RUNS = 24


def _assert_within_spread(ts_new, ts_old, new, olds, what):
    """Every parameter's gradient: |new - nearest old| <= the largest difference between any two runs of the old form."""
    by_new = _per_parameter(ts_new, new)
    by_old = [_per_parameter(ts_old, f) for f in olds]
    worst = ("", 0.0, 0.0)
    for n, v in by_new.items():
        if not v.numel():
            continue
        runs = torch.stack([a[n] for a in by_old])                       # [runs, elements]
        spread = float((runs.amax(0) - runs.amin(0)).max())              # = the largest |a - b| over all pairs of runs
        diff = float((runs - v).abs().amax(1).min())                     # to the nearest run
        if diff > worst[1]:
            worst = (n, diff, spread)
        assert diff <= spread, (what, n, diff, spread)
    print(f"{what}: largest |new - old| {worst[1]:.3e} at {worst[0]} (spread of the old form there {worst[2]:.3e})")


@pytest.mark.parametrize("use_graph", (False, True), ids=("eager", "graph"))
def test_train_step_with_the_form_on_and_off(use_graph, monkeypatch):
    """Pass one with the form on, pass two with it off, each a fresh model of one seed and a TrainStep run three times from ONE
    state: the loss is equal, every parameter gradient within the spread of the old form's runs, nothing left parked; the spy
    sees the hosted entry with a tail and four problems in pass one only (graph: while the step is captured; then three replays)."""
    from mobgt_amd import forms, ops
    from mobgt_amd.train import TrainStep
    res, state = {}, None
    spy = _Spy().install(monkeypatch)
    for on in (True, False):
        # (an eager step defers only when forms "l0_token_host_eager" asks; a step that is being captured defers by default)
        with forms.using(l0_token_host=on, l0_token_host_eager=not use_graph):
            model, batches = _fsq()
            ts = TrainStep(model, batches, use_graph=use_graph, seed=1)
            ts.prepare()
            if state is None:
                state = _state_of(ts)
            runs = []
            for rep in range(3 if on else OLD_RUNS):
                if not use_graph or rep:
                    del spy.calls[:]
                runs.append(_step_from(ts, state))
                assert ops.step_state_leftovers() == {}
                host = [c for c in spy.calls if c[0] == HOST]
                plain = [c for c in spy.calls if c[0] == "mobgt_token_bwd_chain"]
                tails = [c for c in spy.calls if c[0] == "mobgt_layer_backward_tail"]
                if use_graph and rep:
                    assert not host and not plain and not tails, spy.calls             # a replay calls nothing
                elif on:            # the hosted entry with a tail and four problems; the layer's own launch is gone
                    assert host and set(host) == {(HOST, True, 4)}, spy.calls
                    # (graph: the calls since the trainer was built -- its eager passes in front of the capture do not defer)
                    assert use_graph or (len(host) == 1 and not tails and not plain), spy.calls
                else:
                    assert not host and plain and len(tails) >= len(plain), spy.calls
                    assert use_graph or len(plain) == len(tails) == 1, spy.calls
            assert not ts.check_faults(on_fault="return")
            res[on] = (ts, runs)
    (ts_off, off), (ts_on, on_) = res[False], res[True]
    assert all(l == off[0][0] for l, _ in off + on_), [l for l, _ in off + on_]          # the loss is equal
    for rep, (_, g) in enumerate(on_):
        _assert_within_spread(ts_on, ts_off, g, [f for _, f in off], f"use_graph={use_graph} run {rep}")


@pytest.fixture
def eager_host():
    """Eager steps defer too (forms "l0_token_host_eager"): the two cases below watch single eager steps."""
    from mobgt_amd import forms
    with forms.using(l0_token_host_eager=True):
        yield


def test_a_cut_in_front_of_the_first_layer_defers_nothing(monkeypatch, eager_host):
    """Layer 0 carrying `_mobgt_cut` (the trainer's layer-wise gradient buckets cut the backward pass in front of it): its tail is
    its own launch, the encoder input's backward is the plain one."""
    from mobgt_amd import ops
    from mobgt_amd.train import TrainStep
    model, batches = _fsq()
    ts = TrainStep(model, batches, use_graph=False, seed=1)
    ts.prepare()
    state = _state_of(ts)
    spy = _Spy().install(monkeypatch)
    _, want = _step_from(ts, state)
    assert (HOST, True, 4) in spy.calls                          # (without the cut the step defers)
    del spy.calls[:]
    model.layers[0]._mobgt_cut = True
    try:
        _, got = _step_from(ts, state)
    finally:
        monkeypatch.undo()
        model.layers[0]._mobgt_cut = False
    names = [c[0] for c in spy.calls]
    assert HOST not in names and names.count("mobgt_token_bwd_chain") == 1 \
        and names.count("mobgt_layer_backward_tail") == 1, spy.calls
    assert ops.step_state_leftovers() == {}
    assert torch.isfinite(got).all() and float((got - want).abs().max()) <= 3e-3 * float(want.abs().max())


def test_a_backward_that_raises_between_the_park_and_the_launch_leaves_nothing_behind(eager_host):
    """The first layer parks its tail, the token assembly's backward takes it along, and the node after it raises (a hook on
    FuseEmbeddings-4's output, host side): ops.recording_wgrads drops everything parked, the tail included, and the next step is
    a clean step."""
    from mobgt_amd import ops
    from mobgt_amd.step_state import STEP
    from mobgt_amd.train import TrainStep
    model, batches = _fsq()
    ts = TrainStep(model, batches, use_graph=False, seed=1)
    ts.prepare()
    state = _state_of(ts)
    _, want = _step_from(ts, state)

    class Boom(Exception):
        pass
    seen = {}

    def boom(_g):
        seen["pending"] = [bool(p_.get("tail")) for p_ in STEP.token_pending.values()]
        raise Boom("between the park and the launch")
    real = ops.register_token_chain

    def hooked(nf, *a, **k):
        real(nf, *a, **k)
        if nf.requires_grad:
            nf.register_hook(boom)
    ops.register_token_chain = hooked
    raised = False
    try:
        _restore(ts, state)
        try:
            ts.step(0)
        except Boom:
            raised = True
    finally:
        ops.register_token_chain = real
    torch.cuda.synchronize()
    assert raised and seen["pending"] == [True], seen            # the tail was travelling with the parked chain
    assert ops.step_state_leftovers() == {} and not STEP.layer_tails and not STEP.token_pending
    _, after = _step_from(ts, state)
    assert ops.step_state_leftovers() == {}
    assert float((after - want).abs().max()) <= 3e-3 * float(want.abs().max())
