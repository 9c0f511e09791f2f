"""The burst scatter of the encoder input's gradients (libmobgt_tokscatter: mobgt_tokscatter_bwd; forms "scatter_burst",
"dist_gu_ride") against the launch it replaces, mobgt_embed_gather_multi's backward, and against a float64 index_add.

Kernel level.  Gradient values are small integers, |v| <= 64, and at most 608 rows meet in one table row: every sum is below 2^24
and exact in f32 whatever the order of the atomics, so the three results are compared with torch.equal -- no tolerance.  An
identity job's destination is pre-filled with NaN: the launch writes every row of it, pads as zeros.  The ride's gu is compared
bit for bit (the whole buffer, the columns beyond R included) with ops.small_gemm's on the gradient the old form would have seen.

Step level: TrainStep on an S-FSQ batch, 2 layers, both forms on against off from one restored state."""
import collections
import ctypes

import pytest
import torch

import token_abi as tabi
from mobgt_amd import _lib, _tokhost, _tokscatter, ops
from mobgt_amd.ops import _stream

pytestmark = pytest.mark.gpu
DEV = "cuda"
ENTRY = "mobgt_tokscatter_bwd"
ROWS = (1, 3, 4, 5, 37 * 2, 608)
WIDTHS = (4, 32, 64, 68, 128, 192, 192, 32)
PATTERNS = ("random", "all_skip", "one_row", "neg_front", "neg_middle", "neg_end", "null_table", "random")
TI = {tabi.I64: torch.int64, tabi.I32: torch.int32}
_vp, _ci, _i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64


def _job(gen, R, width, pattern, k, dtype):
    """One job: a [rows, width] table, an index of `pattern`, integer gradient rows in a buffer wider than the job."""
    rows, skip = 7 + k, (2 if pattern in ("all_skip", "neg_middle") else -1)
    coff = (0, 4, 32)[k % 3]
    ld = coff + width + (0, 4)[k % 2]
    idx = torch.randint(0, rows, (R,), generator=gen)
    if pattern == "all_skip":
        idx[:] = skip
    elif pattern == "one_row":
        idx[:] = 3
    elif pattern == "neg_front":
        idx[:max(1, R // 3)] = -1
    elif pattern == "neg_middle":
        idx[R // 3:max(R // 3 + 1, 2 * R // 3)] = -1
    elif pattern == "neg_end":
        idx[R - max(1, R // 3):] = -1
    buf = torch.randint(-64, 65, (R, ld), generator=gen).float()
    return dict(rows=rows, width=width, coff=coff, ld=ld, skip=skip, idx=idx.to(DEV, dtype), buf=buf.to(DEV), null=pattern == "null_table")


def _reference(j, extra):
    """float64 index_add of the job's live rows (+ the row-0 vector)."""
    ref = torch.zeros(j["rows"], j["width"], dtype=torch.float64, device=DEV)
    idx = j["idx"].long()
    live = (idx >= 0) & (idx != j["skip"])
    ref.index_add_(0, idx[live], j["buf"][live, j["coff"]:j["coff"] + j["width"]].double())
    if extra is not None:
        ref[0] += extra.double()
    return ref


def _old(jobs, R, code, extra, extra_job):
    outs = [None if j["null"] else torch.zeros(j["rows"], j["width"], device=DEV) for j in jobs]
    jd = [dict(d_table=o, idx=j["idx"], skip=j["skip"], width=j["width"], coff=j["coff"], buf=j["buf"], ld=j["ld"]) for j, o in zip(jobs, outs)]
    _lib.check(tabi.gather_multi(jd, R, code, backward=True, extra_row0=extra, extra_job=extra_job, tables=False), "mobgt_embed_gather_multi")
    return outs


def _args(jobs, outs, R, code, extra=None, extra_job=0, identity=-1, ride=None, n=None):
    m = len(jobs)
    ptrs = lambda ts: (_vp * m)(*[(t.data_ptr() if t is not None else 0) for t in ts])          # noqa: E731
    ride = ride if ride is not None else (None, 0, None, None, 0, 0)
    return (m if n is None else n, ptrs(outs), ptrs([j["idx"] for j in jobs]), (_i64 * m)(*[j["skip"] for j in jobs]),
            (_ci * m)(*[j["width"] for j in jobs]), (_ci * m)(*[j["coff"] for j in jobs]), ptrs([j["buf"] for j in jobs]),
            (_i64 * m)(*[j["ld"] for j in jobs]), R, code, tabi.ptr(extra), extra_job, identity, *ride, _stream())


def _new(jobs, R, code, extra, extra_job, identity=-1, fill=0.0):
    outs = [None if j["null"] else torch.full((j["rows"], j["width"]), fill if k == identity else 0.0, device=DEV) for k, j in enumerate(jobs)]
    _tokscatter.LIBRARY.check(_tokscatter.lib().mobgt_tokscatter_bwd(*_args(jobs, outs, R, code, extra, extra_job, identity)), ENTRY)
    return outs


@pytest.mark.parametrize("code", (tabi.I64, tabi.I32), ids=("i64", "i32"))
@pytest.mark.parametrize("R", ROWS)
def test_burst_scatter_against_the_old_launch_and_float64(R, code):
    gen = torch.Generator().manual_seed(100 * R + code)
    for nj in (1, 3, 8):
        first = {1: 5, 3: 3, 8: 0}[nj]                                # 1 job: width 192; 3 jobs: 68, 128, 192; 8: all of them
        jobs = [_job(gen, R, WIDTHS[(first + k) % 8], PATTERNS[(first + k) % 8] if nj > 1 else "neg_middle", k, TI[code]) for k in range(nj)]
        for with_extra in (False, True):
            extra_job = nj - 1                                        # (never the null-table job: that is job 6 of 8)
            extra = torch.randint(-64, 65, (jobs[extra_job]["width"],), generator=gen).float().to(DEV) if with_extra else None
            old, new = _old(jobs, R, code, extra, extra_job), _new(jobs, R, code, extra, extra_job)
            torch.cuda.synchronize()
            for k, j in enumerate(jobs):
                what = f"R={R} jobs={nj} job {k} ({j['width']} wide) extra={with_extra}"
                if j["null"]:
                    assert old[k] is None and new[k] is None
                    continue
                ref = _reference(j, extra if k == extra_job else None)
                assert torch.equal(new[k].double(), ref), (what, "burst against float64")
                assert torch.equal(old[k], new[k]), (what, "burst against mobgt_embed_gather_multi")


@pytest.mark.parametrize("pads", (False, True), ids=("no_pads", "pads"))
@pytest.mark.parametrize("code", (tabi.I64, tabi.I32), ids=("i64", "i32"))
@pytest.mark.parametrize("R", ROWS)
def test_identity_job_is_written_not_scattered(R, code, pads):
    """Job 0's table has one row per position and idx[r] = r (or -1: a pad); its destination starts as NaN."""
    gen = torch.Generator().manual_seed(7 * R + code)
    jobs = [_job(gen, R, w, p, k, TI[code]) for k, (w, p) in enumerate(((128, "random"), (32, "neg_end"), (192, "one_row")))]
    ident = torch.arange(R)
    if pads:
        ident[::3] = -1
        ident[R - 1] = -1
    jobs[0].update(rows=R, idx=ident.to(DEV, TI[code]), skip=-1)
    extra = torch.randint(-64, 65, (192,), generator=gen).float().to(DEV)
    old = _old(jobs, R, code, extra, 2)
    new = _new(jobs, R, code, extra, 2, identity=0, fill=float("nan"))
    torch.cuda.synchronize()
    for k, j in enumerate(jobs):
        assert torch.equal(new[k].double(), _reference(j, extra if k == 2 else None)), (R, k)
        assert torch.equal(old[k], new[k]), (R, k)


def test_refusals():
    R = 5
    gen = torch.Generator().manual_seed(1)
    jobs = [_job(gen, R, 64, "random", k, torch.int64) for k in range(9)]
    outs = [torch.zeros(j["rows"], j["width"], device=DEV) for j in jobs]
    entry = _tokscatter.lib().mobgt_tokscatter_bwd
    bad, w2 = _tokscatter.EBADDIM, torch.zeros(64, 64, device=DEV)
    gut = torch.zeros(64, 128, dtype=torch.bfloat16, device=DEV)
    ride = (tabi.ptr(w2), 64, None, tabi.ptr(gut), 128, 64)
    wide = dict(jobs[0], width=196, ld=200, buf=torch.zeros(R, 200, device=DEV))
    assert entry(*_args([wide], [torch.zeros(7, 196, device=DEV)], R, tabi.I64)) == bad               # wider than a lane's registers
    assert entry(*_args(jobs, outs, R, tabi.I64)) == bad                                              # nine jobs
    assert entry(*_args(jobs[:2], outs[:2], R, tabi.I64, n=0)) == bad
    assert entry(*_args(jobs[:2], outs[:2], R, 7)) == _tokscatter.EDTYPE
    assert entry(*_args(jobs[:2], outs[:2], R, tabi.I64, identity=2)) == bad                          # not a job
    assert entry(*_args(jobs[:2], [None, outs[1]], R, tabi.I64, identity=0)) == bad                   # an identity job without a table
    assert entry(*_args(jobs[:2], outs[:2], R, tabi.I64, extra=outs[0], extra_job=0, identity=0)) == bad
    assert entry(*_args(jobs[:2], outs[:2], R, tabi.I64, ride=ride)) == bad                           # a ride without an identity job
    assert entry(*_args(jobs[:2], outs[:2], R, tabi.I64, identity=0, ride=ride[:4] + (4, 64))) == bad  # gut rows shorter than R
    assert entry(*_args(jobs[:2], outs[:2], R, tabi.I64, identity=0, ride=(tabi.ptr(w2.data_ptr() + 4),) + ride[1:])) == _tokscatter.EALIGN
    torch.cuda.synchronize()
    assert all(float(o.abs().max()) == 0.0 for o in outs) and float(gut.float().abs().max()) == 0.0    # nothing was launched
    assert entry(*_args(jobs[:2], outs[:2], 0, tabi.I64)) == 0                                        # no rows: nothing to do


@pytest.mark.parametrize("NO", (64, 128))
@pytest.mark.parametrize("R", (5, 37 * 2, 608))
def test_ride_equals_the_small_gemm_launch_bit_for_bit(R, NO):
    """gu = (rs[r] (g W2^T))^T in bf16 from the identity job's gradient rows, pads (whose rows hold NaN here) as zeros."""
    gen = torch.Generator().manual_seed(R + NO)
    d_pt = torch.randn(R, NO + 32, generator=gen).to(DEV)
    ident = torch.arange(R)
    ident[1::4] = -1
    d_pt[ident.to(DEV) < 0] = float("nan")
    w2, rs = (torch.randn(64, NO, generator=gen) * 0.1).to(DEV), torch.rand(R, generator=gen).to(DEV)
    ld = (R + 127) // 128 * 128
    gut_old, gut_new = (torch.full((64, ld), 7.0, dtype=torch.bfloat16, device=DEV) for _ in range(2))
    jobs = [dict(rows=R, width=NO, coff=0, ld=NO + 32, skip=-1, idx=ident.to(DEV), buf=d_pt, null=False),
            dict(rows=9, width=32, coff=NO, ld=NO + 32, skip=0, idx=torch.randint(0, 9, (R,), generator=gen).to(DEV), buf=d_pt, null=True)]
    g = torch.full((R, NO), float("nan"), device=DEV)
    ride = (tabi.ptr(w2), w2.stride(0), tabi.ptr(rs), tabi.ptr(gut_new), ld, 64)
    _tokscatter.LIBRARY.check(_tokscatter.lib().mobgt_tokscatter_bwd(*_args(jobs, [g, None], R, tabi.I64, identity=0, ride=ride)), ENTRY)
    torch.cuda.synchronize()
    want_g = torch.where((ident.to(DEV) >= 0)[:, None], d_pt[:, :NO], torch.zeros((), device=DEV))
    assert torch.equal(g, want_g)
    ops.small_gemm(g, w2, b_is_nk=True, ct=(gut_old, rs, True))
    torch.cuda.synchronize()
    assert torch.equal(gut_new.view(torch.int16), gut_old.view(torch.int16))
    assert torch.equal(gut_new[:, R:].float(), torch.full((64, ld - R), 7.0, device=DEV))           # beyond R: untouched


# ------------------------------------------------------------------------------------------------------------------ step level
from test_gpu_l0_token_host import _fsq, _state_of, _step_from, _assert_within_spread, OLD_RUNS   # noqa: E402


class _Spy:
    """Stands in for the three libraries' handles and counts the calls of every entry point."""

    def __init__(self):
        self.calls = collections.Counter()
        self.real = {"mobgt_tokhost_": _tokhost.lib(), "mobgt_tokscatter_": _tokscatter.lib(), "": _lib.lib()}

    def install(self, monkeypatch):
        monkeypatch.setattr(_lib, "lib", lambda: self)
        monkeypatch.setattr(_tokhost.LIBRARY, "lib", lambda: self)
        monkeypatch.setattr(_tokscatter.LIBRARY, "lib", lambda: self)
        return self

    def __getattr__(self, name):
        self.calls[name] += 1
        return getattr(next(h for p, h in self.real.items() if name.startswith(p)), name)


@pytest.mark.parametrize("use_graph", (False, True), ids=("eager", "graph"))
def test_train_step_with_the_forms_on_and_off(use_graph, monkeypatch):
    """Both forms on, then both off (the old launches), each a fresh model of one seed and a TrainStep run from ONE state: the loss
    is equal, every parameter gradient within the spread of the old form's runs, nothing left parked.  The spy counts entry
    points: with the forms on the step calls mobgt_tokscatter_bwd where it called mobgt_embed_gather_multi's backward, one
    mobgt_small_gemm_f32_act fewer, and every other entry as often -- one launch less per captured (or eager) step.
    The absolute count (41 launches against 42) belongs to the benchmark's 6-layer S-FSQ step, not to this 2-layer model, and a
    captured graph offers no count of its kernel nodes to a test; it is read off the kernel trace of that step
    (profiles/r8_bench_fsq_step_seq.txt against r7's).  Every entry counted here is one launch, so the difference is exact."""
    from mobgt_amd import forms
    from mobgt_amd.train import TrainStep
    res, state, calls = {}, None, {}
    spy = _Spy().install(monkeypatch)
    for on in (True, False):
        with forms.using(scatter_burst=on, dist_gu_ride=on, scatter_burst_eager=not use_graph, dist_gu_ride_eager=not use_graph):
            spy.calls.clear()
            model, batches = _fsq()
            ts = TrainStep(model, batches, use_graph=use_graph, seed=1)
            ts.prepare()
            if state is None:
                state = _state_of(ts)
            runs = []
            for rep in range(3 if on else OLD_RUNS):
                runs.append(_step_from(ts, state))
                assert ops.step_state_leftovers() == {}
                if rep == 0:
                    calls[on] = collections.Counter(spy.calls)
            assert not ts.check_faults(on_fault="return")
            res[on] = (ts, runs)
    (ts_off, off), (ts_on, on_) = res[False], res[True]
    assert all(l == off[0][0] for l, _ in off + on_), [l for l, _ in off + on_]          # the loss is equal
    for rep, (_, g) in enumerate(on_):
        _assert_within_spread(ts_on, ts_off, g, [f for _, f in off], f"use_graph={use_graph} run {rep}")
    k = calls[True][ENTRY]
    assert k >= 1 and calls[False][ENTRY] == 0, (calls[True][ENTRY], calls[False][ENTRY])
    # (queries launch nothing, and their answers are remembered per process: the first trainer of the test asks, the second does not)
    diff = {n: calls[False][n] - calls[True][n] for n in set(calls[False]) | set(calls[True])
            if calls[False][n] != calls[True][n] and not n.endswith(("_bytes", "_size", "_version"))}
    assert diff == {ENTRY: -k, "mobgt_embed_gather_multi": k, "mobgt_small_gemm_f32_act": k}, diff


@pytest.mark.parametrize("why", ("scatter_form_off", "identity_absent"))
def test_nothing_stays_parked_when_the_scatter_does_not_take_the_job(why, monkeypatch):
    """The distance GCN parks its gu product; the scatter does not take it (its form is off / it has no identity job): the GCN's
    backward runs the product itself and drops the job."""
    from mobgt_amd import forms
    from mobgt_amd.step_state import STEP
    from mobgt_amd.train import TrainStep
    parked = []
    real_park = ops.park_dist_gu_job

    def park(*a):
        job = real_park(*a)
        parked.append(job)
        return job
    monkeypatch.setattr(ops, "park_dist_gu_job", park)
    if why == "identity_absent":
        real_gather = ops.embed_gather_multi
        monkeypatch.setattr(ops, "embed_gather_multi", lambda jobs, widths, identity=None: real_gather(jobs, widths, identity=None))
    spy = _Spy().install(monkeypatch)
    with forms.using(scatter_burst_eager=True, dist_gu_ride_eager=True):
        model, batches = _fsq()
        ts = TrainStep(model, batches, use_graph=False, seed=1)
        ts.prepare()
        state = _state_of(ts)
        _, want = _step_from(ts, state)
        del parked[:]
        spy.calls.clear()
        if why == "scatter_form_off":
            # (parked with both forms on, then the scatter's form goes off before the backward decides: the forward's decision is
            #  the gather node's, so switch it there)
            real_fwd = ops._GatherMultiFn.forward

            def fwd(ctx, *a):
                out = real_fwd(ctx, *a)
                ctx.burst = False
                return out
            monkeypatch.setattr(ops._GatherMultiFn, "forward", staticmethod(fwd))
        _, got = _step_from(ts, state)
    assert parked and all(j is not None and not j.get("taken") for j in parked), parked
    assert STEP.dist_gu_job is None and ops.step_state_leftovers() == {}
    assert spy.calls["mobgt_small_gemm_f32_act"] >= 1 and (why == "identity_absent" or spy.calls[ENTRY] == 0)
    assert torch.isfinite(got).all() and float((got - want).abs().max()) <= 3e-3 * float(want.abs().max())
