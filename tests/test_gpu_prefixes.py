"""Every prefix of a session as a sample, on the device (csrc_prefixes/prefixes.hip through mobgt_amd.prefixes) against
`data.prefix_stats_host`: integers, compared for equality, on the crafted cases of prefixes_cases.py -- history lengths on either
side of the wave's chunk edges, one session of 4096 rows, repeats that straddle a chunk edge, extreme ids, a partly filled last
workgroup, every min_history that moves the first stored lane across an edge -- and on golden G14's log through sessionize.  Then
the return codes, the status word, and a PrefixDataset through the collator and the loops against explicitly truncated sessions."""
import ctypes

import numpy as np
import pytest
import torch

import checkins_cases as cc
import prefixes_cases as pc
from mobgt_amd import _prefixes, data, prefixes
from mobgt_amd.model_fqandtoyo import Graphormer
from mobgt_amd.train import EpochLoop, EvalLoop, PredictLoop
from mobgt_amd.workloads import FSQ_MODEL_ARGS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("h", pc.MIN_HISTORIES)
@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_device_form_equals_the_host_form(name, h):
    pc.assert_same(data.prefix_stats(pc.case(name), h, device=DEV), pc.host(name, h))


@pytest.mark.parametrize("sel", sorted(pc.SELECTIONS))
@pytest.mark.parametrize("h", (1, 64))
def test_device_form_over_chosen_sessions(sel, h):
    ds = pc.case("lengths")
    sessions = pc.SELECTIONS[sel](len(ds))
    pc.assert_same(data.prefix_stats(ds, h, sessions, device=DEV), data.prefix_stats_host(ds, h, sessions))


@pytest.fixture(scope="module")
def g14():
    """G14's log through sessionize and build_universe, a collator and an fq model on that universe."""
    res = data.sessionize(device=DEV, **cc.g14_log("sorted"))
    built = data.build_universe(res.dataset, train=res.train, coords_deg=res.coords_deg, radius_km=3.0, device=DEV)
    coll = data.SessionCollator(DEV, bin_table=built.bins.table)
    torch.manual_seed(14)
    model = Graphormer(universe=built.universe, num_bins=built.bins.num_bins + 2, **FSQ_MODEL_ARGS).to(DEV)
    return res, built, coll, model


def test_train_prefixes_of_g14(g14):
    res = g14[0]
    for h in (1, 3):
        got = data.prefix_stats(res.dataset, h, sessions=res.train, device=DEV)
        pc.assert_same(got, data.prefix_stats_host(res.dataset, h, sessions=res.train))
        assert len(got.session) > int(res.train.sum()) and res.train[got.session].all()


# ------------------------------------------------------------------------------------------------ the entry point itself
def _direct(ds, h=1, Q=None, offsets=None, pcum=None):
    """Device buffers of a direct call: (arguments in the order of the prototype as a dict, the tensors that own them)."""
    S, M = len(ds), int(ds.seq.shape[0])
    cnt = np.maximum(np.diff(ds.offsets) - h, 0)
    t = dict(seq=torch.from_numpy(ds.seq).to(DEV), offsets=torch.from_numpy(ds.offsets if offsets is None else offsets).to(DEV),
             pcum=torch.from_numpy(np.r_[0, np.cumsum(cnt)].astype(np.int64) if pcum is None else pcum).to(DEV))
    Q = int(cnt.sum()) if Q is None else Q
    for k in ("session", "cut", "n", "mult"):
        t[k] = torch.full((max(Q, 1),), 77, dtype=torch.int32, device=DEV)                       # (poisoned: every element is written)
    t["status"] = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    return t, S, M, Q


def _call(t, S, M, Q, h, **ptr):
    p = {k: ctypes.c_void_p(v.data_ptr()) for k, v in t.items()}
    p.update(ptr)
    rc = _prefixes.LIBRARY.lib().mobgt_prefixes_stats(p["seq"], p["offsets"], p["pcum"], None, S, M, Q, h, p["session"], p["cut"], p["n"],
                                                      p["mult"], p["status"], ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


def test_return_codes_with_nothing_launched():
    ds = pc.case("lengths")
    t, S, M, Q = _direct(ds)
    before = {k: v.clone() for k, v in t.items()}
    assert _call(t, S, M, Q, 0) == _prefixes.EBADDIM                                               # min_history = 0
    assert _call(t, -1, M, Q, 1) == _prefixes.EBADDIM                                              # S < 0
    assert _call(t, S, M, M + 1, 1) == _prefixes.EBADDIM                                           # Q > M
    assert _call(t, S, -1, 0, 1) == _prefixes.EBADDIM and _call(t, S, 2 ** 31, Q, 1) == _prefixes.EBADDIM
    for name in ("session", "cut", "n", "mult", "status", "seq", "offsets", "pcum"):
        assert _call(t, S, M, Q, 1, **{name: ctypes.c_void_p(0)}) == _prefixes.EALIGN, name        # a null buffer
    for name, off in (("session", 2), ("mult", 1), ("status", 2), ("seq", 2), ("offsets", 4), ("pcum", 4)):
        assert _call(t, S, M, Q, 1, **{name: ctypes.c_void_p(t[name].data_ptr() + off)}) == _prefixes.EALIGN, name
    assert all(torch.equal(v, before[k]) for k, v in t.items())                                    # nothing was launched
    with pytest.raises(_prefixes.MobgtPrefixesError, match="MOBGT_PREFIXES_EBADDIM") as e:
        _prefixes.launch("mobgt_prefixes_stats", *([None] * 4), S, M, Q, 0, *([None] * 6))
    assert e.value.code == _prefixes.EBADDIM
    assert _call(t, S, M, Q, 1) == 0 and int(t["status"][0]) == 0                                  # and the same buffers are good


def _arrays(t, Q):
    return data.PrefixStats(*(t[k][:Q].cpu().numpy() for k in ("session", "cut", "n", "mult")))


def test_the_status_word(monkeypatch):
    """An offsets entry above M is never an index: the kernels skip the sessions that read it and raise SBADINDEX; every other
    session's samples are right, the skipped ones' keep the fill -- no fault, and the next call on the same device is right."""
    ds, want = pc.case("lengths"), pc.host("lengths")
    S, M = len(ds), int(ds.seq.shape[0])
    for s, hit in ((S, [S - 1]), (4, [3, 4]), (0, [0])):                                           # (offsets[4]: the end of a 129-row session)
        offsets = ds.offsets.copy()
        offsets[s] = M + 5 if s else -1
        t, S, M, Q = _direct(ds, offsets=offsets)
        assert _call(t, S, M, Q, 1) == 0 and int(t["status"][0]) == _prefixes.SBADINDEX
        got, skipped = _arrays(t, Q), np.isin(want.session, hit)
        assert skipped.any() and np.all(got.session[skipped] == -1)
        assert all(np.all(v[skipped] == 0) for v in got[1:])
        assert all(np.array_equal(a[~skipped], b[~skipped]) for a, b in zip(got, want))
    # output positions that disagree with the sample count, or run backwards
    pcum = np.r_[0, np.cumsum(np.diff(ds.offsets) - 1)].astype(np.int64)
    for s, value in ((7, pcum[7] + 1), (7, pcum[6] - 1), (S, pcum[S] + 1)):
        bad = pcum.copy()
        bad[s] = value
        t, S, M, Q = _direct(ds, pcum=bad)
        assert _call(t, S, M, Q, 1) == 0 and int(t["status"][0]) == _prefixes.SBADINDEX
        got, skipped = _arrays(t, Q), np.isin(want.session, [s - 1, s])
        assert np.all(got.session[skipped] == -1) and all(np.array_equal(a[~skipped], b[~skipped]) for a, b in zip(got, want))
    t, S, M, Q = _direct(ds)
    assert _call(t, S, M, Q, 1) == 0 and int(t["status"][0]) == 0
    pc.assert_same(_arrays(t, Q), want)
    # the public call: the same corruption, injected behind the host's validation, is a ValueError naming the session
    launch = prefixes._launch

    def corrupt(d_seq, d_offsets, *rest):
        d_offsets[13] = M + 5
        return launch(d_seq, d_offsets, *rest)
    monkeypatch.setattr(prefixes, "_launch", corrupt)
    with pytest.raises(ValueError, match=rf"status {_prefixes.SBADINDEX}\), the first of them session 12:"):
        data.prefix_stats(ds, device=DEV)
    monkeypatch.undo()
    pc.assert_same(data.prefix_stats(ds, device=DEV), want)


# ------------------------------------------------------------------------------------------------ the collator and the loops
def test_collated_prefixes_equal_collated_truncated_sessions(g14):
    res, built, coll, _ = g14
    pds = data.PrefixDataset(res.dataset, sessions=res.train, device=DEV)
    first = int(np.nonzero(pds.session == pds.session[0])[0][-1]) + 1                              # the cuts of the first session
    ids = list(range(first)) + [first + 2, len(pds) - 1, first, len(pds) // 2, 1]                  # ... mixed with cuts of others
    assert len(set(pds.session[ids].tolist())) >= 4 and first >= 4
    got, want = coll([pds[i] for i in ids]), coll(pc.truncated(pds, ids))
    for f in data.DeviceBatch1._fields:
        x, y = getattr(got, f), getattr(want, f)
        assert x.is_cuda and x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), f
    assert got.x.shape[0] == len(ids) and torch.equal(got.y.cpu(), torch.tensor([int(pds[i].checkins[-1, 0]) for i in ids]))


def test_predict_and_eval_loops_over_prefixes_equal_those_over_truncated_sessions(g14):
    res, built, coll, model = g14
    pds = data.PrefixDataset(res.dataset, sessions=~res.train, device=DEV)
    explicit = data.SessionDataset(pc.truncated(pds))
    assert len(pds) == len(explicit) > int((~res.train).sum()) and np.array_equal(explicit.n, pds.n) and np.array_equal(explicit.mult, pds.mult)
    model.eval()
    si, ii, vi = PredictLoop(model, coll, pds, k=5).run()
    se, ie, ve = PredictLoop(model, coll, explicit, k=5).run()
    torch.cuda.synchronize()
    assert torch.equal(si, se) and si.tolist() == list(range(len(pds))) and torch.equal(ii, ie) and torch.equal(vi, ve)
    assert int(ii.min()) >= 0 and bool(torch.isfinite(vi).all())
    got, want = EvalLoop(model, coll, pds).run(), EvalLoop(model, coll, explicit).run()
    assert got["n"] == want["n"] == len(pds)
    keys = [k for k in got if "acc" in k.lower()]
    assert len(keys) == 4, sorted(got)
    assert all(got[k] == want[k] for k in keys)
    rows = model.recommend(pds, coll, k=5)
    assert all(len(r) == len(pds) for r in rows)


def test_an_epoch_loop_trains_on_prefixes(g14):
    res, built, coll, _ = g14
    torch.manual_seed(15)
    model = Graphormer(universe=built.universe, num_bins=built.bins.num_bins + 2, **FSQ_MODEL_ARGS).to(DEV)       # (of its own: it trains)
    pds = data.PrefixDataset(res.dataset, sessions=res.train, device=DEV)
    losses = []
    out = EpochLoop(model, coll, pds, batch_size=16, shuffle=False).run_epoch(max_steps=3, on_step=lambda k, l: losses.append(l))
    torch.cuda.synchronize()
    assert out["steps"] == 3 and out["sample_ids"] == list(range(48)) and len(losses) == 3
    assert all(bool(torch.isfinite(l.float()).all()) for l in losses)
