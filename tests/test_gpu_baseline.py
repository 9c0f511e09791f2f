"""The Markov baseline on the device (csrc_baseline/baseline.hip through mobgt_amd.baseline) against baseline.ranks_host /
topk_host: integers, compared for equality, on every crafted case of baseline_cases.py -- row lengths on either side of the wave's
64 entries, the target at either end of its row or absent from it, the first and the last range of the user table, history
lengths 1 .. 4096 with the only revisit on either side of row 64, a partly filled last workgroup, no sample at all -- for all three
orders, and on golden G14's log through sessionize.  Then the fit on the device against the fit in numpy, and the two entry
points themselves: return codes with nothing launched, every output element written, and the status word for indices that the
kernels must refuse without reading through them."""
import ctypes

import numpy as np
import pytest
import torch

import baseline_cases as bc
import checkins_cases as cc
from mobgt_amd import _baseline, baseline, data

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def fitted():
    cache = {}

    def get(name):
        if name not in cache:
            c = bc.case(name)
            cache[name] = data.MarkovBaseline.fit(c.ds, c.train, device=DEV)
        return cache[name]
    return get


# ------------------------------------------------------------------------------------------------ device against host
@pytest.mark.parametrize("order", bc.ORDERS)
@pytest.mark.parametrize("name", sorted(bc.CASES))
def test_device_ranks_equal_the_host_form(fitted, name, order):
    rank, revisit = fitted(name).ranks(bc.case(name).samples, order)
    want = bc.host(name, order)
    assert rank.dtype == torch.int32 and revisit.dtype == torch.uint8 and rank.device == revisit.device == torch.device(DEV)
    assert np.array_equal(rank.cpu().numpy(), want[0]) and np.array_equal(revisit.cpu().numpy(), want[1])


@pytest.mark.parametrize("k", bc.KS)
@pytest.mark.parametrize("order", bc.ORDERS)
@pytest.mark.parametrize("name", sorted(bc.CASES))
def test_device_lists_equal_the_host_form(fitted, name, order, k):
    ids = fitted(name).recommend(bc.case(name).samples, k, order)
    want = bc.host_lists(name, order, k)
    assert ids.dtype == torch.int32 and ids.shape == want.shape and ids.device == torch.device(DEV)
    assert np.array_equal(ids.cpu().numpy(), want)


@pytest.mark.parametrize("name", sorted(bc.CASES))
def test_device_fitted_tables_equal_the_cpu_fitted_ones(fitted, name):
    c = bc.case(name)
    dev, cpu = fitted(name), baseline.MarkovBaseline.fit(c.ds, c.train, device="cpu")
    assert (dev.P, dev.U) == (cpu.P, cpu.U) and dev.device == torch.device(DEV)
    pairs = [(getattr(dev, f), getattr(cpu, f)) for f in ("ukey", "uval", "pop", "pop_rank", "pop_order")]
    pairs += [(getattr(dev.graph, f), getattr(cpu.graph, f)) for f in ("rowptr", "col", "val")]
    for x, y in pairs:
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.cpu(), y)


def _assert_evaluates_to(mb, samples, order, host_rank, host_revisit):
    """mb.evaluate against the same f64 sums over the host form's ranks (CPU torch: the sums may differ in their last bits)."""
    rank, revisit = torch.from_numpy(host_rank), torch.from_numpy(host_revisit)
    want = baseline._metrics_of(rank)
    want["new"], want["revisit"] = baseline._metrics_of(rank, revisit == 0), baseline._metrics_of(rank, revisit != 0)
    got = mb.evaluate(samples, order, split_revisits=True)
    assert set(got) == set(want) and want["n"] > 0 and "new" not in mb.evaluate(samples, order)
    for g, w in ((got, want), (got["new"], want["new"]), (got["revisit"], want["revisit"])):
        assert set(g) - {"new", "revisit"} == set(w) - {"new", "revisit"} and g["n"] == w["n"]
        for key in w:
            if key not in ("new", "revisit", "n"):
                assert g[key] == pytest.approx(w[key], rel=1e-12, abs=0), key
                if key.startswith("acc"):
                    assert g[key] == w[key], key                                                   # (a count over n)


def test_evaluate_on_the_device_is_the_dict_of_the_host_ranks(fitted):
    for order in bc.ORDERS:
        _assert_evaluates_to(fitted("walks"), bc.case("walks").samples, order, *bc.host("walks", order))


def test_a_history_beyond_the_limit_is_refused_before_the_launch(fitted):
    ds = bc.dataset([(0, np.arange(4098) % 17 + 1)])
    with pytest.raises(ValueError, match=r"sample 0 \(session 0\) has a history of 4097 check-ins, the device forms take up to 4096"):
        fitted("walks").ranks(ds)


# ------------------------------------------------------------------------------------------------ golden G14's log
def test_the_test_prefixes_of_g14():
    res = data.sessionize(device=DEV, **cc.g14_log("sorted"))
    mb = data.MarkovBaseline.fit(res.dataset, res.train, device=DEV)
    samples = data.PrefixDataset(res.dataset, sessions=~res.train, device=DEV)
    assert len(samples) > int((~res.train).sum()) > 0
    for order in bc.ORDERS:
        want = baseline.ranks_host(res.dataset, res.train, samples, order)
        rank, revisit = mb.ranks(samples, order)
        assert np.array_equal(rank.cpu().numpy(), want[0]) and np.array_equal(revisit.cpu().numpy(), want[1])
        for k in (5, 20):
            assert np.array_equal(mb.recommend(samples, k, order).cpu().numpy(), baseline.topk_host(res.dataset, res.train, samples, order, k))
        _assert_evaluates_to(mb, samples, order, *want)


# ------------------------------------------------------------------------------------------------ the entry points themselves
SIZES = ("S", "M", "Q", "nnz", "nnzU", "U", "P", "order", "k")
RANKS_ARGS = ("seq", "offsets", "users", "S", "M", "session", "cut", "Q", "rowptr", "col", "val", "nnz", "ukey", "uval", "nnzU", "U",
              "pop_rank", "P", "order", "rank", "revisit", "status")
TOPK_ARGS = RANKS_ARGS[:17] + ("pop_order", "P", "order", "k", "ids", "status")
POISON = 77


def _direct(name="rows", order=0, k=20, **replace):
    """Device buffers and sizes of a direct call on a case, the tables fitted on the CPU: {argument: tensor or int}.  `replace`:
    numpy arrays that take the place of a buffer."""
    c = bc.case(name)
    mb = baseline.MarkovBaseline.fit(c.ds, c.train, device="cpu")
    base, session, cut = baseline._samples(c.samples, mb.P, "test")
    arrays = dict(seq=base.seq, offsets=base.offsets, users=base.users, session=session, cut=cut, rowptr=mb.graph.rowptr.numpy(),
                  col=mb.graph.col.numpy(), val=mb.graph.val.numpy(), ukey=mb.ukey.numpy(), uval=mb.uval.numpy(),
                  pop_rank=mb.pop_rank.numpy(), pop_order=mb.pop_order.numpy())
    arrays.update(replace)
    t = {key: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for key, v in arrays.items()}
    Q = len(arrays["session"])
    t.update(S=len(base), M=int(base.seq.shape[0]), Q=Q, nnz=len(arrays["col"]), nnzU=len(arrays["ukey"]), U=mb.U, P=mb.P, order=order, k=k)
    t["rank"] = torch.full((Q,), POISON, dtype=torch.int32, device=DEV)                            # (poisoned: every element is written)
    t["revisit"] = torch.full((Q,), POISON, dtype=torch.uint8, device=DEV)
    t["ids"] = torch.full((Q, k), POISON, dtype=torch.int32, device=DEV)
    t["status"] = torch.full((1,), POISON, dtype=torch.int32, device=DEV)
    return t


def _call(fn, t, **over):
    args = []
    for a in (RANKS_ARGS if fn == "mobgt_baseline_ranks" else TOPK_ARGS):
        v = over.get(a, t[a])
        args.append(v if a in SIZES or isinstance(v, ctypes.c_void_p) else ctypes.c_void_p(v.data_ptr()))
    rc = getattr(_baseline.LIBRARY.lib(), fn)(*args, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


OUTPUTS = ("rank", "revisit", "ids", "status")


@pytest.mark.parametrize("fn", ("mobgt_baseline_ranks", "mobgt_baseline_topk"))
def test_return_codes_with_nothing_launched(fn):
    t = _direct()
    before = {key: t[key].clone() for key in OUTPUTS}
    bad = [("Q", -1), ("Q", 2 ** 31), ("S", -1), ("S", 2 ** 31), ("M", -1), ("M", 2 ** 31), ("nnz", -1), ("nnz", 2 ** 31), ("nnzU", -1),
           ("nnzU", 2 ** 31), ("P", 0), ("P", 2 ** 31), ("U", -1), ("U", 2 ** 63 // (t["P"] * t["P"]) + 1), ("order", -1), ("order", 3)]
    if fn == "mobgt_baseline_topk":
        bad += [("k", 0), ("k", 65)]
    for key, value in bad:
        assert _call(fn, t, **{key: value}) == _baseline.EBADDIM, (key, value)
    mine = ("rank", "revisit") if fn == "mobgt_baseline_ranks" else ("ids", "pop_order")
    pointers = ("seq", "offsets", "users", "session", "cut", "rowptr", "col", "val", "ukey", "uval", "pop_rank", "status") + mine
    for key in pointers:
        assert _call(fn, t, **{key: ctypes.c_void_p(0)}) == _baseline.EALIGN, key                 # a null buffer
        if key != "revisit":                                                                       # (bytes: any address is aligned)
            off = 4 if t[key].dtype == torch.int64 else 2
            assert _call(fn, t, **{key: ctypes.c_void_p(t[key].data_ptr() + off)}) == _baseline.EALIGN, key
    assert all(torch.equal(t[key], before[key]) for key in OUTPUTS)                                # nothing was launched
    names = RANKS_ARGS if fn == "mobgt_baseline_ranks" else TOPK_ARGS
    with pytest.raises(_baseline.MobgtBaselineError, match="MOBGT_BASELINE_EBADDIM") as e:
        _baseline.launch(fn, *(-1 if a == "Q" else 1 if a in SIZES else None for a in names), None)
    assert e.value.code == _baseline.EBADDIM
    assert _call(fn, t) == 0 and int(t["status"][0]) == 0                                          # and the same buffers are good


def _assert_good(t, name, order, k, but=(), other=()):
    """The outputs of a direct ranks + topk call pair equal the host form's, except at the samples `but`, which hold the refusal,
    and at the samples `other`, which were given other tables than the host form and are not looked at."""
    want_rank, want_revisit = bc.host(name, bc.ORDERS[order])
    want_ids = bc.host_lists(name, bc.ORDERS[order], k)
    q = np.arange(len(want_rank))
    refused = np.isin(q, but)
    ok = ~refused & ~np.isin(q, other)
    rank, revisit, ids = (t[key].cpu().numpy() for key in ("rank", "revisit", "ids"))
    assert np.array_equal(rank[ok], want_rank[ok]) and np.array_equal(revisit[ok], want_revisit[ok]) and np.array_equal(ids[ok], want_ids[ok])
    assert np.all(rank[refused] == -1) and np.all(revisit[refused] == 0) and np.all(ids[refused] == -1)


@pytest.mark.parametrize("order", (0, 1, 2))
def test_every_output_element_is_written(order):
    for name, k in (("rows", 20), ("p1", 64), ("empty", 1), ("untrained", 20)):
        t = _direct(name, order, k)
        assert _call("mobgt_baseline_ranks", t) == 0 and int(t["status"][0]) == 0
        t["status"].fill_(POISON)
        assert _call("mobgt_baseline_topk", t) == 0 and int(t["status"][0]) == 0
        _assert_good(t, name, order, k)
    t = _direct("untrained", order)                                                                 # nnz = nnzU = 0: null tables
    null = {key: ctypes.c_void_p(0) for key in ("col", "val", "ukey", "uval")}
    assert _call("mobgt_baseline_ranks", t, **null) == 0 and _call("mobgt_baseline_topk", t, **null) == 0 and int(t["status"][0]) == 0
    _assert_good(t, "untrained", order, 20)


def _refused(replace, hit, other=(), name="rows", order=0, k=20):
    assert len(hit) > 0
    t = _direct(name, order, k, **replace)
    assert _call("mobgt_baseline_ranks", t) == 0 and int(t["status"][0]) == _baseline.SBADINDEX
    t["status"].fill_(POISON)
    assert _call("mobgt_baseline_topk", t) == 0 and int(t["status"][0]) == _baseline.SBADINDEX
    _assert_good(t, name, order, k, but=hit, other=other)


def test_the_status_word():
    """Every index a sample reads through is checked before it is used: the sample that fails keeps rank -1, revisit 0 and a list of
    -1, SBADINDEX is raised, and its neighbours are right.  None of these inputs is read out of bounds."""
    c = bc.case("rows")
    base, session, cut = baseline._samples(c.samples, 2 ** 31 - 1, "test")
    L = (np.diff(base.offsets) - 1)[session]
    S, Q = len(base), len(session)

    def with_(array, q, value):
        out = array.copy()
        out[q] = value
        return out
    for q, value in ((0, -1), (5, S), (Q - 1, 2 ** 31 - 1)):                                       # a session out of range
        _refused(dict(session=with_(session, q, value)), [q])
    for q in (0, 6, Q - 1):
        _refused(dict(cut=with_(cut, q, 0)), [q])                                                   # a cut of 0
        _refused(dict(cut=with_(cut, q, L[q] + 1)), [q])                                            # a cut of L + 1
        _refused(dict(cut=with_(cut, q, -3)), [q])
    # a descending rowptr pair, and one beyond nnz: the samples whose previous POI is that row's
    _, a, t = bc.previous_and_target(c.samples)
    mb = baseline.MarkovBaseline.fit(c.ds, c.train, device="cpu")
    rowptr = mb.graph.rowptr.numpy()
    for hub in (3, 5):                                                                              # rowptr[hub] closes row hub and opens row hub + 1
        # descending for row hub; row hub + 1 then starts early, inside the entries: in range, but not the host form's row
        _refused(dict(rowptr=with_(rowptr, hub, rowptr[hub - 1] - 1)), np.nonzero(a == hub)[0], other=np.nonzero(a == hub + 1)[0])
    _refused(dict(rowptr=with_(rowptr, 5, mb.graph.nnz + 1)), np.nonzero((a == 5) | (a == 6))[0])   # beyond nnz, and descending for row 6
    _refused(dict(rowptr=with_(rowptr, mb.P, mb.graph.nnz + 7)), np.nonzero(a == mb.P)[0])          # the last entry, beyond nnz
    _refused(dict(rowptr=with_(rowptr, 0, -1)), np.nonzero(a == 1)[0])
    # a target or a previous POI outside 1 .. P (behind the host's validation: straight in seq)
    q = 7
    row = int(base.offsets[session[q]] + cut[q])
    for value in (0, mb.P + 1, -5):
        seq = base.seq.copy()
        seq[row, 0] = value
        hit = [i for i in range(Q) if int(base.offsets[session[i]] + cut[i]) in (row, row + 1)]   # as a target, and as the next sample's previous POI
        _refused(dict(seq=seq), hit)
    # offsets that run beyond the check-ins
    _refused(dict(offsets=with_(base.offsets, S, base.seq.shape[0] + 3)), np.nonzero(session == S - 1)[0])
    # a history beyond the limit: its own bit
    long = bc.dataset([(0, np.arange(4100) % 30 + 1), (1, [1, 2, 3])])
    t = _direct("walks", session=np.array([0, 0, 1], dtype=np.int32), cut=np.array([4097, 4096, 2], dtype=np.int32), seq=long.seq,
                offsets=long.offsets, users=long.users)
    t["S"], t["M"] = 2, int(long.seq.shape[0])
    assert _call("mobgt_baseline_ranks", t) == 0 and int(t["status"][0]) == _baseline.STOOLONG
    rank = t["rank"].cpu().numpy()
    assert rank[0] == -1 and rank[1] >= 0 and rank[2] >= 0 and t["revisit"].cpu().tolist() == [0, 1, 0]
    assert _call("mobgt_baseline_topk", t) == 0 and int(t["status"][0]) == _baseline.STOOLONG
    ids = t["ids"].cpu().numpy()
    assert np.all(ids[0] == -1) and np.all(ids[1:] >= 1)


def test_a_col_beyond_the_pois_is_skipped_and_flagged():
    """An entry of col >= P (or negative) is never an index into pop_rank: it is skipped, SBADINDEX is raised, and every sample
    whose row does not hold it is right.  The samples of that row count the other entries."""
    c = bc.case("rows")
    mb = baseline.MarkovBaseline.fit(c.ds, c.train, device="cpu")
    _, a, t = bc.previous_and_target(c.samples)
    rowptr, col = mb.graph.rowptr.numpy(), mb.graph.col.numpy()
    for hub, value in ((6, mb.P), (2, 2 ** 31 - 1), (5, -1)):                                      # rows of 200, 63 and 129 entries
        e = int(rowptr[hub]) - 1                                                                   # the row's last entry
        bad = col.copy()
        bad[e] = value
        hit = np.nonzero(a == hub)[0]
        tt = _direct("rows", 0, 20, col=bad)
        assert _call("mobgt_baseline_ranks", tt) == 0 and int(tt["status"][0]) == _baseline.SBADINDEX
        tt["status"].fill_(POISON)
        assert _call("mobgt_baseline_topk", tt) == 0 and int(tt["status"][0]) == _baseline.SBADINDEX
        ok = ~np.isin(np.arange(len(a)), hit)
        rank, ids = tt["rank"].cpu().numpy(), tt["ids"].cpu().numpy()
        assert np.array_equal(rank[ok], bc.host("rows", "user")[0][ok]) and np.array_equal(ids[ok], bc.host_lists("rows", "user", 20)[ok])
        assert np.array_equal(tt["revisit"].cpu().numpy(), bc.host("rows", "user")[1])
        assert len(hit) >= 3 and np.all(rank[hit] >= 0) and np.all(rank[hit] < mb.P) and np.all(ids[hit] >= 1)
    # pop_order is a value, never an index: an entry outside [0, P) is left out of the lists and flagged
    assert bc.case("untrained").ds.seq[:, 0].max() == 5
    tt = _direct("untrained", 2, 5, pop_order=np.array([5, 1, 2, 3, 4], dtype=np.int32))            # (POIs 1 .. 5 are 0 .. 4 here)
    assert _call("mobgt_baseline_topk", tt) == 0 and int(tt["status"][0]) == _baseline.SBADINDEX
    assert tt["Q"] == 5 and tt["ids"].cpu().tolist() == [[2, 3, 4, 5, -1]] * 5


def test_the_public_call_reports_a_status(monkeypatch, fitted):
    """The same corruption injected behind the host's validation is a ValueError that names the first sample skipped; the next
    call on the same device is right."""
    c, mb = bc.case("rows"), fitted("rows")
    launch = _baseline.launch

    def corrupt(fn, seq, offsets, users, S, M, session, cut, Q, *rest):
        bad = torch.zeros(Q, dtype=torch.int32, device=DEV)
        bad[:] = torch.from_numpy(np.ascontiguousarray(c.samples.cut)).to(DEV)
        bad[9] = 0
        torch.cuda.synchronize()
        keep.append(bad)
        return launch(fn, seq, offsets, users, S, M, session, ctypes.c_void_p(bad.data_ptr()), Q, *rest)
    keep = []
    monkeypatch.setattr(_baseline, "launch", corrupt)
    with pytest.raises(ValueError, match=rf"MarkovBaseline.ranks: .*\(status {_baseline.SBADINDEX}\), the first of them sample 9:"):
        mb.ranks(c.samples)
    with pytest.raises(ValueError, match=rf"MarkovBaseline.recommend: .*\(status {_baseline.SBADINDEX}\), the first of them sample 9:"):
        mb.recommend(c.samples, 5)
    monkeypatch.undo()
    assert np.array_equal(mb.ranks(c.samples)[0].cpu().numpy(), bc.host("rows", "user")[0])
