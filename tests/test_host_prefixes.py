"""Every prefix of a session as a sample, on the host: `data.prefix_stats_host` (the rule's plain loop, the reference of the kernels
in csrc_prefixes/prefixes.hip) against brute force on the crafted cases of prefixes_cases.py and on golden G12's sessions,
`data.PrefixDataset(device="cpu")`, what the rest of the data path makes of one, and the ninth library's header.  No GPU."""
import numpy as np
import pytest

import prefixes_cases as pc
from mobgt_amd import _prefixes, data, prefixes


@pytest.mark.parametrize("h", pc.MIN_HISTORIES)
@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_host_form_equals_brute_force(name, h):
    pc.assert_same(data.prefix_stats_host(pc.case(name), h), pc.expected(name, h))
    pc.assert_same(data.prefix_stats(pc.case(name), h, device="cpu"), pc.expected(name, h))       # (without a GPU: the host form)


@pytest.mark.parametrize("sel", sorted(pc.SELECTIONS))
@pytest.mark.parametrize("h", (1, 64))
def test_host_form_over_chosen_sessions(sel, h):
    ds = pc.case("lengths")
    sessions = pc.SELECTIONS[sel](len(ds))
    got = data.prefix_stats_host(ds, h, sessions)
    pc.assert_same(got, pc.expected("lengths", h, sessions))
    assert (len(got.session) == 0) == (sel == "none") and np.all(np.diff(got.session) >= 0)


def test_the_cases_are_what_they_claim():
    L = lambda name: (np.diff(pc.case(name).offsets) - 1).tolist()
    assert set(L("lengths")) == {1, 2, 15, 16, 63, 64, 65, 127, 128, 129} and L("lengths")[:4] == [1, 64, 2, 129]
    assert L("long_4096").count(4096) == 1 and max(L("long_4096")) == prefixes.DEVICE_MAX_L == _prefixes.MAX_L
    p = pc.case("long_4096")[1].checkins[:, 0]
    assert np.nonzero(p == 9001)[0].tolist() == [63, 64] and np.nonzero(p == 9002)[0].tolist() == [0, 4095]
    s = pc.host("same_poi")
    assert np.all(s.n == 1) and np.array_equal(s.mult, s.cut)
    d = pc.host("distinct")
    assert np.all(d.mult == 1) and np.array_equal(d.n, d.cut)
    a = pc.host("alternating")
    assert np.array_equal(a.n, np.minimum(a.cut, 2)) and np.array_equal(a.mult, (a.cut + 1) // 2)
    st = pc.host("straddle")
    first = st.session == 0
    assert np.array_equal(st.n[first], np.where(st.cut[first] <= 64, st.cut[first], st.cut[first] - 1))
    assert np.array_equal(st.mult[first], np.where(st.cut[first] <= 64, 1, 2))
    assert {pc.INT32_MIN, -1, 0, pc.INT32_MAX} == set(pc.case("extreme_ids").seq[:, 0].tolist())
    assert len(pc.case("empty")) == 0 and len(pc.case("one")) == 1 and len(pc.case("many")) == 257
    # min_history: sessions that yield nothing, a session that yields exactly one sample, the first stored row on either side of 64
    per = lambda h: np.bincount(pc.host("lengths", h).session, minlength=22).tolist()
    assert per(64)[:4] == [0, 1, 0, 66] and per(65)[:4] == [0, 0, 0, 65] and per(3)[:3] == [0, 62, 0]
    assert pc.host("lengths", 64).cut.min() == 64 and pc.host("lengths", 65).cut.min() == 65


@pytest.mark.parametrize("name", ["lengths", "g12", "long_4096"])
def test_the_last_cut_is_the_base_datasets_sample(name):
    ds, st = pc.case(name), pc.host(name)
    last = st.cut == (np.diff(ds.offsets) - 1)[st.session]
    assert int(last.sum()) == len(ds) and np.array_equal(st.session[last], np.arange(len(ds)))
    assert np.array_equal(st.n[last], ds.n) and np.array_equal(st.mult[last], ds.mult)


def test_prefix_dataset_on_the_host():
    ds = pc.case("g12")
    pds = data.PrefixDataset(ds, device="cpu")
    want = pc.expected("g12")
    assert pds.base is ds and pds.min_history == 1 and len(pds) == len(want.session) == int((np.diff(ds.offsets) - 1).sum())
    pc.assert_same(data.PrefixStats(pds.session, pds.cut, pds.n, pds.mult), want)
    assert pds.users.dtype == np.int64 and np.array_equal(pds.users, ds.users[pds.session])
    assert pds.last.dtype == np.bool_ and np.array_equal(pds.last, pds.cut == (np.diff(ds.offsets) - 1)[pds.session])
    assert int(pds.last.sum()) == len(ds) and pds.max_n == int(pds.n.max()) == ds.max_n
    for i in range(len(pds)):
        r, full = pds[i], ds[int(pds.session[i])]
        c = int(pds.cut[i])
        assert isinstance(r, data.SessionRecord) and np.shares_memory(r.checkins, pds.base.seq)
        assert r.checkins.shape == (c + 1, 3) and np.array_equal(r.checkins, full.checkins[:c + 1])
        assert np.array_equal(r.checkins[-1], full.checkins[c])                               # the last row is the target row
        assert (r.user, r.n, r.mult) == (full.user, int(pds.n[i]), int(pds.mult[i]))
        b = data._as_record((full.user, full.checkins[:c + 1]))
        assert (r.user, r.n, r.mult) == (b.user, b.n, b.mult)
    assert pds[-1].checkins.shape == pds[len(pds) - 1].checkins.shape and np.array_equal(pds[-1].checkins, ds[-1].checkins)
    for bad in (len(pds), -len(pds) - 1):
        with pytest.raises(IndexError):
            pds[bad]
    # min_history and sessions=
    train = np.arange(len(ds)) % 3 != 0
    p3 = data.PrefixDataset(ds, min_history=3, sessions=train, device="cpu")
    pc.assert_same(data.PrefixStats(p3.session, p3.cut, p3.n, p3.mult), pc.expected("g12", 3, train))
    assert p3.min_history == 3 and p3.cut.min() == 3 and not np.isin(p3.session, np.nonzero(~train)[0]).any()
    by_index = data.PrefixDataset(ds, min_history=3, sessions=np.nonzero(train)[0][::-1], device="cpu")
    assert np.array_equal(by_index.session, p3.session) and np.array_equal(by_index.cut, p3.cut)


def test_an_empty_prefix_dataset_is_valid():
    for pds in (data.PrefixDataset(pc.case("empty"), device="cpu"), data.PrefixDataset(pc.case("one"), min_history=4, device="cpu"),
                data.PrefixDataset(pc.case("lengths"), sessions=np.zeros(22, dtype=bool), device="cpu")):
        assert len(pds) == 0 and pds.max_n == 0 and pds.last.shape == (0,) and pds.users.shape == (0,)
        assert all(getattr(pds, f).dtype == np.int32 and getattr(pds, f).shape == (0,) for f in ("session", "cut", "n", "mult"))
        with pytest.raises(IndexError):
            pds[0]
        assert data.SessionCollator.lengths_of(pds) == [] and data.sessions_to_trajectories(pds) == []
    assert len(data.PrefixDataset(pc.case("one"), min_history=3, device="cpu")) == 1


def test_every_refusal():
    ds = pc.case("lengths")
    S = len(ds)
    sessions = [(r.user, r.checkins) for r in (ds[i] for i in range(3))]
    for make in (data.PrefixDataset, data.prefix_stats, lambda d, **k: data.prefix_stats_host(d, **{a: b for a, b in k.items() if a != "device"})):
        with pytest.raises(TypeError, match="SessionDataset"):
            make(sessions, device="cpu")
        with pytest.raises(TypeError, match=r"\.base"):
            make(data.PrefixDataset(ds, device="cpu"), device="cpu")
        for h in (0, -1, 1.0, 2.5, True, None, "3"):
            with pytest.raises(ValueError, match="min_history"):
                make(ds, min_history=h, device="cpu")
        with pytest.raises(ValueError, match=rf"mask of {S - 1} flags for {S} sessions"):
            make(ds, sessions=np.ones(S - 1, dtype=bool), device="cpu")
        for bad in (S, -1):
            with pytest.raises(ValueError, match=rf"session index {bad} is not in 0 \.\. {S - 1}"):
                make(ds, sessions=[0, bad, 2], device="cpu")
        with pytest.raises(ValueError, match="session index 4 is given more than once"):
            make(ds, sessions=[4, 1, 4], device="cpu")
        with pytest.raises(ValueError, match="boolean mask"):
            make(ds, sessions=np.array([0.0, 1.0]), device="cpu")
    assert len(data.PrefixDataset(ds, min_history=np.int64(2), sessions=np.array([], dtype=np.int64), device="cpu")) == 0


def test_trajectories_of_prefixes_equal_those_of_truncated_sessions():
    pds = data.PrefixDataset(pc.case("g12"), device="cpu")
    got, want = data.sessions_to_trajectories(pds), data.sessions_to_trajectories(pc.truncated(pds))
    assert len(got) == len(want) == len(pds)
    for a, b in zip(got, want):
        assert a.keys() == b.keys()
        for k in a:
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k


def test_lengths_come_from_n_without_building_a_record(monkeypatch):
    pds = data.PrefixDataset(pc.case("lengths"), min_history=3, device="cpu")
    want = [int(v) for v in pds.n]

    def refuse(self, i):
        raise AssertionError("lengths_of built a record")
    monkeypatch.setattr(data.PrefixDataset, "__getitem__", refuse)
    assert data.SessionCollator.lengths_of(pds) == want and len(want) == len(pds)


def test_the_universe_is_not_counted_over_prefixes():
    pds = data.PrefixDataset(pc.case("g12"), device="cpu")
    train = np.ones(len(pds), dtype=bool)
    for count in (data.universe_counts_host, data.universe_counts, lambda d, t: data.build_universe(d, t, np.zeros((4, 2)))):
        with pytest.raises(TypeError, match=r"pds\.base"):
            count(pds, train)


def test_the_header_is_readable_without_the_built_library():
    sig = _prefixes.SIGNATURES
    assert list(sig) == ["mobgt_prefixes_abi_version", "mobgt_prefixes_stats"] and _prefixes.ABI_VERSION == 1
    res, args = sig["mobgt_prefixes_stats"]
    assert len(args) == 14 and [a.__name__ for a in args[4:8]] == ["c_long"] * 4 and all(a.__name__ == "c_void_p" for a in args[:4] + args[8:])
    assert (_prefixes.MAX_L, _prefixes.WAVE, _prefixes.EBADDIM, _prefixes.EALIGN, _prefixes.SBADINDEX) == (4096, 64, -1, -2, 1)
    from mobgt_amd import _lib_data, _native
    assert _prefixes.MAX_L == _lib_data.MAX_LP and len(_native._MODULES) == 5 and "_prefixes" not in _native._MODULES
