"""Sessions from a raw check-in log on the host: `data.sessionize_host` (the reference of the kernels in
csrc_checkins/sessions.hip) against the reference's own run (golden G14, the time-sorted and the shuffled copy), what the crafted
cases are for, `SessionDataset.from_packed`, the scan of composed maps the cut kernel runs, everything that is refused before a
launch, and the eighth library's header.  No GPU."""
import os
import types

import numpy as np
import pytest

import checkins_cases as cc
from mobgt_amd import _cabi, _checkins, _native, _pairbins, _universe, checkins, data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("copy", ["sorted", "shuffled"])
def test_host_form_equals_the_reference_run_g14(copy):
    z, res = cc.g14(), cc.host("g14_" + copy)
    ds = res.dataset
    assert ds.seq.dtype == np.int32 and np.array_equal(ds.seq, z[copy + "_seq"])
    assert np.array_equal(ds.offsets, z[copy + "_offsets"]) and np.array_equal(ds.users, z[copy + "_users"])
    assert res.train.dtype == np.bool_ and np.array_equal(res.train, z[copy + "_train"])
    assert np.array_equal(res.user_ids, z[copy + "_uid_order"]) and np.array_equal(res.poi_ids, z[copy + "_vid_order"])
    assert np.array_equal(res.cat_ids, z[copy + "_cat_order"])
    assert res.coords_deg.dtype == np.float64 and np.array_equal(res.coords_deg, z[copy + "_coords"])
    log = cc.g14_log(copy)
    assert np.array_equal(res.poi_ids[ds.seq[:, 0] - 1], log["poi"][res.kept])                     # kept: the log positions
    assert np.array_equal(ds.seq[:, 1], log["t"][res.kept] % 86400 // 1800)
    assert np.array_equal(res.user_ids[np.repeat(ds.users, np.diff(ds.offsets))], log["user"][res.kept])
    assert (res.cat_ids[ds.seq[:, 2] - 1] != log["cat"][res.kept]).any()                            # the POI's category, not the row's
    assert set(res.user_ids) <= set(res.users_order) and "once" in res.users_order and "tiny" not in res.users_order


def test_the_two_copies_differ_and_hold_what_g14_is_for():
    a, b = cc.host("g14_sorted"), cc.host("g14_shuffled")
    assert len(a.dataset) > len(b.dataset) > 20 and (np.diff(cc.g14_log("shuffled")["t"]) < 0).any()
    s = cc.sessions_of(a)
    assert s["full"] == [11, 6] and s["edge"] == [6, 6] and "once" not in s and "tiny" not in s
    assert max(max(v) for v in s.values()) == 11 and min(min(v) for v in s.values()) == 5
    counts = {u: int((cc.g14_log("sorted")["user"] == u).sum()) for u in a.user_ids}
    assert len(set(counts.values())) < len(counts)                     # ties in the user count


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_dataset_equals_the_constructor_and_feeds_the_pipeline(name):
    res = cc.host(name)
    ds = res.dataset
    old = data.SessionDataset([(int(u), ds.seq[a:b]) for u, a, b in zip(ds.users, ds.offsets[:-1], ds.offsets[1:])])
    for f in cc.FIELDS:
        assert getattr(old, f).dtype == getattr(ds, f).dtype and np.array_equal(getattr(old, f), getattr(ds, f)), f
    assert len(ds) == len(res.train) and ds.max_n == (int(ds.n.max()) if len(ds) else 0)
    trajs = data.sessions_to_trajectories(ds)
    assert len(trajs) == len(ds) and all(len(t["node_name"]) == n for t, n in zip(trajs, ds.n))
    if len(ds):
        assert ds[0].n == ds.n[0] and ds[len(ds) - 1].checkins.shape == (ds.offsets[-1] - ds.offsets[-2], 3)
        c = data.universe_counts_host(ds, train=res.train)             # (no two-category error: a row carries its POI's category)
        assert c.P == len(res.poi_ids) and c.n_cat <= len(res.cat_ids) and int(c.checkin_cnt.sum()) == len(ds.seq)
        users = ds.users
        assert users[0] == 0 and set(np.diff(users)) <= {0, 1} and users[-1] == len(res.user_ids) - 1
        for u in range(len(res.user_ids)):                             # the first floor(0.8 n) sessions of every user are train
            flags = res.train[users == u]
            k = int(np.floor(cc.case(name)[1].get("train_split", 0.8) * len(flags)))
            assert flags[:k].all() and not flags[k:].any() and k >= 1


def test_the_cases_hold_what_they_are_for():
    s = cc.sessions_of(cc.host("chunk_edges"))
    cols, _ = cc.case("chunk_edges")
    remaining = {u: int(((cols["user"] == u) & (cols["poi"] < 100)).sum()) for u in set(cols["user"])}
    assert sorted(remaining.values()) == [0, 1, 63, 64, 65, 128, 129] and "u0" not in s and "u1" not in s and "u129" in s
    assert "gone" not in cc.sessions_of(cc.host("all_filtered")) and "gone" in cc.host("all_filtered").users_order
    for m in (1, 10, 15):
        lens = [n for v in cc.sessions_of(cc.host(f"session_max_{m}")).values() for n in v]
        assert max(lens) == m + 1 and min(lens) >= 2
    assert cc.sessions_of(cc.host("under_min_gap_after_full")) == {"a": [11, 8], "b": [11, 8]}
    # session_max = 1: the 11 records pair up and leave a session of one, which is not full: the whole 60 s run is dropped
    assert cc.sessions_of(cc.host("under_min_gap_session_max_1")) == {"a": [2] * 5 + [2] * 4, "b": [2] * 5 + [2] * 4}
    t = cc.sessions_of(cc.host("thresholds"))
    assert t["g86400"] == [4, 5] and t["g86399"] == [9] and t["g86401"] == [4, 5] and t["g600"] == [9] and t["g599"] == [8] and t["g601"] == [9]
    e = cc.sessions_of(cc.host("trace_and_visit_edges"))
    assert "nine" not in e and "ten" in e and sum(e["big"]) == 31
    logged = cc.case("ties")[0]["user"].tolist()
    want = sorted("abcdef", key=lambda u: (-logged.count(u), logged.index(u)))                    # count descending, then first seen
    assert list(cc.host("ties").user_ids) == want and want[0] == "f" and set(want[1:3]) == {"a", "b"} and want[1:] != sorted(want[1:])
    sp = cc.host("split_counts")
    assert {str(u): int(sp.train[sp.dataset.users == k].sum()) for k, u in enumerate(sp.user_ids)} == {"s15": 12, "s10": 8, "s5": 4, "s3": 2, "s2": 1}
    mc = cc.host("multi_category")
    assert len(mc.cat_ids) > len(set(mc.dataset.seq[:, 2]))            # own categories are numbered, POI categories are carried
    for name in ("empty_result", "no_records"):
        r = cc.host(name)
        assert len(r.dataset) == 0 and r.dataset.seq.shape == (0, 3) and r.dataset.offsets.tolist() == [0] and r.train.shape == (0,)
        assert r.kept.shape == (0,) and r.coords_deg is None and len(r.poi_ids) == 0


def _cut_by_scan(kinds, session_max, chunk):
    """The cut kernel's formulation in Python integers: every record a map of the session length as 16 nibbles, an inclusive
    scan of composed maps per chunk, applied to the carried state -> the actions (2 start, 1 append, 0 drop)."""
    ident = 0xFEDCBA9876543210
    append = sum((k + 1) << 4 * k for k in range(session_max))
    skip = sum(k << 4 * k for k in range(session_max))
    then = lambda f, g: sum(((g >> 4 * ((f >> 4 * k) & 15)) & 15) << 4 * k for k in range(16))
    apply = lambda f, s: ((f >> 4 * (s - 1)) & 15) + 1
    out, carry = [], 1
    for base in range(0, len(kinds), chunk):
        maps = [{0: 0, 1: append, 2: skip}[k] for k in kinds[base:base + chunk]]
        maps += [ident] * (chunk - len(maps))
        f = list(maps)
        d = 1
        while d < chunk:                                               # Hillis-Steele, as the wave's shuffles run it
            f = [then(f[i - d], f[i]) if i >= d else f[i] for i in range(chunk)]
            d *= 2
        for i, k in enumerate(kinds[base:base + chunk]):
            s = apply(f[i - 1] if i else ident, carry)
            out.append(2 if k == 0 or s > session_max else 1 if k == 1 else 0)
        carry = apply(f[-1], carry)
    return out


@pytest.mark.parametrize("session_max", [1, 2, 3, 10, 15])
def test_the_scan_of_composed_maps_equals_the_sequential_cut(session_max):
    rng = np.random.RandomState(session_max)
    for n in (1, 2, 63, 64, 65, 128, 129, 300):
        kinds = [0] + rng.choice(3, size=n - 1, p=[0.1, 0.6, 0.3]).tolist()
        want, s = [], 0
        for k in kinds:
            if k == 0 or s > session_max:
                want.append(2)
                s = 1
            elif k == 1:
                want.append(1)
                s += 1
            else:
                want.append(0)
        assert _cut_by_scan(kinds, session_max, 64) == want


def test_from_packed_validates_vectorised():
    ds = cc.host("ties").dataset
    again = data.SessionDataset.from_packed(ds.seq, ds.offsets, ds.users, ds.n, ds.mult)
    assert again.seq is ds.seq or np.shares_memory(again.seq, ds.seq)  # stored as they come
    bad = lambda **kw: data.SessionDataset.from_packed(**dict(dict(seq=ds.seq, offsets=ds.offsets, users=ds.users, n=ds.n, mult=ds.mult), **kw))
    with pytest.raises(ValueError, match=r"\[M, 3\]"):
        bad(seq=ds.seq[:, :2])
    with pytest.raises(ValueError, match="offsets run from"):
        bad(offsets=ds.offsets + 1)
    with pytest.raises(ValueError, match="need offsets"):
        bad(offsets=ds.offsets[:-1])
    short = ds.offsets.copy()
    short[1] = 1
    with pytest.raises(ValueError, match=r"session 0 has 1 check-in\(s\)"):
        bad(offsets=short)
    with pytest.raises(ValueError, match="session 0: n = 0"):
        bad(n=ds.n * 0)
    with pytest.raises(ValueError, match="must be integers"):
        bad(seq=ds.seq.astype(np.float64))
    with pytest.raises(ValueError, match="does not fit int32"):
        bad(seq=ds.seq.astype(np.int64) + 2 ** 40)


@pytest.mark.parametrize("form", [data.sessionize_host, lambda *a, **k: data.sessionize(*a, device="cuda", **k)], ids=["host", "device"])
def test_bad_input_is_refused_on_the_host(form, monkeypatch):
    """Both forms validate before anything else: the device form raises these without a GPU, without its library."""
    monkeypatch.setattr(_checkins.LIBRARY, "lib", lambda: pytest.fail("validation comes before the library is loaded"))
    u, t = np.arange(12) % 2, cc.steps(12)
    with pytest.raises(ValueError, match="of equal length"):
        form(u, u[:-1], u, t)
    with pytest.raises(ValueError, match="of equal length"):
        form(u, u, u, t, lat=np.zeros(3), lon=np.zeros(3))
    with pytest.raises(ValueError, match="lat and lon come together"):
        form(u, u, u, t, lat=np.zeros(12))
    huge = np.broadcast_to(np.int64(1), (2 ** 31,))                    # a view of one element, no memory behind it
    with pytest.raises(ValueError, match=r"N < 2\*\*31"):
        form(huge, huge, huge, huge)
    with pytest.raises(ValueError, match="t must be integer seconds"):
        form(u, u, u, t.astype(np.float64))
    with pytest.raises(ValueError, match="session_min = 1"):
        form(u, u, u, t, session_min=1)
    for name in ("trace_min", "global_visit", "hour_gap", "min_gap", "sessions_min"):
        with pytest.raises(ValueError, match=f"{name} = -1 is negative"):
            form(u, u, u, t, **{name: -1})
    with pytest.raises(ValueError, match="hour_gap must be an integer"):
        form(u, u, u, t, hour_gap=1.5)
    for split in (0.0, 1.5, -0.2):
        with pytest.raises(ValueError, match="train_split"):
            form(u, u, u, t, train_split=split)
    with pytest.raises(ValueError, match="session_max = 0"):
        form(u, u, u, t, session_max=0)
    with pytest.raises(ValueError, match=r"dense = \(U0, P0, C0\)"):
        form(u, u, u, t, dense=(2, 0, 2))
    with pytest.raises(ValueError, match="integer ids"):
        form(u.astype(str), u, u, t, dense=(2, 2, 2))
    with pytest.raises(TypeError, match="unknown parameter"):
        form(u, u, u, t, session_maxx=3)


def test_session_max_limit_is_the_device_forms_and_host_names_bad_ids_and_zero_splits(monkeypatch):
    monkeypatch.setattr(_checkins.LIBRARY, "lib", lambda: pytest.fail("validation comes before the library is loaded"))
    u, t = np.zeros(40, dtype=np.int64), cc.steps(40)
    with pytest.raises(ValueError, match=r"session_max = 16 is not in 1 \.\. 15"):
        data.sessionize(u, u, u, t, session_max=16, device="cuda")
    r = data.sessionize_host(u, u, u, t, session_max=16, **cc.SMALL)
    assert np.diff(r.dataset.offsets).tolist() == [17, 17, 6] and checkins.DEVICE_SESSION_MAX == _checkins.MAX_SESSION_MAX == 15
    with pytest.raises(ValueError, match=r"record 3 has \(user, poi, cat\) = \(1, 9, 1\)"):
        data.sessionize_host(u + 1, np.where(np.arange(40) == 3, 9, 1), u + 1, t, dense=(1, 8, 1), **cc.SMALL)
    with pytest.raises(ValueError, match=r"user 'solo' survives with 1 session\(s\)"):
        data.sessionize_host(["solo"] * 6, u[:6], u[:6], t[:6], **dict(cc.SMALL, train_split=0.8))
    assert data.sessionize(u, u, u, t, device="cpu", **cc.SMALL).dataset.seq.shape == (40, 3)      # without a GPU: the host form


def test_header_binds_and_the_library_stays_out_of_the_pinned_five():
    protos, consts = _cabi.load(os.path.join(ROOT, "include", "mobgt_checkins.h"))
    vp, ci, i64, f64 = _cabi.ctypes.c_void_p, _cabi.ctypes.c_int, _cabi.ctypes.c_int64, _cabi.ctypes.c_double
    assert list(protos) == ["mobgt_checkins_abi_version", "mobgt_checkins_count", "mobgt_checkins_keys", "mobgt_checkins_cut",
                            "mobgt_checkins_sessions", "mobgt_checkins_first", "mobgt_checkins_emit"]
    assert protos["mobgt_checkins_abi_version"] == (ci, [])
    assert protos["mobgt_checkins_count"] == (ci, [vp] * 3 + [i64] * 5 + [vp] * 6)
    assert protos["mobgt_checkins_keys"] == (ci, [vp] * 3 + [i64] * 4 + [vp, i64, vp, i64, vp, vp])
    assert protos["mobgt_checkins_cut"] == (ci, [vp, i64, vp, i64, i64, i64, i64, ci, vp, vp, vp, vp])
    assert protos["mobgt_checkins_sessions"] == (ci, [vp] * 4 + [i64] * 5 + [f64] + [vp] * 11)
    assert protos["mobgt_checkins_first"] == (ci, [vp] * 3 + [i64] * 2 + [vp] * 2 + [i64] * 3 + [vp] * 7)
    assert protos["mobgt_checkins_emit"] == (ci, [vp] * 5 + [i64] + [vp] * 5 + [i64] * 5 + [vp] * 4 + [i64] * 2 + [vp] * 4 + [i64] * 2 + [vp] * 11)
    assert protos == _checkins.SIGNATURES and consts["MOBGT_CHECKINS_ABI_VERSION"] == _checkins.ABI_VERSION == 1
    assert _checkins.EBADDIM < 0 and _checkins.EALIGN < 0 and _checkins.WAVE == 64 and _checkins.NOKEY == 2 ** 63 - 1
    assert min(_checkins.MAX_U0, _checkins.MAX_P0, _checkins.MAX_C0) > 1_300_000 and _checkins.MAX_P0 > _universe.MAX_P
    bits = [_checkins.SBADUSER, _checkins.SBADPOI, _checkins.SBADCAT, _checkins.SBADINDEX, _checkins.SZEROSPLIT]
    assert sorted(bits) == [1, 2, 4, 8, 16]
    assert issubclass(_checkins.MobgtCheckinsError, RuntimeError) and callable(_checkins.launch)

    class Recorder:                                                    # every prototype binds to a handle that has the names
        def __getattr__(self, name):
            fn = types.SimpleNamespace()
            setattr(self, name, fn)
            return fn
    handle = _checkins.LIBRARY.bind(Recorder())
    for name, (res, args) in protos.items():
        assert getattr(handle, name).restype is res and getattr(handle, name).argtypes == args
    assert len(_native.LIBRARIES) == 5 and _checkins.LIBRARY not in _native.LIBRARIES
    assert _checkins.LIBRARY.hip and os.path.basename(_checkins.LIBRARY.path) == "libmobgt_checkins.so"
    for other in _native.LIBRARIES + (_pairbins.LIBRARY, _universe.LIBRARY):       # nothing of the other seven is redeclared
        assert not set(protos) & set(other.SIGNATURES)
        assert not {k for k in consts if k in other.CONSTANTS}
    assert data.sessionize is checkins.sessionize and data.sessionize_host is checkins.sessionize_host
