"""Check-in sessions on the host: `data.sessions_to_trajectories` against what the reference's gen_pickles writes for the same
sessions (golden G12, tests/golden/make_golden_sessions.py), `data.SessionDataset`, the limit bounds of `data.SessionCollator`
and the third library's header.  No GPU."""
import os
import re

import numpy as np
import pytest

from mobgt_amd import _cabi, _lib, _lib_data, data, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def g12_sessions(golden_dir):
    z = np.load(os.path.join(golden_dir, "g12_sessions.npz"))
    o = z["offsets"]
    return z, [(int(z["users"][i]), z["checkins"][o[i]:o[i + 1]]) for i in range(len(z["users"]))]


def test_converter_equals_the_reference_bit_for_bit(golden_dir):
    z, sessions = g12_sessions(golden_dir)
    assert 20 <= len(sessions) <= 48
    no, eo = z["node_offsets"], z["edge_offsets"]
    trajs = data.sessions_to_trajectories(sessions)
    for i, (t, (user, c)) in enumerate(zip(trajs, sessions)):
        name = str(z["names"][i])
        node = slice(no[i], no[i + 1])
        assert len(t["node_name"]) == z["ref_num_node"][i] == len(np.unique(c[:-1, 0])), name
        assert np.array_equal(t["node_name"], z["ref_node_name"][node]), name
        assert np.array_equal(t["edge_type"].reshape(-1), z["ref_edge_type"][eo[i]:eo[i + 1]]), name
        assert np.array_equal(t["time"], z["ref_time"][node]) and np.array_equal(t["cat"], z["ref_cat"][node]), name
        assert t["time_normal"].dtype == np.float32
        assert np.array_equal(t["time_normal"].view(np.uint32), z["ref_time_normal"][node].view(np.uint32)), name
        assert t["target"].tolist() == [z["ref_target"][i]] == [c[-1, 0]] and t["user"].tolist() == [z["ref_user"][i]] == [user]
        assert t["node_name"][-1] == c[-2, 0], name                   # the last node IS the last history check-in
        assert int(t["edge_type"].sum()) == len(c) - 2, name          # one count per transition of the history
    by = {str(n): t for n, t in zip(z["names"], trajs)}
    assert by["issue_example"]["node_name"].tolist() == [2, 1, 4]
    assert by["issue_example"]["edge_type"].tolist() == [[0, 1, 0], [0, 0, 2], [1, 0, 3]]
    assert by["two_checkins"]["edge_type"].tolist() == [[0]] and by["one_poi_repeated"]["edge_type"].tolist() == [[11]]
    assert {0, 47} <= set(by["slots_0_and_47"]["time"].tolist())


def test_time_normal_is_the_float_of_the_double_quotient():
    hist = np.stack([np.arange(1, 49), np.arange(48), np.ones(48, dtype=np.int64)], 1)
    tn = data.session_graph(hist)["time_normal"]
    for t in range(48):
        want = np.float32(0) if t == 0 else np.float32(t / 48)
        assert tn[t].view(np.uint32) == want.view(np.uint32), t


def test_dataset_validates_once_and_records_n(golden_dir):
    _, sessions = g12_sessions(golden_dir)
    ds = data.SessionDataset(sessions)
    assert len(ds) == len(sessions) and ds.seq.dtype == np.int32 and ds.offsets[-1] == sum(len(c) for _, c in sessions)
    for i, (user, c) in enumerate(sessions):
        r = ds[i]
        _, cnt = np.unique(c[:-1, 0], return_counts=True)
        assert (r.user, r.n, r.mult) == (user, len(cnt), cnt.max()) and np.array_equal(r.checkins, c)
    assert ds.max_n == max(ds[i].n for i in range(len(ds))) == int(ds.n.max())
    assert ds[-1].user == sessions[-1][0]
    with pytest.raises(IndexError):
        ds[len(ds)]
    trajs = data.sessions_to_trajectories(ds)                          # a dataset converts like its sessions
    assert all(np.array_equal(a["edge_type"], b["edge_type"]) for a, b in zip(trajs, data.sessions_to_trajectories(sessions)))
    one = np.array([[3, 1, 2]])
    with pytest.raises(ValueError, match="session 2 "):
        data.SessionDataset(sessions[:2] + [(0, one)])
    with pytest.raises(ValueError, match="session 0"):
        data.SessionDataset([(0, np.zeros((4, 2), dtype=np.int64))])
    with pytest.raises(ValueError, match="session 1"):
        data.SessionDataset([sessions[0], (0, np.zeros((4, 3), dtype=np.float32))])
    with pytest.raises(ValueError, match="session 0"):
        data.SessionDataset([(0, np.full((4, 3), 2 ** 31, dtype=np.int64))])


def test_raw_pairs_are_validated_like_a_datasets():
    good = (1, np.array([[3, 1, 2], [4, 2, 2]]))
    assert data._as_record(good).n == 1 and data.sessions_to_trajectories([good])[0]["target"].tolist() == [4]
    for bad, match in (((1, np.array([[3, 1, 2]])), "1 check-in"), ((1, np.full((3, 3), 2 ** 31, dtype=np.int64)), "int32"),
                       ((1, np.zeros((3, 3), dtype=np.float64)), "integers"), ((1.5, good[1]), "integers"), (7, "expected")):
        with pytest.raises(ValueError, match=match):
            data.sessions_to_trajectories([bad])
    coll = data.SessionCollator.__new__(data.SessionCollator)
    coll.max_node = 0                                                  # (every session is dropped: said so, before any device work)
    with pytest.raises(ValueError, match="no session to collate"):
        coll([good, None])
    with pytest.raises(ValueError, match="session 1 has 1 check-in"):
        coll([good, (1, np.array([[3, 1, 2]]))])


def _violation_from_dicts(recs, L, N):
    """DeviceCollator's own check (the dict path) on the converted sessions: the exact answer."""
    coll = data.DeviceCollator.__new__(data.DeviceCollator)
    coll.max_node = 30000
    return coll.limit_violation(coll.pack_host(data.sessions_to_trajectories(recs), n_pad=N), L)


def test_cheap_bounds_never_pass_what_the_exact_check_rejects():
    """Seeded random batches against small tables: the session path reports exactly what the dict path reports -- the same
    field, the same index, the same table size -- and in particular never None where the dict path finds a violation."""
    rng = np.random.RandomState(5)
    coll = data.SessionCollator.__new__(data.SessionCollator)
    coll.max_node = 30000
    hits = {}
    for trial in range(400):
        P = int(rng.choice([3, 6, 12, 40]))
        recs = []
        for _ in range(int(rng.randint(1, 5))):
            L = int(rng.randint(1, 40))
            c = np.stack([rng.randint(1, P + 1, L + 1), rng.randint(0, 48, L + 1), rng.randint(1, 9, L + 1)], 1)
            recs.append(data._as_record((int(rng.randint(0, 9)), c)))
        limits = dict(x=int(rng.randint(2, 45)), user=int(rng.randint(3, 12)), y=int(rng.randint(2, 45)), edge=int(rng.randint(4, 12)),
                      deg=int(rng.randint(2, 9)), slots=int(rng.randint(20, 50)))
        for keys in (limits, {k: limits[k] for k in ("edge", "deg", "slots")}, {"slots": limits["slots"]}, {"deg": limits["deg"]}):
            Lp = max(len(r.checkins) - 1 for r in recs)
            N = data.bucket_nodes(max(r.n for r in recs))
            buf = np.zeros(data.SessionLayout(len(recs)).nbytes(Lp), dtype=np.uint8)
            h = coll.pack_sessions(recs, 0, data.SessionLayout(len(recs)).views_np(buf, Lp))
            got, want = coll.limit_violation(h, keys), _violation_from_dicts(recs, keys, N)
            assert got == want, (trial, keys, got, want)
            hits[want and want[0]] = hits.get(want and want[0], 0) + 1
    assert set(hits) == {None, "x", "user", "y", "edge_input", "degree", "time_normal"}, hits     # every branch was taken


def test_synthetic_sessions_have_the_node_counts_asked_for():
    uni = synth.make_universe(P=200, n_cat=8, n_user=8, seed=0)
    sess = synth.make_sessions(seed=3, G=6, P=uni.P, n_user=uni.n_user, cat_of_poi=uni.cat_of_poi, n_nodes=[1, 2, 5, 17, 64, 150])
    ds = data.SessionDataset(sess)
    assert ds.n.tolist() == [1, 2, 5, 17, 64, 150]
    assert all(c.dtype == np.int32 and c[:, 0].min() >= 1 and c[:, 0].max() <= uni.P for _, c in sess)


def test_header_parses_and_states_the_limits():
    protos, consts = _cabi.load(os.path.join(ROOT, "include", "mobgt_data.h"))
    vp, ci = _cabi.ctypes.c_void_p, _cabi.ctypes.c_int
    assert list(protos) == ["mobgt_data_abi_version", "mobgt_sessions_to_raw"]
    res, args = protos["mobgt_sessions_to_raw"]
    assert res is ci and args == [vp] * 9 + [ci, ci, ci, vp]
    assert consts["MOBGT_DATA_ABI_VERSION"] == _lib_data.ABI_VERSION == 1
    assert consts["MOBGT_DATA_MAX_LP"] >= 4096 and consts["MOBGT_DATA_MAX_N"] >= max(data.BUCKETS) == 1024
    assert consts["MOBGT_DATA_EBADDIM"] < 0 and consts["MOBGT_DATA_SOK"] == 0 and _lib_data.SBADLEN and _lib_data.SNODES
    assert not set(protos) & set(_lib.SIGNATURES)                      # a library of its own: nothing of the closed ABI


def test_nothing_reaches_the_new_library_through_a_function_named_call():
    pkg = os.path.join(ROOT, "mobgt_amd")
    for f in sorted(os.listdir(pkg)):
        if not f.endswith(".py"):
            continue
        text = open(os.path.join(pkg, f), encoding="utf-8").read()
        assert not re.search(r"\bcall\(\s*[\"']mobgt_(data_|sessions_)", text), f
        assert not re.search(r"_lib_data\.call\b|def call\b", text) or f == "_lib.py", f
    assert not hasattr(_lib_data, "call") and callable(_lib_data.launch)
