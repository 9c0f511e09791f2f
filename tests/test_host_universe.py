"""The POI table and the transition graphs from check-in sessions on the host: `data.universe_counts_host` (the reference of the
kernels in csrc_universe/counts.hip) against the reference's own files (golden G13) and against plain loops,
`data.first_seen_ids`, `write_csvs`, everything that is refused before a launch, and the seventh library's header.  No GPU."""
import os
import types

import numpy as np
import pytest
import torch

import universe_cases as uc
from mobgt_amd import _cabi, _native, _pairbins, _universe, data, geo, synth, universe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_form_equals_the_reference_files_g13():
    z, c = uc.g13(), uc.host("g13")
    P, n_cat = len(z["ref_poi"]), len(z["ref_cat"])
    assert (c.P, c.n_cat) == (P, n_cat) and c.T == int(z["ref_adj"].sum()) == int(z["ref_cat"].sum())
    for t, shape in ((c.checkin_cnt, (P,)), (c.cat_cnt, (n_cat,)), (c.poi_cat, (P,)), (c.check_freq, (P,)), (c.graph_cat, (n_cat, n_cat))):
        assert t.dtype == torch.int32 and tuple(t.shape) == shape
    assert np.array_equal(c.checkin_cnt.numpy(), z["ref_poi"][:, 1])
    assert np.array_equal(c.poi_cat.numpy(), z["ref_poi"][:, 4])
    assert np.array_equal(c.check_freq.numpy(), z["ref_poi"][:, 5])
    table = c.poi_table(z["coords"])
    assert table.dtype == np.float64 and np.array_equal(table, z["ref_poi"])           # POI ID, lat and lon too
    assert np.array_equal(c.graph_cat.numpy(), z["ref_cat"])
    assert np.array_equal(c.graph_adj.to_dense(), z["ref_adj"]) and c.graph_adj.to_dense().dtype == np.float32
    assert (c.graph_adj.to_scipy() != z["ref_adj"]).sum() == 0
    assert np.diagonal(z["ref_adj"]).sum() > 0 and z["ref_adj"].max() >= 2              # G13 has self transitions and repeats
    # the train flags as indices, and as the sessions themselves instead of a dataset
    again = data.universe_counts_host(uc.g13_sessions(), np.nonzero(z["train"])[0])
    assert torch.equal(again.graph_cat, c.graph_cat) and torch.equal(again.graph_adj.val, c.graph_adj.val)
    # the within-radius graph of the same coordinates is the reference's Graph_dist
    assert np.array_equal(geo.radius_graph_host(z["coords"], 3.0).to_dense01(), z["ref_dist"])


def test_first_seen_ids_give_the_reference_numbering_g13():
    z = uc.g13()
    for raw, col in (("raw_poi", 0), ("raw_cat", 2)):
        dense, lookup = data.first_seen_ids(z[raw])
        assert dense.dtype == np.int64 and np.array_equal(dense, z["seq"][:, col])
        assert len(lookup) == dense.max() and np.array_equal(lookup[dense - 1], z[raw])
        as_list, _ = data.first_seen_ids(list(z[raw]))
        assert np.array_equal(as_list, dense)
    dense, lookup = data.first_seen_ids([("a", 1), 7, ("a", 1), "x", 7])               # any hashable
    assert dense.tolist() == [1, 2, 1, 3, 2] and list(lookup) == [("a", 1), 7, "x"]
    assert data.first_seen_ids(np.array([40, 7, 40, 2 ** 40]))[0].tolist() == [1, 2, 1, 3]
    assert data.first_seen_ids([])[0].shape == (0,)
    with pytest.raises(ValueError, match="flat"):
        data.first_seen_ids(np.zeros((2, 2), dtype=np.int64))


@pytest.mark.parametrize("name", uc.LOOPED)
def test_host_form_equals_plain_loops(name):
    ds, train, _, _ = uc.case(name)
    c = uc.host(name)
    checkin_cnt, cat_cnt, graph_cat, adj = uc.loop_counts(ds, train, c.P, c.n_cat)
    assert np.array_equal(c.checkin_cnt.numpy(), checkin_cnt) and np.array_equal(c.cat_cnt.numpy(), cat_cnt)
    assert np.array_equal(c.graph_cat.numpy(), graph_cat) and uc.csr_dict(c.graph_adj) == adj
    assert c.T == sum(adj.values()) == int(graph_cat.sum()) and int(checkin_cnt.sum()) == len(ds.seq)
    seen = checkin_cnt > 0
    assert (c.poi_cat.numpy()[~seen] == 0).all() and (c.check_freq.numpy()[~seen] == 0).all() and (c.poi_cat.numpy()[seen] >= 1).all()
    assert np.array_equal(c.check_freq.numpy()[seen], cat_cnt[c.poi_cat.numpy()[seen] - 1])


def test_the_cases_hold_what_they_are_for():
    ds, train, P, _ = uc.case("boundaries")
    adj = uc.csr_dict(uc.host("boundaries").graph_adj)
    assert adj and all(q == p + 1 for p, q in adj)                     # inside a session: x -> x + 1 only
    ends = ds.offsets[1:-1]
    across = set(zip(ds.seq[ends - 1, 0].tolist(), ds.seq[ends, 0].tolist()))
    assert len(across) > 500 and not across & set(adj)                 # every pair across a boundary: absent from the truth
    assert train[::2].all() and not train[1::2].any()
    assert uc.csr_dict(uc.host("one_poi_100k").graph_adj) == {(2, 2): 99999}
    assert uc.csr_dict(uc.host("one_transition_70k").graph_adj) == {(5, 9): 70000}
    assert uc.THRESHOLD == _universe.LDS_MAX_CAT and 4 * uc.THRESHOLD ** 2 <= 48 * 1024
    for name, n_cat in (("n_cat_1", 1), ("n_cat_threshold", uc.THRESHOLD), ("n_cat_threshold_plus_1", uc.THRESHOLD + 1), ("n_cat_600", 600),
                        ("n_cat_max", _universe.MAX_CAT)):
        c = uc.host(name)
        assert c.n_cat == n_cat and (c.cat_cnt > 0).all() and int(c.graph_cat.sum()) == c.T > uc.CHUNK
    kw = uc.host("key_width")
    assert kw.P == 100000 and kw.graph_adj.rowptr.shape == (100001,) and 50 < kw.graph_adj.nnz <= 144
    e, n = uc.host("empty"), uc.host("no_train")
    assert (e.P, e.n_cat, e.T, e.graph_adj.nnz) == (1, 1, 0, 0) and e.graph_adj.rowptr.tolist() == [0, 0]
    assert n.T == 0 and n.graph_adj.nnz == 0 and not n.graph_cat.any() and int(n.checkin_cnt.sum()) == len(uc.case("no_train")[0].seq)


def test_unvisited_pois_and_given_sizes():
    ds = data.SessionDataset([(0, [[2, 0, 3], [5, 1, 1], [2, 2, 3]]), (1, [[5, 0, 1], [5, 3, 1]])])
    c = data.universe_counts_host(ds, [0], P=7, n_cat=4)
    assert c.checkin_cnt.tolist() == [0, 2, 0, 0, 3, 0, 0] and c.poi_cat.tolist() == [0, 3, 0, 0, 1, 0, 0]
    assert c.cat_cnt.tolist() == [3, 0, 2, 0] and c.check_freq.tolist() == [0, 2, 0, 0, 3, 0, 0]
    assert uc.csr_dict(c.graph_adj) == {(2, 5): 1, (5, 2): 1} and c.graph_cat.tolist() == [[0, 0, 1, 0], [0] * 4, [1, 0, 0, 0], [0] * 4]
    d = data.universe_counts_host(ds, np.array([True, True]))
    assert (d.P, d.n_cat) == (5, 3) and uc.csr_dict(d.graph_adj) == {(2, 5): 1, (5, 2): 1, (5, 5): 1}
    with pytest.raises(ValueError, match=r"\[7, 2\]"):
        c.poi_table(np.zeros((5, 2)))


@pytest.mark.parametrize("counts", [data.universe_counts_host, lambda *a, **k: data.universe_counts(*a, device="cuda", **k)],
                         ids=["host", "device"])
def test_bad_input_is_refused_on_the_host_with_the_session_named(counts, monkeypatch):
    """Both forms validate before anything else: the device form raises these without a GPU, without its library."""
    monkeypatch.setattr(_universe.LIBRARY, "lib", lambda: pytest.fail("validation comes before the library is loaded"))
    good = [(0, [[2, 0, 3], [5, 1, 1]]), (1, [[5, 0, 1], [4, 3, 2], [1, 0, 1]]), (1, [[3, 0, 2], [3, 3, 2]])]

    def broken(session, row, col, value):
        s = [(u, np.array(c)) for u, c in good]
        s[session][1][row, col] = value
        return data.SessionDataset(s)

    for ds, kw, match in ((broken(1, 2, 0, 0), {}, r"session 1: POI id 0 at check-in 2"),
                          (broken(2, 0, 0, -4), {}, r"session 2: POI id -4 at check-in 0"),
                          (broken(1, 1, 2, 0), {}, r"session 1: category id 0 at check-in 1"),
                          (data.SessionDataset(good), dict(P=4), r"session 0: POI id 5 at check-in 1 is not in 1 \.\. 4"),
                          (data.SessionDataset(good), dict(n_cat=2), r"session 0: category id 3 at check-in 0 is not in 1 \.\. 2")):
        with pytest.raises(ValueError, match=match):
            counts(ds, np.ones(3, dtype=bool), **kw)
    ds = data.SessionDataset(good)
    with pytest.raises(ValueError, match="train: a mask of 2 flags for 3 sessions"):
        counts(ds, np.ones(2, dtype=bool))
    with pytest.raises(ValueError, match="train: session index 3 is not in 0 .. 2"):
        counts(ds, [0, 3])
    with pytest.raises(ValueError, match="train: a boolean mask"):
        counts(ds, [0.5])
    # 2**31 check-ins: a view of one row, no memory behind it; session 1 holds check-in number 2**31
    huge = types.SimpleNamespace(seq=np.broadcast_to(np.array([[1, 0, 1]], dtype=np.int32), (2 ** 31, 3)),
                                 offsets=np.array([0, 5, 2 ** 31], dtype=np.int64), users=np.zeros(2, dtype=np.int64))
    with pytest.raises(ValueError, match=r"session 1: check-in number 2\*\*31"):
        counts(huge, np.ones(2, dtype=bool))


def test_a_poi_with_two_categories_is_refused_by_name():
    ds = data.SessionDataset([(0, [[2, 0, 3], [5, 1, 1]]), (1, [[4, 0, 1], [5, 3, 2]])])
    with pytest.raises(ValueError, match=r"POI 5 was seen with more than one category \(1 \.\. 2\)"):
        data.universe_counts_host(ds, [0, 1])
    with pytest.raises(ValueError, match="POI 3 was seen"):                 # what the device form does with the kernel's min / max
        universe._one_category(np.array([1, 2 ** 31 - 1, 2, 4]), np.array([1, 0, 5, 4]))
    assert universe._one_category(np.array([1, 2 ** 31 - 1, 4]), np.array([1, 0, 4])).tolist() == [1, 0, 4]
    with pytest.raises(ValueError, match="universe_counts_host"):
        data.universe_counts(ds, [0], device="cpu")


def test_wide_ids_are_refused_before_any_cast_and_dense_copies_above_a_stated_size():
    wide = types.SimpleNamespace(seq=np.array([[2, 0, 1], [2 ** 32 + 1, 0, 1], [3, 0, 2 ** 32 + 2]], dtype=np.int64),
                                 offsets=np.array([0, 1, 3], dtype=np.int64), users=np.zeros(2, dtype=np.int64))
    with pytest.raises(ValueError, match=rf"session 1: POI id {2 ** 32 + 1} at check-in 0"):      # (as int32 it would be POI 1)
        data.universe_counts_host(wide, [0, 1])
    with pytest.raises(ValueError, match=rf"session 1: POI id {2 ** 32 + 1} at check-in 0 is not in 1 \.\. 5"):
        data.universe_counts_host(wide, [0, 1], P=5)
    wide.seq[1, 0] = 1
    with pytest.raises(ValueError, match=rf"session 1: category id {2 ** 32 + 2} at check-in 1"):
        data.universe_counts_host(wide, [0, 1], n_cat=2)
    big = universe.TransitionGraph(universe.MAX_DENSE_P + 1, torch.zeros(universe.MAX_DENSE_P + 2, dtype=torch.int64),
                                   torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.int32))
    with pytest.raises(ValueError, match=f"up to {universe.MAX_DENSE_P} POIs"):
        big.to_dense()
    assert big.to_scipy().nnz == 0 and universe.MAX_CSV_P <= universe.MAX_DENSE_P


def _built_on_the_host():
    """build_universe's result with the host forms in place of the device ones (what write_csvs reads)."""
    z, c = uc.g13(), uc.host("g13")
    uni = synth.Universe(P=c.P, n_cat=c.n_cat, n_user=12, poi_table=c.poi_table(z["coords"]), graph_adj=c.graph_adj,
                         graph_dist=geo.radius_graph_host(z["coords"], 3.0), graph_cat=c.graph_cat.numpy().astype(np.float32),
                         distance=None, poi_columns=universe.POI_COLUMNS)
    return data.BuiltUniverse(uni, None, c, z["coords"])


def test_write_csvs_reads_back_as_the_reference_files(tmp_path):
    import pandas as pd
    z, built = uc.g13(), _built_on_the_host()
    built.write_csvs(str(tmp_path / "raw"))
    frames = {k: pd.read_csv(tmp_path / "raw" / f"Graph_{k}.csv") for k in ("poi", "cat", "adj", "dist")}
    for k, f in frames.items():
        got = f.to_numpy()
        assert got.shape == z["ref_" + k].shape and np.array_equal(got, z["ref_" + k]), k
    assert tuple(frames["poi"].columns) == synth.Universe.poi_columns == universe.POI_COLUMNS
    assert frames["poi"]["checkin_cnt"].dtype == np.int64 and frames["poi"]["lat"].dtype == np.float64
    for k in ("cat", "adj", "dist"):                                   # headers 1 .. K, no index column
        assert [int(c) for c in frames[k].columns] == list(range(1, len(frames[k]) + 1))
    big = data.BuiltUniverse(None, None, types.SimpleNamespace(P=universe.MAX_CSV_P + 1), None)
    with pytest.raises(ValueError, match=f"up to {universe.MAX_CSV_P} POIs"):
        big.write_csvs(str(tmp_path / "big"))
    assert not (tmp_path / "big").exists()


def test_header_binds_and_the_library_stays_out_of_the_pinned_five():
    protos, consts = _cabi.load(os.path.join(ROOT, "include", "mobgt_universe.h"))
    vp, ci, i64 = _cabi.ctypes.c_void_p, _cabi.ctypes.c_int, _cabi.ctypes.c_int64
    assert list(protos) == ["mobgt_universe_abi_version", "mobgt_universe_counts", "mobgt_universe_run_heads", "mobgt_universe_run_fill"]
    assert protos["mobgt_universe_counts"] == (ci, [vp, vp, i64, vp, vp, i64, i64, ci] + [vp] * 6 + [i64, vp, vp])
    assert protos["mobgt_universe_run_heads"] == (ci, [vp, i64, vp, vp])
    assert protos["mobgt_universe_run_fill"] == (ci, [vp, vp, i64, i64, i64, vp, vp, vp, vp])
    assert protos == _universe.SIGNATURES and consts["MOBGT_UNIVERSE_ABI_VERSION"] == _universe.ABI_VERSION == 1
    assert _universe.EBADDIM < 0 and _universe.EALIGN < 0 and _universe.MAX_P >= 100000 and _universe.MAX_CAT >= 600
    assert 4 * (_universe.LDS_MAX_CAT ** 2 + _universe.MAX_CAT) <= 64 * 1024         # cat_cnt and graph_cat side by side in LDS
    assert len({_universe.SBADPOI, _universe.SBADCAT, _universe.SBADSESSION}) == 3
    assert issubclass(_universe.MobgtUniverseError, RuntimeError) and callable(_universe.launch)

    class Recorder:                                                    # every prototype binds to a handle that has the names
        def __getattr__(self, name):
            fn = types.SimpleNamespace()
            setattr(self, name, fn)
            return fn
    handle = _universe.LIBRARY.bind(Recorder())
    for name, (res, args) in protos.items():
        assert getattr(handle, name).restype is res and getattr(handle, name).argtypes == args
    assert len(_native.LIBRARIES) == 5 and _universe.LIBRARY not in _native.LIBRARIES
    assert _universe.LIBRARY.hip and os.path.basename(_universe.LIBRARY.path) == "libmobgt_universe.so"
    for other in _native.LIBRARIES + (_pairbins.LIBRARY,):             # nothing of theirs is redeclared
        assert not set(protos) & set(other.SIGNATURES)
    assert data.universe_counts is universe.universe_counts and data.build_universe is universe.build_universe
