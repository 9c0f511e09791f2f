"""The POI table and the transition graphs from check-in sessions on the device (csrc_universe/counts.hip through
mobgt_amd.universe) against `data.universe_counts_host`: integer counts, compared for equality, on golden G13 and on the crafted
cases of universe_cases.py -- empty inputs, session ends on every lane of a wave and across the workgroups' chunk edges, counts and
runs beyond 16 bits, both sides of the LDS threshold of the category counters, keys beyond 32 bits, P = 1.  Then end to end:
build_universe on G13's sessions and coordinates gives the Graphormer the reference's files give."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

import universe_cases as uc
from mobgt_amd import _universe, data, synth, universe, workloads
from mobgt_amd.ops import _p, _stream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def assert_same_counts(got, want):
    assert (got.P, got.n_cat, got.T) == (want.P, want.n_cat, want.T)
    for name in ("checkin_cnt", "cat_cnt", "poi_cat", "check_freq", "graph_cat"):
        a, b = getattr(got, name), getattr(want, name)
        assert a.is_cuda and a.dtype == b.dtype == torch.int32 and a.shape == b.shape, name
        assert torch.equal(a.cpu(), b), name
    for name in ("rowptr", "col", "val"):
        a, b = getattr(got.graph_adj, name), getattr(want.graph_adj, name)
        assert a.is_cuda and a.dtype == b.dtype and a.shape == b.shape, name
        assert torch.equal(a.cpu(), b), name


@pytest.mark.parametrize("name", list(uc.CASES))
def test_device_counts_equal_the_host_form(name):
    ds, train, P, n_cat = uc.case(name)
    got = data.universe_counts(ds, train, P=P, n_cat=n_cat, device=DEV)
    assert_same_counts(got, uc.host(name))
    adj = uc.csr_dict(got.graph_adj)                                   # rowptr, ascending columns, positive values
    assert sum(adj.values()) == got.T == int(got.graph_adj.val.sum()) == int(got.graph_cat.sum())
    assert int(got.graph_adj.rowptr[-1]) == got.graph_adj.nnz and int(got.checkin_cnt.sum()) == len(ds.seq)
    if got.P <= 2000:
        assert np.array_equal(got.graph_adj.to_dense(), uc.host(name).graph_adj.to_dense())


def test_wide_counts_and_wide_keys():
    one = data.universe_counts(*uc.case("one_poi_100k")[:2], P=3, n_cat=2, device=DEV)
    assert uc.csr_dict(one.graph_adj) == {(2, 2): 99999} and one.graph_cat.tolist() == [[99999, 0], [0, 0]]
    assert one.checkin_cnt.tolist() == [0, 100000, 0] and one.check_freq.tolist() == [0, 100000, 0]
    run = data.universe_counts(*uc.case("one_transition_70k")[:2], P=12, n_cat=3, device=DEV)
    assert uc.csr_dict(run.graph_adj) == {(5, 9): 70000} and int(run.graph_cat[1, 0]) == 70000
    ds, train, P, n_cat = uc.case("key_width")
    wide = uc.csr_dict(data.universe_counts(ds, train, P=P, n_cat=n_cat, device=DEV).graph_adj)
    assert wide == uc.loop_counts(ds, train, P, n_cat)[3] and max(p for p, _ in wide) == 100000


def test_the_kernel_never_indexes_with_a_bad_id():
    """The host refuses bad ids before a launch; the kernel, called directly, skips them and says so in status."""
    seq = torch.tensor([[1, 0, 1], [9, 0, 1], [2, 0, 1], [2, 0, 7], [3, 0, 2], [-5, 0, 0], [3, 0, 2]], dtype=torch.int32, device=DEV)
    sid = torch.tensor([0, 0, 0, 0, 0, 0, 4], dtype=torch.int32, device=DEV)
    first, slot0 = torch.tensor([0], dtype=torch.int32, device=DEV), torch.tensor([0], dtype=torch.int32, device=DEV)
    P, n_cat, T = 3, 2, 5
    i32 = lambda *s: torch.full(s, -77, dtype=torch.int32, device=DEV)
    checkin_cnt, cat_cnt, lo, hi, graph_cat, status = i32(P), i32(n_cat), i32(P), i32(P), i32(n_cat, n_cat), i32(1)
    keys = torch.full((T,), -77, dtype=torch.int64, device=DEV)
    _universe.launch("mobgt_universe_counts", _p(seq), _p(sid), 7, _p(first), _p(slot0), 1, P, n_cat, _p(checkin_cnt), _p(cat_cnt),
                     _p(lo), _p(hi), _p(graph_cat), _p(keys), T, _p(status), _stream())
    assert int(status[0]) == _universe.SBADPOI | _universe.SBADCAT | _universe.SBADSESSION
    assert checkin_cnt.tolist() == [1, 1, 2] and cat_cnt.tolist() == [2, 2]
    assert lo.tolist() == [1, 1, 2] and hi.tolist() == [1, 1, 2]
    assert not graph_cat.any() and keys.tolist() == [-1] * T                       # every transition touches a skipped check-in
    null = ctypes.c_void_p(0)
    for code, name, args in (
            (_universe.EBADDIM, "mobgt_universe_counts", (_p(seq), _p(sid), 7, _p(first), _p(slot0), 1, 0, n_cat, _p(checkin_cnt),
                                                         _p(cat_cnt), _p(lo), _p(hi), _p(graph_cat), _p(keys), T, _p(status), _stream())),
            (_universe.EBADDIM, "mobgt_universe_counts", (_p(seq), _p(sid), 2 ** 31, _p(first), _p(slot0), 1, P, n_cat, _p(checkin_cnt),
                                                         _p(cat_cnt), _p(lo), _p(hi), _p(graph_cat), _p(keys), T, _p(status), _stream())),
            (_universe.EALIGN, "mobgt_universe_counts", (_p(seq), null, 7, _p(first), _p(slot0), 1, P, n_cat, _p(checkin_cnt),
                                                        _p(cat_cnt), _p(lo), _p(hi), _p(graph_cat), _p(keys), T, _p(status), _stream())),
            (_universe.EBADDIM, "mobgt_universe_run_heads", (_p(keys), 0, _p(checkin_cnt), _stream())),
            (_universe.EBADDIM, "mobgt_universe_run_fill", (_p(keys), _p(keys), T, P, T + 1, _p(keys), _p(lo), _p(hi), _stream())),
            (_universe.EALIGN, "mobgt_universe_run_fill", (_p(keys), _p(keys), T, P, 2, null, _p(lo), _p(hi), _stream()))):
        with pytest.raises(_universe.MobgtUniverseError, match="MOBGT_UNIVERSE_E") as e:
            _universe.launch(name, *args)
        assert e.value.code == code, (name, e.value.code)
    torch.cuda.synchronize()


def test_transition_csr_of_given_keys():
    P = 50000
    pairs = [(49999, 49999), (0, 0), (49999, 0), (7, 3), (0, 0), (7, 3), (7, 2), (0, 49999), (7, 3)]
    keys = torch.tensor([p * P + q for p, q in pairs], dtype=torch.int64, device=DEV)
    g = universe.transition_csr(keys, P)
    assert uc.csr_dict(g) == {(1, 1): 2, (1, 50000): 1, (8, 3): 1, (8, 4): 3, (50000, 1): 1, (50000, 50000): 1}
    empty = universe.transition_csr(keys[:0], 5)
    assert empty.nnz == 0 and empty.rowptr.tolist() == [0] * 6


def _model(uni, num_bins):
    from mobgt_amd.model_fqandtoyo import Graphormer
    torch.manual_seed(13)
    args = dict(workloads.COMMON, n_layers=2, hidden_dim=128, dataset_name="foursquaregraph", ffn_dim=256)
    return Graphormer(universe=uni, num_bins=num_bins, **args).to(DEV).eval()


def test_sessions_and_coordinates_in_a_graphormer_out_g13():
    """build_universe on G13's sessions and coordinates against a synth.Universe of the reference's own four files: the same
    model buffers and, with the same seed and the same batch, the same logits bit for bit.  Graph_dist of the second model is
    the golden's array as a scipy CSR, the form that sends the f32 GCN down the path a RadiusGraph takes (csrc/spmm.hip)."""
    from scipy import sparse
    z = uc.g13()
    ds = data.SessionDataset(uc.g13_sessions())
    built = data.build_universe(ds, train=z["train"], coords_deg=z["coords"], radius_km=3.0, device=DEV)
    assert_same_counts(built.counts, uc.host("g13"))
    u = built.universe
    assert np.array_equal(u.poi_table, z["ref_poi"]) and np.array_equal(u.graph_cat, z["ref_cat"]) and u.graph_cat.dtype == np.float32
    assert np.array_equal(u.graph_dist.to_dense01(), z["ref_dist"]) and np.array_equal(u.graph_adj.to_dense(), z["ref_adj"])
    assert u.distance is None and (u.P, u.n_cat, u.n_user) == (len(z["ref_poi"]), len(z["ref_cat"]), 12)
    ref_uni = synth.Universe(P=u.P, n_cat=u.n_cat, n_user=12, poi_table=z["ref_poi"], graph_adj=z["ref_adj"].astype(np.float32),
                             graph_dist=sparse.csr_matrix(z["ref_dist"].astype(np.float32)), graph_cat=z["ref_cat"].astype(np.float32))
    num_bins = built.bins.num_bins + 2
    ours, theirs = _model(u, num_bins), _model(ref_uni, num_bins)
    assert ours.fre_embed_model.num_embeddings == theirs.fre_embed_model.num_embeddings == int(z["ref_poi"][:, 5].max()) + 1
    for name in ("X", "C_X", "C_A", "C_AX", "poi2cat", "D_AX", "D_A_rowptr", "D_A_col", "D_A_val"):
        a, b = getattr(ours, name), getattr(theirs, name)
        assert a.dtype == b.dtype and torch.equal(a, b), name
    coll = data.SessionCollator(DEV, bin_table=built.bins.table)
    batch = coll([ds[i] for i in range(len(ds))])
    assert int(batch.poi_pos.max()) < num_bins
    with torch.no_grad():
        a, b = ours(batch), theirs(batch)
    for x, y in zip(a[:2], b[:2]):
        assert x.shape == y.shape and torch.isfinite(x).all() and torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert a[0].shape == (len(ds), u.P)
