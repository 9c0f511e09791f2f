"""The within-radius POI graph on the host: `geo.radius_graph_host` against today's constructions (synth.make_universe's
haversine graph, MaskAdj.from_dense01, CsrAdj.from_scipy of model_fqandtoyo's a_hat), the host copies of a RadiusGraph, and
the fourth library's header.  No GPU."""
import dataclasses
import os
import re

import numpy as np
import pytest
import torch

import geo_cases
from mobgt_amd import _cabi, _lib, _lib_data, _lib_geo, geo, synth, workloads
from mobgt_amd.modelGNN import CsrAdj, MaskAdj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def universe():
    uni = synth.make_universe(P=200, n_cat=8, n_user=8, seed=0)
    coords = uni.poi_table[:, 2:4]
    geo_cases.assert_margin(coords)                                    # formula variants of `0 < d <= 3` cannot disagree here
    return uni, coords


def a_hat_of(graph01):
    """model_fqandtoyo.Graphormer's sparse-path construction of (D+I)^-1 (A+I), in f64."""
    from scipy import sparse
    a = sparse.csr_matrix(graph01, dtype=np.float64)
    deg = np.asarray(a.sum(axis=1)).reshape(-1) + 1.0
    return sparse.diags(1.0 / deg) @ (a + sparse.identity(a.shape[0], format="csr"))


def same(got, want):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape, (k, a.dtype, b.dtype, a.shape, b.shape)
        raw = lambda t: t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t
        assert torch.equal(raw(a), raw(b)), k


def test_header_parses_and_is_a_library_of_its_own():
    protos, consts = _cabi.load(os.path.join(ROOT, "include", "mobgt_geo.h"))
    vp, ci, i64, f64 = _cabi.ctypes.c_void_p, _cabi.ctypes.c_int, _cabi.ctypes.c_int64, _cabi.ctypes.c_double
    assert list(protos) == ["mobgt_geo_abi_version", "mobgt_geo_unit_vectors", "mobgt_geo_radius_words", "mobgt_geo_radius_count",
                            "mobgt_geo_radius_fill"]
    assert protos["mobgt_geo_unit_vectors"] == (ci, [vp, vp, i64, vp])
    assert protos["mobgt_geo_radius_words"] == (ci, [vp, i64, f64, vp, vp, vp])
    assert protos["mobgt_geo_radius_count"] == (ci, [vp, i64, f64, vp, vp])
    assert protos["mobgt_geo_radius_fill"] == (ci, [vp, i64, f64, vp, vp, vp, vp])
    assert protos == _lib_geo.SIGNATURES and consts["MOBGT_GEO_ABI_VERSION"] == _lib_geo.ABI_VERSION == 1
    assert consts["MOBGT_GEO_EBADDIM"] == _lib_geo.EBADDIM < 0 and consts["MOBGT_GEO_EALIGN"] == _lib_geo.EALIGN < 0
    assert consts["MOBGT_GEO_MAX_P"] >= 100000 and consts["MOBGT_GEO_TILE"] == 2048
    assert not set(protos) & set(_lib.SIGNATURES) and not set(protos) & set(_lib_data.SIGNATURES)
    text = open(os.path.join(ROOT, "include", "mobgt_geo.h"), encoding="utf-8").read()
    blocks = re.findall(r"/\*(?:(?!\*/).)*\*/\s*int mobgt_geo_(?:unit|radius)\w+\(", text, re.S)
    assert len(blocks) == 4
    for block in blocks:                                               # every entry point cites the lines it replaces
        assert "foursquare_process.py:" in block and ":15-23" in block, block[:80]
        assert ":689-702" in block or "mobgt_geo_unit_vectors" in block, block[:80]
    assert callable(_lib_geo.launch) and not hasattr(_lib_geo, "call")
    src = open(os.path.join(ROOT, "mobgt_amd", "geo.py"), encoding="utf-8").read()
    assert not re.search(r"\bcall\(", src)


def test_host_graph_is_todays_haversine_graph():
    uni, coords = universe()
    g = geo.radius_graph_host(coords, 3.0)
    assert g.forms == ("mask", "csr") and g.P == 200 and g.deg.dtype == torch.int32
    assert np.array_equal(g.to_dense01(), uni.graph_dist) and g.to_dense01().dtype == np.float32
    assert np.array_equal(g.deg.numpy(), uni.graph_dist.sum(axis=1).astype(np.int32)) and 0 == g.deg.min() < g.deg.max()
    sp = g.to_scipy()
    assert sp.dtype == np.float32 and sp.has_sorted_indices and np.array_equal(np.asarray(sp.todense()), uni.graph_dist)
    for forms in (("mask",), ("csr",), "csr"):                         # each form alone describes the same graph
        one = geo.radius_graph_host(coords, 3.0, forms=forms)
        assert one.forms == ((forms,) if isinstance(forms, str) else forms)
        assert np.array_equal(one.to_dense01(), uni.graph_dist) and torch.equal(one.deg, g.deg)
    padded = np.concatenate([np.full((1, 2), 77.0), coords])           # [P + 1, 2]: row 0 = the pad POI
    assert torch.equal(geo.radius_graph_host(padded, 3.0, pad_row=True).col, g.col)
    assert geo.radius_graph_host(coords, 0.5).deg.sum() < g.deg.sum() < geo.radius_graph_host(coords, 6.0).deg.sum()


def test_packing_equals_todays_constructions_bit_for_bit():
    uni, coords = universe()
    g = geo.radius_graph_host(coords, 3.0)
    same(g.mask_adj(), MaskAdj.from_dense01(uni.graph_dist))
    same(g.csr_adj(), CsrAdj.from_scipy(a_hat_of(uni.graph_dist)))
    assert g.mask_adj()[0].shape == (200, 8) and g.rowptr[-1] == g.col.numel() == int(g.deg.sum()) + 200


def test_awkward_points_follow_the_reference_rule():
    c, g = geo_cases.reference(129)
    d = g.to_dense01()
    assert np.array_equal(d, d.T) and not d.diagonal().any()
    assert g.deg[3] == 0 and g.deg[128] == 0                           # the pole, the equator: isolated
    assert d[11, 64] == 1 and d[64, 11] == 1                           # across longitude +-180
    for a, b in ((7, 20), (127, 21)):                                  # exact duplicates: not neighbours, same rows otherwise
        assert d[a, b] == 0 and d[b, a] == 0
        rest = np.ones(129, dtype=bool)
        rest[[a, b]] = False
        assert np.array_equal(d[a, rest], d[b, rest])
    lat, lon = c[:, 0], c[:, 1]
    hav = synth.haversine_km(lat[:, None], lon[:, None], lat[None, :], lon[None, :])
    assert np.array_equal(d, ((hav > 0) & (hav <= 3.0)).astype(np.float32))
    for P in (1, 2):
        _, s = geo_cases.reference(P)
        assert s.deg.tolist() == [P - 1] * P and s.mask_adj()[0].shape == (P, 4) and s.col.tolist() == list(range(P)) * P


def test_arguments_are_checked():
    for bad, match in ((np.zeros((3, 3)), "expected"), (np.zeros((0, 2)), "no POI"), (np.array([[np.nan, 1.0]]), "finite")):
        with pytest.raises(ValueError, match=match):
            geo.radius_graph_host(bad)
    with pytest.raises(ValueError, match="forms"):
        geo.radius_graph_host(np.zeros((2, 2)), forms=("dense",))
    with pytest.raises(ValueError, match="radius_graph_host"):
        geo.radius_graph(np.zeros((2, 2)), device="cpu")
    g = geo.radius_graph_host(np.zeros((2, 2)), forms=("csr",))
    with pytest.raises(ValueError, match="'mask'"):
        g.mask_adj()


def test_graphormer_registers_a_radius_graph_as_it_registers_todays_inputs():
    """The constructor's new branch, on a host RadiusGraph: the same buffers, bit for bit, as from the dense matrix (bf16 GCN:
    the bitmask configuration) and from the scipy matrix (the CSR path)."""
    from mobgt_amd.model_fqandtoyo import Graphormer
    uni, coords = universe()
    g = geo.radius_graph_host(coords, 3.0)
    args = dict(workloads.COMMON, n_layers=1, hidden_dim=128, dataset_name="foursquaregraph", ffn_dim=256)
    for kw, today, sparse, names in (
            ({}, g.to_scipy(), True, ("D_AX", "D_A_rowptr", "D_A_col", "D_A_val", "D_AT_rowptr", "D_AT_col", "D_AT_val")),
            (dict(gcn_dtype=torch.bfloat16), uni.graph_dist, False, ("D_AX", "D_A", "D_A_T", "D_mask", "D_mask_t", "D_scale"))):
        a = Graphormer(universe=dataclasses.replace(uni, graph_dist=g), **args, **kw)
        b = Graphormer(universe=dataclasses.replace(uni, graph_dist=today), **args, **kw)
        assert a.sparse_adj == b.sparse_adj == sparse
        same([getattr(a, n).float() if getattr(a, n).dtype == torch.bfloat16 else getattr(a, n) for n in names],
             [getattr(b, n).float() if getattr(b, n).dtype == torch.bfloat16 else getattr(b, n) for n in names])
    with pytest.raises(ValueError, match="'csr'"):
        Graphormer(universe=dataclasses.replace(uni, graph_dist=geo.radius_graph_host(coords, 3.0, forms=("mask",))), **args)
