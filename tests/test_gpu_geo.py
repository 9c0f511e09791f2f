"""The within-radius POI graph on the device (csrc_geo/radius.hip through mobgt_amd.geo) against `geo.radius_graph_host`, exactly:
every input is first checked on the CPU to keep every pair 1e-6 km away from the radius and from distance zero
(geo_cases.assert_margin), so the two f64 evaluations of the rule cannot disagree.  Shapes: the word (32), word-group (128) and
column-tile (2048) edges, and a 5000-POI city.  Inputs hold isolated POIs, exact duplicates, the pole and a pair across +-180."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

import geo_cases
from mobgt_amd import _lib_geo, geo, synth, workloads
from mobgt_amd.ops import _p, _stream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = (1, 2, 31, 32, 33, 127, 128, 129, 2049, 5000)
C2 = geo.chord2_max(geo_cases.RADIUS_KM)


def poisoned(shape, dtype):
    """Every byte 0xFF."""
    return torch.full(shape, -1, dtype=torch.int64 if dtype == torch.int64 else torch.int32, device=DEV).view(dtype)


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def same(got, want):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape, (k, a.dtype, b.dtype, a.shape, b.shape)
        assert torch.equal(bits(a.cpu()), bits(b.cpu())), k


def unpack(words, P):
    """int32 [P, W] -> bool [P, W * 32], little-endian bits."""
    return np.unpackbits(np.ascontiguousarray(words.cpu().numpy()).view(np.uint8), axis=1, bitorder="little").astype(bool)


@pytest.mark.parametrize("P", SHAPES)
def test_every_entry_point_equals_the_host_graph(P):
    c, ref = geo_cases.reference(P)
    unit = geo.unit_vectors(torch.tensor(c, device=DEV))
    # (not part of the exact comparison: sin and cos of two libraries, each within 2 ulp of values <= 1, and one product)
    assert np.abs(unit.cpu().numpy() - geo.unit_vectors_host(c)).max() <= 5 * np.finfo(np.float64).eps

    W = geo.mask_pitch(P)
    words, deg = geo.radius_words(unit, C2, poisoned((P, W), torch.int32), poisoned((P,), torch.int32))
    assert torch.equal(words.cpu(), ref.words) and torch.equal(deg.cpu(), ref.deg)
    b = unpack(words, P)
    assert not b[:, P:].any()                                          # the poison is gone from the padding too
    assert np.array_equal(b[:, :P], b[:, :P].T) and b[:, :P].diagonal().all()
    assert np.array_equal(b.sum(axis=1) - 1, deg.cpu().numpy())

    deg2 = geo.radius_count(unit, C2, poisoned((P,), torch.int32))     # the path that stores nothing of size P^2
    assert torch.equal(deg2, deg)
    rowptr = geo.row_offsets(deg2)
    nnz = int(rowptr[-1])
    assert torch.equal(rowptr.cpu(), ref.rowptr) and nnz == ref.col.numel()
    col, val = geo.radius_fill(unit, C2, rowptr, poisoned((nnz,), torch.int32), poisoned((nnz,), torch.float32))
    assert torch.equal(col.cpu(), ref.col) and torch.equal(bits(val.cpu()), bits(ref.val))
    col_np, rp = col.cpu().numpy(), rowptr.cpu().numpy()
    inner = np.ones(nnz, dtype=bool)
    inner[rp[:-1]] = False                                             # (every row has its diagonal: no empty row)
    assert (np.diff(col_np)[inner[1:]] > 0).all()                      # strictly ascending inside every row
    from_csr = np.zeros((P, P), dtype=bool)
    from_csr[np.repeat(np.arange(P), np.diff(rp)), col_np] = True
    assert np.array_equal(from_csr, b[:, :P])                          # CSR and words: one graph
    assert torch.equal(bits(val), bits(torch.repeat_interleave((1.0 / (deg.double() + 1.0)).float(), deg.long() + 1)))


@pytest.mark.parametrize("P", (129, 2049))
def test_radius_graph_forms_agree(P):
    c, ref = geo_cases.reference(P)
    both = geo.radius_graph(c, geo_cases.RADIUS_KM, device=DEV)
    csr = geo.radius_graph(c, geo_cases.RADIUS_KM, device=DEV, forms=("csr",))
    mask = geo.radius_graph(c, geo_cases.RADIUS_KM, device=DEV, forms=("mask",))
    assert both.forms == ("mask", "csr") and csr.forms == ("csr",) and mask.forms == ("mask",)
    assert csr.words is None and mask.col is None and both.deg.is_cuda and both.deg.dtype == torch.int32
    same((csr.deg, csr.rowptr, csr.col, csr.val), (both.deg, both.rowptr, both.col, both.val))
    same((mask.deg, mask.words), (both.deg, both.words))
    same(both.mask_adj(), ref.mask_adj())                              # == MaskAdj.from_dense01 (test_host_geo.py)
    same(both.csr_adj(), ref.csr_adj())                                # == CsrAdj.from_scipy of model_fqandtoyo's a_hat
    assert both.mask_adj()[1] is both.mask_adj()[0]
    want = ref.to_dense01()
    for g in (both, csr, mask):                                        # the host copies, from whichever form there is
        assert np.array_equal(g.to_dense01(), want) and (g.to_scipy() != ref.to_scipy()).nnz == 0
    padded = np.concatenate([np.zeros((1, 2)), c])                     # the [P + 1, 2] table of DeviceCollator(coords=)
    same((geo.radius_graph(padded, geo_cases.RADIUS_KM, device=DEV, forms=("csr",), pad_row=True).col,), (both.col,))
    geo_cases.assert_margin(c, 1.0)                                    # another radius, coordinates as a tensor
    same((geo.radius_graph(torch.tensor(c), 1.0, device=DEV).words,), (geo.radius_graph_host(c, 1.0).words,))


def test_bad_arguments_are_refused_before_any_launch():
    c, ref = geo_cases.reference(33)
    unit = geo.unit_vectors(torch.tensor(c, device=DEV))
    deg = torch.zeros(33, dtype=torch.int32, device=DEV)
    words = torch.zeros(33, 4, dtype=torch.int32, device=DEV)
    null, c2 = ctypes.c_void_p(0), ctypes.c_double(C2)
    odd = ctypes.c_void_p(unit.data_ptr() + 4)                         # f64 data at a 4-byte boundary
    for code, name, args in (
            (_lib_geo.EBADDIM, "mobgt_geo_unit_vectors", (_p(unit), _p(unit), 0, _stream())),
            (_lib_geo.EBADDIM, "mobgt_geo_radius_words", (_p(unit), 0, c2, _p(words), _p(deg), _stream())),
            (_lib_geo.EBADDIM, "mobgt_geo_radius_count", (_p(unit), -5, c2, _p(deg), _stream())),
            (_lib_geo.EBADDIM, "mobgt_geo_radius_fill", (_p(unit), _lib_geo.MAX_P + 1, c2, _p(deg), _p(deg), _p(deg), _stream())),
            (_lib_geo.EALIGN, "mobgt_geo_unit_vectors", (null, _p(unit), 33, _stream())),
            (_lib_geo.EALIGN, "mobgt_geo_radius_words", (_p(unit), 33, c2, null, _p(deg), _stream())),
            (_lib_geo.EALIGN, "mobgt_geo_radius_count", (odd, 33, c2, _p(deg), _stream())),
            (_lib_geo.EALIGN, "mobgt_geo_radius_fill", (_p(unit), 33, c2, null, _p(deg), _p(deg), _stream()))):
        with pytest.raises(_lib_geo.MobgtGeoError, match="MOBGT_GEO_E") as e:
            _lib_geo.launch(name, *args)
        assert e.value.code == code, (name, e.value.code)
    rowptr = ref.rowptr.to(DEV)
    nnz = int(rowptr[-1])
    col, val = torch.zeros(nnz, dtype=torch.int32, device=DEV), torch.zeros(nnz, dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError, match="rowptr ends at"):            # a col buffer sized from another rowptr
        geo.radius_fill(unit, C2, rowptr + torch.arange(34, device=DEV), col, val)
    with pytest.raises(ValueError, match="rowptr ends at"):
        geo.radius_fill(unit, C2, rowptr, col, val[:-1])
    shuffled = rowptr.clone()
    shuffled[5], shuffled[6] = rowptr[6] + 9, rowptr[5]
    with pytest.raises(ValueError, match="not the prefix sum"):
        geo.radius_fill(unit, C2, shuffled, col, val)
    with pytest.raises(ValueError, match="not the prefix sum"):
        geo.radius_fill(unit, C2, rowptr + 1, col, val)
    with pytest.raises(ValueError, match="expected a contiguous"):
        geo.radius_words(unit, C2, words[:, :3], deg)
    assert not col.any() and not val.any() and not words.any()         # nothing was launched
    torch.cuda.synchronize()


def _models(uni, graph_a, graph_b, **kw):
    from mobgt_amd.model_fqandtoyo import Graphormer
    args = dict(workloads.COMMON, n_layers=1, hidden_dim=128, dataset_name="foursquaregraph", ffn_dim=256)
    out = []
    for graph in (graph_a, graph_b):
        torch.manual_seed(4)
        out.append(Graphormer(universe=dataclasses.replace(uni, graph_dist=graph), **args, **kw).to(DEV).eval())
    return out


def _same_buffers(a, b, names):
    for name in names:
        ta, tb = getattr(a, name), getattr(b, name)
        assert ta is not None and ta.is_cuda and ta.dtype == tb.dtype and ta.shape == tb.shape, name
        raw = lambda t: t.contiguous().view(torch.int16) if t.dtype == torch.bfloat16 else bits(t)
        assert torch.equal(raw(ta), raw(tb)), name


def test_graphormer_takes_the_graph_from_the_device():
    from mobgt_amd.modelGNN import CsrAdj, MaskAdj
    P = 300
    uni = synth.make_universe(P=P, n_cat=8, n_user=8, seed=0)
    coords = uni.poi_table[:, 2:4]
    geo_cases.assert_margin(coords)
    g = geo.radius_graph(coords, 3.0, device=DEV)
    assert np.array_equal(g.to_dense01(), uni.graph_dist)
    rows = (torch.arange(64, dtype=torch.int64, device=DEV) * 7) % P

    sparse_g, sparse_h = _models(uni, g, g.to_scipy())                 # f32 GCN: the CSR path (csrc/spmm.hip)
    assert sparse_g.sparse_adj and sparse_h.sparse_adj
    csr_names = ("D_AX", "D_A_rowptr", "D_A_col", "D_A_val", "D_AT_rowptr", "D_AT_col", "D_AT_val")
    _same_buffers(sparse_g, sparse_h, csr_names)
    assert sparse_g.D_A_col.data_ptr() == g.col.data_ptr()             # registered as it lies on the device
    with torch.no_grad():
        for r in (None, rows):
            out = [m.poi_distance_model(m.X, CsrAdj(*[getattr(m, n) for n in csr_names[1:]]), m.D_AX, rows=r)
                   for m in (sparse_g, sparse_h)]
            assert out[0].shape == (P if r is None else 64, 128) and torch.equal(bits(out[0]), bits(out[1]))

    mask_g, mask_h = _models(uni, g, g.to_dense01(), gcn_dtype=torch.bfloat16)      # bf16 GCN: the bitmask path (csrc/maskgemm.hip)
    assert not mask_g.sparse_adj and not mask_h.sparse_adj
    _same_buffers(mask_g, mask_h, ("D_AX", "D_A", "D_A_T", "D_mask", "D_mask_t", "D_scale"))
    assert mask_g.D_mask.data_ptr() == g.words.data_ptr()
    with torch.no_grad():
        for r in (None, rows):
            out = [m.poi_distance_model(m.X, m.D_A, m.D_AX, rows=r, adj_t=m.D_A_T, mask_adj=MaskAdj(m.D_mask, m.D_mask_t, m.D_scale),
                                        parts_ok=True) for m in (mask_g, mask_h)]
            assert out[0].shape[0] == (P if r is None else 64) and torch.equal(bits(out[0].float()), bits(out[1].float()))
    with pytest.raises(ValueError, match="'csr'"):                     # f32 GCN needs the CSR form
        _models(uni, geo.radius_graph(coords, 3.0, device=DEV, forms=("mask",)), g.to_scipy())
