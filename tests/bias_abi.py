"""The bias assembly's C ABI (include/mobgt_hip.h: mobgt_bias_pack, mobgt_build_bias, mobgt_build_bias_bwd,
mobgt_build_bias_bwd_set_workgroups, mobgt_front_sgemm_job / _pending, mobgt_small_gcn_bwd_bias with its bias passenger) as plain
Python callers over dicts of device tensors.  Every caller RETURNS the status code (0 = launched); `_lib.check` is the caller's.

i: attn_bias [G,T,T] f32, rel_pos, poi_pos (or None) [G,N,N], edge_input [G,N,N,D_in,F] (or None), rel_table, poi_table, hop_table,
   vdist;  o: bias, bias_t (or None) [G,H,T,ld];  g: dbias (f32 [G,H,T,ld] or bf16 slices), d_rel, d_poi, d_hop, d_vdist.
dims: dict G, N, H, D_in, D, F, n_rel, n_poi, n_edge, ld.  Dtype codes are passed as given, so that a test can pass a wrong one."""
from mobgt_amd import _lib
from mobgt_amd.ops import _p, _stream

EBADDIM, EALIGN, EDTYPE = (_lib.CONSTANTS[k] for k in ("MOBGT_EBADDIM", "MOBGT_EALIGN", "MOBGT_EDTYPE"))
F32, BF16, I64, I32, I16, U8 = _lib.F32, _lib.BF16, _lib.I64, _lib.I32, _lib.I16, _lib.U8
_DIMS = ("G", "N", "H", "D_in", "D", "F", "n_rel", "n_poi", "n_edge", "ld")


def _g(d, k):
    t = d.get(k)
    return _p(t) if t is not None else None


def bias_pack(src, src_dtype, strides, bias, bias_t, bias_dtype, G, H, T, ld):
    """strides: (s_g, s_h, s_i, s_j) in elements of src."""
    return _lib.lib().mobgt_bias_pack(_p(src), src_dtype, *[int(v) for v in strides], _p(bias), _p(bias_t) if bias_t is not None else None,
                                      bias_dtype, G, H, T, ld, _stream())


def build_bias(i, o, dims, idx_dtype, edge_dtype, bias_dtype):
    return _lib.lib().mobgt_build_bias(_p(i["attn_bias"]), _p(i["rel_pos"]), _g(i, "poi_pos"), _g(i, "edge_input"), _p(i["rel_table"]),
                                       _g(i, "poi_table"), _g(i, "hop_table"), _p(i["vdist"]), _p(o["bias"]), _g(o, "bias_t"),
                                       *[int(dims[k]) for k in _DIMS], idx_dtype, edge_dtype, bias_dtype, _stream())


def _bwd_args(i, g, dims, dbias_dtype, n_slices, slice_stride, idx_dtype, edge_dtype):
    return (_p(g["dbias"]), dbias_dtype, int(n_slices), int(slice_stride), _p(i["attn_bias"]), _p(i["rel_pos"]), _g(i, "poi_pos"),
            _g(i, "edge_input"), _p(g["d_rel"]), _g(g, "d_poi"), _g(g, "d_hop"), _p(g["d_vdist"]), *[int(dims[k]) for k in _DIMS],
            idx_dtype, edge_dtype)


def build_bias_bwd(i, g, dims, dbias_dtype, n_slices, slice_stride, idx_dtype, edge_dtype):
    return _lib.lib().mobgt_build_bias_bwd(*_bwd_args(i, g, dims, dbias_dtype, n_slices, slice_stride, idx_dtype, edge_dtype), _stream())


def set_workgroups(n):
    return _lib.lib().mobgt_build_bias_bwd_set_workgroups(int(n))


def front_sgemm_job(a, b, bias, leaky, slope, c, M, N, K, k_b):
    """a = None drops a pending job."""
    if a is None:
        return _lib.lib().mobgt_front_sgemm_job(None, 0, None, 0, None, 0, 0.0, None, 0, None, 0, 0, 0, 0, 0)
    return _lib.lib().mobgt_front_sgemm_job(_p(a), a.stride(0), _p(b), b.stride(0), _p(bias) if bias is not None else None, int(leaky),
                                            float(slope), _p(c), c.stride(0), None, 0, M, N, K, k_b)


def front_sgemm_pending():
    return _lib.lib().mobgt_front_sgemm_pending()


def small_gcn_bwd_bias(n_, w, i, g, dims, dbias_dtype, n_slices, slice_stride, idx_dtype, edge_dtype, with_bias=1):
    """n_: dict n, K0, H1, H2, H3;  w: the category GCN's side of the launch -- g [n,H3], ax [n,K0], a_t [n,n], w1 [H1,H2], w2 [H2,H3],
    h1, t [n,H1], h2, t2 [n,H2], dw0, db0, dw1, db1, dw2, db2, dt2 [n,H2], dt [n,H1], counter [4] (zeros)."""
    names = ("g", "ax", "a_t", "w1", "w2", "h1", "t", "h2", "t2", "dw0", "db0", "dw1", "db1", "dw2", "db2", "dt2", "dt", "counter")
    return _lib.lib().mobgt_small_gcn_bwd_bias(*[_p(w[k]) for k in names], n_["n"], n_["K0"], n_["H1"], n_["H2"], n_["H3"], 0.01, 0.0, 0,
                                               None, 0, int(with_bias),
                                               *_bwd_args(i, g, dims, dbias_dtype, n_slices, slice_stride, idx_dtype, edge_dtype),
                                               _stream())
