"""The one-launch GCN's and the CSR adjacency product's C ABI (include/mobgt_hip.h: mobgt_small_gcn_fwd / _fwd_pack / _bwd /
_bwd_bias of csrc/smallgcn.hip, mobgt_spmm_csr / _t_rows / _t_rows_gather of csrc/spmm.hip) as plain Python callers over device
pointers.  Every size and leading dimension is an argument; an operand may be a tensor, a raw address (int: the refusals pass
misaligned ones) or None.  Every caller RETURNS the status code (0 = launched)."""
import ctypes

from mobgt_amd import _lib
from mobgt_amd.ops import _stream

EBADDIM, EALIGN = (_lib.CONSTANTS["MOBGT_" + n] for n in ("EBADDIM", "EALIGN"))
NO_NODE_INDEX = [0, None, 0, 0, 0, None, 0, 0, None, None, None, 0, None, None, 0, 0, 0]
NO_HOP = [0, None, None, None, 0, 0, 0, 0]
NO_BIAS = [0, None, 0, 1, 0] + [None] * 8 + [0] * 9 + [0, 0, 0]


def addr(t):
    if t is None:
        return None
    return t if isinstance(t, int) else t.data_ptr()


def _drop(seed, seed_dev, salt):
    return int(seed), addr(seed_dev), int(salt) & 0xFFFFFFFF


def small_gcn_fwd(ax, a, ws, outs, counter, n, K0, widths, slope, dropout_p, seed, seed_dev, salt):
    """ws = (w0, b0, w1, b1, w2, b2); outs = (h1, t, h2, t2, out); widths = (H1, H2, H3)."""
    return _lib.lib().mobgt_small_gcn_fwd(addr(ax), addr(a), *[addr(w) for w in ws], *[addr(o) for o in outs], addr(counter), n, K0,
                                          *widths, float(slope), float(dropout_p), *_drop(seed, seed_dev, salt), _stream())


def pack_arrays(jobs):
    """jobs: [(src bf16 [N, K] tensor, dst tensor, transposed)] -> the five arrays of mobgt_pack_mfma_b, after their count."""
    nj = len(jobs)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    N = [s.shape[1] if t else s.shape[0] for s, _, t in jobs]
    K = [s.shape[0] if t else s.shape[1] for s, _, t in jobs]
    return [nj, (vp * nj)(*[s.data_ptr() for s, _, _ in jobs]), (vp * nj)(*[d.data_ptr() for _, d, _ in jobs]), (ci * nj)(*N),
            (ci * nj)(*K), (ci * nj)(*[int(t) for _, _, t in jobs])]


def small_gcn_fwd_pack(ax, a, ws, outs, counter, n, K0, widths, slope, dropout_p, seed, seed_dev, salt, pack=None, node_index=None,
                       hop=None):
    """pack: pack_arrays(...) or None; node_index / hop: the argument lists of mobgt_node_index / mobgt_hop_table_fwd or None."""
    pack = pack if pack is not None else [0, None, None, None, None, None]
    ni = [1] + list(node_index) if node_index is not None else NO_NODE_INDEX
    hp = [1] + list(hop) if hop is not None else NO_HOP
    return _lib.lib().mobgt_small_gcn_fwd_pack(addr(ax), addr(a), *[addr(w) for w in ws], *[addr(o) for o in outs], addr(counter), n,
                                               K0, *widths, float(slope), float(dropout_p), *_drop(seed, seed_dev, salt), *pack, *ni,
                                               *hp, _stream())


def pack_mfma_b(pack):
    return _lib.lib().mobgt_pack_mfma_b(*pack, _stream())


def node_index(args):
    return _lib.lib().mobgt_node_index(*args, _stream())


def hop_table_fwd(args):
    return _lib.lib().mobgt_hop_table_fwd(*args, _stream())


def _bwd_args(g, ax, a_t, w1, w2, saved, grads, dt2, dt, counter, n, K0, widths, slope, dropout_p, seed, seed_dev, salt):
    return [addr(g), addr(ax), addr(a_t), addr(w1), addr(w2), *[addr(s) for s in saved], *[addr(x) for x in grads], addr(dt2),
            addr(dt), addr(counter), n, K0, *widths, float(slope), float(dropout_p), *_drop(seed, seed_dev, salt)]


def small_gcn_bwd(g, ax, a_t, w1, w2, saved, grads, dt2, dt, counter, n, K0, widths, slope, dropout_p, seed, seed_dev, salt):
    """saved = (h1, t, h2, t2); grads = (dw0, db0, dw1, db1, dw2, db2)."""
    return _lib.lib().mobgt_small_gcn_bwd(*_bwd_args(g, ax, a_t, w1, w2, saved, grads, dt2, dt, counter, n, K0, widths, slope, dropout_p,
                                                     seed, seed_dev, salt), _stream())


def small_gcn_bwd_bias(g, ax, a_t, w1, w2, saved, grads, dt2, dt, counter, n, K0, widths, slope, dropout_p, seed, seed_dev, salt,
                       bias=None):
    """bias: the 25 trailing arguments of the passenger (with_bias first) or None for none."""
    return _lib.lib().mobgt_small_gcn_bwd_bias(*_bwd_args(g, ax, a_t, w1, w2, saved, grads, dt2, dt, counter, n, K0, widths, slope,
                                                          dropout_p, seed, seed_dev, salt), *(bias if bias is not None else NO_BIAS),
                                               _stream())


def small_gcn_faults(reset=0):
    c = ctypes.c_uint32(0)
    _lib.check(_lib.lib().mobgt_small_gcn_faults(int(reset), ctypes.byref(c)), "mobgt_small_gcn_faults")
    return int(c.value)


def spmm_csr(rowptr, col, val, rows, b, ldb, bias, out, ld_out, R, C):
    return _lib.lib().mobgt_spmm_csr(addr(rowptr), addr(col), addr(val), addr(rows), addr(b), ldb, addr(bias), addr(out), ld_out, R, C,
                                     _stream())


def spmm_csr_t_rows(rowptr, col, val, rows, g, ldg, db, ld_db, R, C):
    return _lib.lib().mobgt_spmm_csr_t_rows(addr(rowptr), addr(col), addr(val), addr(rows), addr(g), ldg, addr(db), ld_db, R, C,
                                            _stream())


def spmm_csr_t_rows_gather(t_rowptr, t_col, t_val, rows, head, nxt, g, ldg, db, ld_db, P, R, C):
    return _lib.lib().mobgt_spmm_csr_t_rows_gather(addr(t_rowptr), addr(t_col), addr(t_val), addr(rows), addr(head), addr(nxt), addr(g),
                                                   ldg, addr(db), ld_db, P, R, C, _stream())
