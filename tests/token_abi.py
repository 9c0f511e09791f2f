"""The encoder-input kernels' C ABI (include/mobgt_hip.h: mobgt_assemble_tokens_fwd / _bwd / _qkv, mobgt_token_fwd_chain,
mobgt_token_bwd_chain, mobgt_embed_gather_multi) as plain Python callers over dicts of device tensors.  Every stride and leading
dimension is an argument; every caller RETURNS the status code (0 = launched); `_lib.check` is the caller's.  A missing dict entry
goes in as a null pointer."""
import ctypes

from chain_abi import pack                                       # noqa: F401  (the QKV weight's MFMA operand order)
from mobgt_amd import _lib
from mobgt_amd.ops import _stream

EBADDIM, EALIGN, EDTYPE = (_lib.CONSTANTS[k] for k in ("MOBGT_EBADDIM", "MOBGT_EALIGN", "MOBGT_EDTYPE"))
I64, I32, I16 = (_lib.CONSTANTS[k] for k in ("MOBGT_I64", "MOBGT_I32", "MOBGT_I16"))
SALTS = (0x1001, 0x1002, 0x1003)                                 # salt_nf, salt_tok, salt_in: the model's (ops.assemble_tokens)

_vp, _ci, _i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64


def ptr(t):
    """A device tensor, a raw address (int: deliberately misaligned / null pointers) or None."""
    if t is None:
        return _vp(0)
    return _vp(t if isinstance(t, int) else t.data_ptr())


def _g(d, k):
    return ptr(d.get(k))


def _tail(G, N, C, p_pos, p_in, seed, seed_dev, salts):
    return (G, N, C, float(p_pos), float(p_in), int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(seed_dev), salts[0], salts[1], salts[2], _stream())


def assemble_fwd(i, o, G, N, C, p_pos=0.0, p_in=0.0, seed=0, seed_dev=None, salts=SALTS):
    """i: nf, real, add, token, pe0;  o: out (+ out16)."""
    return _lib.lib().mobgt_assemble_tokens_fwd(_g(i, "nf"), _g(i, "real"), _g(i, "add"), _g(i, "token"), _g(i, "pe0"), _g(o, "out"),
                                                _g(o, "out16"), *_tail(G, N, C, p_pos, p_in, seed, seed_dev, salts))


def assemble_bwd(i, o, G, N, C, p_pos=0.0, p_in=0.0, seed=0, seed_dev=None, salts=SALTS):
    """i: dout, real;  o: d_nf, d_add, d_token."""
    return _lib.lib().mobgt_assemble_tokens_bwd(_g(i, "dout"), _g(i, "real"), _g(o, "d_nf"), _g(o, "d_add"), _g(o, "d_token"),
                                                *_tail(G, N, C, p_pos, p_in, seed, seed_dev, salts))


def assemble_qkv(i, o, G, N, C, p_pos=0.0, p_in=0.0, seed=0, seed_dev=None, salts=SALTS):
    """i: nf, real, add, token, pe0, wq (packed), bq;  o: out, out16, qkv."""
    return _lib.lib().mobgt_assemble_tokens_qkv(_g(i, "nf"), _g(i, "real"), _g(i, "add"), _g(i, "token"), _g(i, "pe0"), _g(o, "out"),
                                                _g(o, "out16"), _g(i, "wq"), _g(i, "bq"), _g(o, "qkv"),
                                                *_tail(G, N, C, p_pos, p_in, seed, seed_dev, salts))


def _jobs(jobs, *fields):
    """jobs: dicts with table / d_table / idx / buf (tensor, int address or None), width, coff, accum, slot, skip, ld."""
    n = max(1, len(jobs))
    out = []
    for f in fields:
        if f in ("table", "d_table", "idx", "buf"):
            out.append((_vp * n)(*[ptr(j.get(f)).value or 0 for j in jobs]))
        elif f in ("skip", "ld"):
            out.append((_i64 * n)(*[int(j.get(f, -1 if f == "skip" else 0)) for j in jobs]))
        else:
            out.append((_ci * n)(*[int(j.get(f, 0)) for j in jobs]))
    return out


def token_fwd_chain(jobs, i, o, G, N, C=192, W2=160, idx_dtype=I64, slope2=0.2, slope4=0.2, p_pos=0.0, p_in=0.0, seed=0, seed_dev=None,
                    salts=SALTS, n=None):
    """jobs: table, idx, width, coff, accum, slot;  i: w2, b2, w4, b4, real, token, pe0, wq (packed), bq;
    o: pt, x4, add, nf, out, out16, qkv."""
    tables, idx, width, coff, accum, slot = _jobs(jobs, "table", "idx", "width", "coff", "accum", "slot")
    return _lib.lib().mobgt_token_fwd_chain(
        len(jobs) if n is None else n, tables, idx, width, coff, accum, slot, idx_dtype, _g(o, "pt"), _g(o, "x4"), _g(o, "add"),
        _g(o, "nf"), W2, _g(i, "w2"), _g(i, "b2"), float(slope2), _g(i, "w4"), _g(i, "b4"), float(slope4), _g(i, "real"),
        _g(i, "token"), _g(i, "pe0"), _g(o, "out"), _g(o, "out16"), _g(i, "wq"), _g(i, "bq"), _g(o, "qkv"),
        *_tail(G, N, C, p_pos, p_in, seed, seed_dev, salts))


def token_bwd_chain(i, o, G, N, ld_y2, ld_dx4, C=192, W2=160, slope4=0.2, slope2=0.2, p_pos=0.0, p_in=0.0, seed=0, seed_dev=None,
                    salts=SALTS):
    """i: dout, real, y4, y2 (row stride ld_y2), w4, w2;  o: d_nf, d_add, dx4 (row stride ld_dx4), d_pt, d_token."""
    return _lib.lib().mobgt_token_bwd_chain(
        _g(i, "dout"), _g(i, "real"), _g(i, "y4"), _g(i, "y2"), ld_y2, _g(i, "w4"), _g(i, "w2"), _g(o, "d_nf"), _g(o, "d_add"),
        _g(o, "dx4"), ld_dx4, _g(o, "d_pt"), _g(o, "d_token"), G, N, C, W2, float(slope4), float(slope2), float(p_pos), float(p_in),
        int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(seed_dev), salts[0], salts[1], salts[2], _stream())


def gather_multi(jobs, R, idx_dtype=I64, backward=False, extra_row0=None, extra_job=0, tables=True, n=None):
    """jobs: table (forward) / d_table (backward; None: that table gets no gradient), idx, skip, width, coff, accum, buf, ld.
    tables=False passes a null `tables` array (what a backward call may do)."""
    tab, dtab, idx, skip, width, coff, accum, buf, ld = _jobs(jobs, "table", "d_table", "idx", "skip", "width", "coff", "accum", "buf", "ld")
    return _lib.lib().mobgt_embed_gather_multi(len(jobs) if n is None else n, tab if tables else None, dtab if backward else None, idx,
                                               skip, width, coff, accum, buf, ld, R, idx_dtype, 1 if backward else 0,
                                               ptr(extra_row0), extra_job, _stream())
