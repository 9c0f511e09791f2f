"""The chain kernels' C ABI (include/mobgt_hip.h: mobgt_pack_mfma_b, mobgt_layer_chain_fwd / _bwd / _bwd_preln / _bwd_big) as plain
Python callers over dicts of device tensors -- one copy of the 40-argument ctypes calls for the tests that go through `_lib`.
Every caller RETURNS the status code (0 = launched); `_lib.check` is the caller's."""
import ctypes

import torch

from mobgt_amd import _lib
from mobgt_amd.ops import _p, _stream

EBADDIM, EALIGN = _lib.CONSTANTS["MOBGT_EBADDIM"], _lib.CONSTANTS["MOBGT_EALIGN"]
SUM_NAMES = ("dnxw", "dnxb", "db2", "dn1w", "dn1b", "dbo")


def pack(w, transposed=False):
    """bf16 [N, K] -> MFMA operand order; transposed: w is [K, N] and its transpose is packed (the operand of dX = dY W)."""
    lib = _lib.lib()
    out = torch.empty(w.numel(), dtype=torch.bfloat16, device=w.device)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    N, K = (w.shape[1], w.shape[0]) if transposed else w.shape
    _lib.check(lib.mobgt_pack_mfma_b(1, (vp * 1)(w.data_ptr()), (vp * 1)(out.data_ptr()), (ci * 1)(N), (ci * 1)(K),
                                     (ci * 1)(1 if transposed else 0), _stream()), "mobgt_pack_mfma_b")
    return out


def _g(d, k):
    t = d.get(k)
    return _p(t) if t is not None else None


def chain_fwd(w, i, o, R, C, F, p, seed, seed_dev, ws, salt1=9, salt2=10):
    """w: packed wo, w1, w2, wq + bo, b1, b2, bq + n1w, n1b, nxw, nxb (wq / bq / nxw / nxb may be missing: null);  i: a, x;
    o: x1, z, u, h, x2, out, out_a, qkv, mean1, rstd1, mean2, rstd2 (missing: null)."""
    return _lib.lib().mobgt_layer_chain_fwd(
        _p(i["a"]), _p(i["x"]), _p(w["wo"]), _p(w["bo"]), _p(w["n1w"]), _p(w["n1b"]), _p(w["w1"]), _p(w["b1"]), _p(w["w2"]), _p(w["b2"]),
        _g(w, "nxw"), _g(w, "nxb"), _g(w, "wq"), _g(w, "bq"), _p(o["x1"]), _p(o["z"]), _p(o["u"]), _p(o["h"]), _p(o["x2"]), _g(o, "out"),
        _g(o, "out_a"), _g(o, "qkv"), _p(o["mean1"]), _p(o["rstd1"]), _g(o, "mean2"), _g(o, "rstd2"), R, C, F, p, seed,
        _p(seed_dev) if seed_dev is not None else None, salt1, salt2, _p(ws) if ws is not None else None, _stream())


def _bwd_head(w, s, i, o):
    return (_p(i["dout"]), _p(s["x2"]), _p(s["x1"]), _p(s["u"]), _p(s["mean1"]), _p(s["rstd1"]), _g(s, "mean2"), _g(s, "rstd2"),
            _p(w["n1w"]), _g(w, "nxw"), _p(w["w2t"]), _p(w["w1t"]), _p(w["wot"]), _p(o["df"]), _p(o["du"]), _p(o["dy"]), _p(o["da"]),
            _p(o["dx1"])) + tuple(_p(o[k]) for k in SUM_NAMES)


def chain_bwd(w, s, i, o, R, C, F, p, seed, seed_dev, ws, passengers=(), preln=False, salt1=9, salt2=10, n_wg=None):
    """mobgt_layer_chain_bwd (preln: _bwd_preln).  w: packed transposes w2t, w1t, wot (+ wqt for a tail) + n1w, nxw;  s: the saved x1,
    x2, u, mean1, rstd1, mean2, rstd2;  i: dout (+ dqkv: the tail);  o: df, du, dy, da, dx1 and the six sums;  passengers: dicts
    g [R, M] (ldg), x [R, N] (ldx), dw [M, N] (ldw), db [M] or None."""
    lib = _lib.lib()
    n = len(passengers) if n_wg is None else n_wg
    vp, i64, ci = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    m = max(1, len(passengers))
    arr = lambda t, f: (t * m)(*[f(q) for q in passengers])                     # noqa: E731
    wg = ((arr(vp, lambda q: q["g"].data_ptr()), arr(i64, lambda q: q["g"].stride(0)), arr(vp, lambda q: q["x"].data_ptr()),
           arr(i64, lambda q: q["x"].stride(0)), arr(vp, lambda q: q["dw"].data_ptr()), arr(i64, lambda q: q["dw"].stride(0)),
           arr(vp, lambda q: q["db"].data_ptr() if q.get("db") is not None else 0), arr(ci, lambda q: q["dw"].shape[0]),
           arr(ci, lambda q: q["dw"].shape[1])) if passengers else (None,) * 9)
    fn = lib.mobgt_layer_chain_bwd_preln if preln else lib.mobgt_layer_chain_bwd
    tail = i.get("dqkv") is not None
    return fn(*_bwd_head(w, s, i, o), R, C, F, p, seed, _p(seed_dev) if seed_dev is not None else None, salt1, salt2,
              _p(i["dqkv"]) if tail else None, _p(w["wqt"]) if tail else None, n, *wg, _p(ws) if ws is not None else None, _stream())


def chain_bwd_big(w, s, i, o, R, C, F, p, seed, seed_dev, salt1=9, salt2=10):
    """mobgt_layer_chain_bwd_big: as chain_bwd without passengers and workspace; o["db1"] [F] (missing: null)."""
    tail = i.get("dqkv") is not None
    return _lib.lib().mobgt_layer_chain_bwd_big(*_bwd_head(w, s, i, o), _g(o, "db1"), R, C, F, p, seed,
                                                _p(seed_dev) if seed_dev is not None else None, salt1, salt2,
                                                _p(i["dqkv"]) if tail else None, _p(w["wqt"]) if tail else None, _stream())
