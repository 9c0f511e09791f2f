"""The classifier head's and the loss kernels' C ABI (include/mobgt_hip.h: the six mobgt_skinny_linear_* training entries of
csrc/skinny.hip, mobgt_gradient_tail_loss and mobgt_cross_entropy of csrc/layer.hip) as plain Python callers over device tensors.
An operand may be a tensor, a raw address (int: the refusals pass misaligned ones) or None.  Every caller RETURNS the status code
(0 = launched); `_lib.check` is the caller's."""
from mobgt_amd import _lib
from mobgt_amd.ops import _stream

EBADDIM, EALIGN = (_lib.CONSTANTS["MOBGT_" + n] for n in ("EBADDIM", "EALIGN"))


def addr(t):
    if t is None:
        return None
    return t if isinstance(t, int) else t.data_ptr()


def fwd(x, w, b, y, G, K, V):
    return _lib.lib().mobgt_skinny_linear_fwd(addr(x), addr(w), addr(b), addr(y), G, K, V, _stream())


def bwd(dy, x, w, dx, dw, db, G, K, V):
    return _lib.lib().mobgt_skinny_linear_bwd(addr(dy), addr(x), addr(w), addr(dx), addr(dw), addr(db), G, K, V, _stream())


def dx(dy, w, dx_, G, K, V):
    return _lib.lib().mobgt_skinny_linear_dx(addr(dy), addr(w), addr(dx_), G, K, V, _stream())


def bwd_both(dy, x, w, dx_, dw, db, G, K, V):
    return _lib.lib().mobgt_skinny_linear_bwd_both(addr(dy), addr(x), addr(w), addr(dx_), addr(dw), addr(db), G, K, V, _stream())


def fwd_mfma(x, w, b, y, G, K, V):
    return _lib.lib().mobgt_skinny_linear_fwd_mfma(addr(x), addr(w), addr(b), addr(y), G, K, V, _stream())


def gtl(x, w, b, targets, target_offset, logits, dlogits, loss, G, K, V, alpha):
    return _lib.lib().mobgt_skinny_linear_gtl(addr(x), addr(w), addr(b), addr(targets), int(target_offset), addr(logits),
                                              addr(dlogits), addr(loss), G, K, V, float(alpha), _stream())


def gradient_tail_loss(logits, targets, target_offset, dlogits, loss, G, V, alpha):
    return _lib.lib().mobgt_gradient_tail_loss(addr(logits), addr(targets), int(target_offset), addr(dlogits), addr(loss), G, V,
                                               float(alpha), _stream())


def cross_entropy(logits, targets, ignore_index, dlogits, loss, G, V):
    return _lib.lib().mobgt_cross_entropy(addr(logits), addr(targets), int(ignore_index), addr(dlogits), addr(loss), G, V, _stream())
