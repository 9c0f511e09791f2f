"""Device-side helpers shared by the kernel matrices (tests/test_gpu_maskgemm_matrix.py, tests/test_gpu_gcn_matrix.py,
tests/test_gpu_spd_matrix.py): staging of NumPy operands, destinations inside sentinel-filled guard buffers (float matrices:
Guarded; integer arrays and bit patterns of any shape: GuardedFlat), strided operands inside wider buffers of 1000s."""
import numpy as np
import torch

DEV = "cuda"
SENT = -12345.0
BF, F32 = torch.bfloat16, torch.float32


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def opt(a):
    return dev(a) if a is not None else None


class Guarded:
    """A [rows, cols] f32 or bf16 destination inside a sentinel-filled buffer: `gr` guard rows above and below, `off` guard columns
    to the left and `pad` to the right.  `init`: the destination's contents on entry (default: the sentinel)."""

    def __init__(self, rows, cols, dtype=F32, off=0, pad=0, gr=2, init=None):
        self.ld = cols + off + pad
        self.box = (gr, gr + rows, off, off + cols)
        self.sent = torch.tensor(SENT, dtype=dtype, device=DEV)
        self.big = torch.full((rows + 2 * gr, self.ld), SENT, dtype=dtype, device=DEV)
        self.view = self.big[gr:gr + rows, off:off + cols]
        if init is not None:
            self.view.fill_(init)

    def result(self):
        """The destination on the host (f32 values, or uint16 patterns of a bf16 one); asserts that nothing outside was written."""
        r0, r1, c0, c1 = self.box
        out = self.view.contiguous().cpu()
        outside = self.big == self.sent
        outside[r0:r1, c0:c1] = True
        assert bool(outside.all()), "a guard row or column was written"
        return out.view(torch.int16).numpy().view(np.uint16) if out.dtype == BF else out.numpy()

    def untouched(self):
        return bool((self.big == self.sent).all())


# what no correct integer result holds; a float destination starts as a quiet NaN with a payload, compared as its int32 pattern
POISON = {torch.uint8: 0xA5, torch.int16: -12345, torch.int32: -1234567, torch.int64: -1234567, torch.float32: 0x7FC5A5A5}


class GuardedFlat:
    """`shape` elements of an integer dtype (or f32) inside a poison-filled 1-d buffer with `guard` elements on either side (a
    multiple of 16 bytes, so the view keeps the allocation's alignment).  `init`: a NumPy array the view starts as."""

    def __init__(self, shape, dtype, guard=64, init=None):
        self.shape = tuple(int(s) for s in np.atleast_1d(shape))
        self.count = int(np.prod(self.shape, dtype=np.int64))
        self.guard, self.dtype = guard, dtype
        self.raw = torch.int32 if dtype == F32 else dtype
        self.poison = POISON[dtype]
        self.buf = torch.full((self.count + 2 * guard,), self.poison, dtype=self.raw, device=DEV)
        self.view = self.buf[guard:guard + self.count]
        if init is not None:
            self.view.copy_(dev(np.ascontiguousarray(init).reshape(-1)).view(self.raw))

    def ptr(self):
        return self.view.data_ptr()

    def result(self):
        """The view on the host in its shape (a float view as int32 patterns); asserts that both guards still hold the poison."""
        b = self.buf.cpu().numpy()
        g = self.guard
        assert (b[:g] == self.poison).all(), "an element in front of the array was written"
        assert (b[g + self.count:] == self.poison).all(), "an element behind the array was written"
        return b[g:g + self.count].reshape(self.shape)

    def untouched(self):
        return bool((self.buf == self.poison).all())


def place(a, dtype=F32, off=4, pad=4, fill=1000.0, view=True):
    """(device tensor, leading dimension) of operand a [R, C]: columns off .. off + C of a wider buffer whose other columns hold
    `fill` -- a kernel that reads them is wrong by thousands."""
    R, C = a.shape
    if not view:
        return dev(a, dtype), C
    wide = torch.full((R, C + off + pad), fill, dtype=dtype, device=DEV)
    v = wide[:, off:off + C]
    v.copy_(dev(a, dtype))
    return v, C + off + pad
