"""Device-side helpers shared by the kernel matrices (tests/test_gpu_maskgemm_matrix.py, tests/test_gpu_gcn_matrix.py): staging
of NumPy operands, destinations inside sentinel-filled guard buffers, strided operands inside wider buffers of 1000s."""
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
