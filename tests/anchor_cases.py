"""History rows for the anchor search that the three blend_rows kernels share (mobgt_amd/csrc_prior/blend_rows.h): a workgroup of 256
threads, four waves of 64, thread t looking at the positions t, t + 256, ...  The widths stand on either side of a wave and of
the workgroup; the rows place their ids so that the answer has to cross lanes, waves and strides."""
import numpy as np

G, V, LABEL_OFFSET = 4, 33, 1
WIDTHS = (0, 1, 63, 64, 65, 255, 256, 257, 600)


def positions(n):
    """-> (first, later) of the row with two ids: in different waves where the width has two (first in wave 0, later in the last
    one used), and beyond the workgroup in different strides, the later one in an EARLIER wave than the first -- so neither the
    larger lane nor the larger wave wins, only the larger position."""
    if n <= 256:
        return (63 if n > 64 else 0), n - 1                             # (n <= 64: one wave holds both, at its two ends)
    return 255, (n - 1) // 256 * 256 + min(10, (n - 1) % 256)           # wave 3 of stride 0; wave 0 of the last stride


def rows(n, first_id, later_id, dtype):
    """-> hist [4, n]: all zero; the only id at position 0; the only id at n - 1; first_id and later_id at positions(n)."""
    hist = np.zeros((G, n), dtype=dtype)
    if n:
        first, later = positions(n)
        hist[1, 0] = hist[2, n - 1] = later_id
        hist[3, first], hist[3, later] = first_id, later_id             # (n = 1: one position, the later id stands)
    return hist


def loser(hist):
    """hist with the deciding id of the last row removed: what a search that let the wrong position win would blend"""
    other = hist.copy()
    if hist.shape[1] > 1:
        other[3, positions(hist.shape[1])[1]] = 0
    return other
