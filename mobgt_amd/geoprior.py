"""A fitted distance-decay curve as a prior on a model's next-POI scores: how much more often than chance a train transition lands
in each distance bin, as one f32 table over the bins of a geo.PairBins, added to the [G, V] scores that Graphormer.metric_step /
recommend_step rank -- on the device, in one launch (csrc_geoprior/geoprior.hip through _geoprior), inside the loops' captured
graphs.  The count terms of prior.MarkovPrior score a POI the anchor never led to by popularity only; this term tells a venue
300 m away from one 40 km away.

Inputs.  A fitted data.MarkovBaseline `mb`, whose transition CSR mb.graph (rowptr, col, val) is counted over the TRAIN sessions
only, and a geo.PairBins `pb` of the same P POIs: unit f64 [P, 3] and thresholds f64 [nthr], non-decreasing,
MOBGT_BINS_MIN_THRESHOLDS <= nthr <= MOBGT_BINS_MAX_THRESHOLDS.

Bin of a pair.  For 0-based POIs i, j:  bin(i, j) = #{k : thresholds[k] <= c2(i, j)}, in 0 .. nthr, with c2 the squared chord of
include/mobgt_bins.h bit for bit (geo._chord2_rows_host here, bins_search.h's chord2 and count_thresholds on the device, built
with -ffp-contract=off).  B = nthr + 1 is the number of bins.

Fit: two exact integer histograms, int64 [B].

    n[b] = the number of ORDERED pairs (i, j) in [0, P)^2, the diagonal included, with bin(i, j) = b      sum(n) = P^2
    t[b] = the sum of val[e] over the CSR entries e of row a with bin(a, col[e]) = b                       sum(t) = sum(val)

n is the multiset geo.chord2_order_stats defines.  Both see the train sessions only where they see sessions at all (n sees none).

Table.  table[b] = f32( log((t[b] + 1) / (T + B)) - log((n[b] + 1) / (N + B)) ), T = sum(t), N = sum(n): the log of how much more
often than chance a transition lands in bin b; the add-one terms keep empty bins finite.  It is evaluated in numpy float64 on the
host and rounded once (table_from_counts); the same f32 table is uploaded for the device and kept for the host, so both forms
hold the same bits: no transcendental runs in a kernel.

Blend.  Row g of the scores has the history ids hist[g, 0:n] (Restriction.hist(batch): the trajectory's nodes, 0 = padding).
  * The anchor a is the LAST entry of hist[g] that is not 0 -- MarkovPrior's anchor, the one near="last" documents: the last
    history check-in for graphs made from sessions (nodes ordered by their last visit), not necessarily for a hand-made dict.
    An id outside 1 .. P means no anchor and is never used as an index.
  * Column c is POI p = c + label_offset (model.label_offset).
  * Where a exists and 1 <= p <= P:   out[g, c] = s + w * table[bin(a - 1, p - 1)],   the product and the sum each rounded to
    f32 on their own, no FMA.  Every other element is copied bit for bit: -0.0, NaN payloads and -inf survive.  A term with
    weight 0 is still added (x + 0 * table[.]: a score of -0.0 becomes +0.0 where the table entry is not negative, and
    nothing else changes).
  * w is ONE f32 weight ("distance"), read from device memory: `prior.weights`, f32 [1]; set_weights copies into it, so a captured
    graph that blends stays valid when the weight changes.

`pair_hist_host`, `csr_hist_host`, `table_from_counts` and `blend_host` are this rule in numpy: the kernels' references and the CPU
forms.  prior.Stack(mb.prior(), mb.distance_prior(pb)) blends both priors, one launch each."""
import collections

import numpy as np
import torch

from . import _geoprior
from .geo import PairBins, _checked_thresholds, _chord2_rows_host, chord2_to_km
from .prior import Prior, check_weights

WEIGHTS = ("distance",)                                                 # the order of a weights row
SBADINDEX = _geoprior.SBADINDEX

DistanceTables = collections.namedtuple("DistanceTables", "unit thresholds table P")
DistanceTables.__doc__ = "numpy: unit f64 [P, 3], thresholds f64 [nthr], table f32 [nthr + 1]; int P"


def _bins_of(unit, thresholds):
    u = np.ascontiguousarray(unit, dtype=np.float64)
    if u.ndim != 2 or u.shape[1] != 3 or u.shape[0] < 1:
        raise ValueError(f"unit: expected [P >= 1, 3] f64 unit vectors, got shape {u.shape}")
    return u, _checked_thresholds(thresholds)


def pair_hist_host(unit, thresholds):
    """n of the module's docstring -> int64 [nthr + 1]: np.searchsorted(thresholds, c2, side="right") of all P^2 ordered pairs,
    counted row block by row block (never P x P at once)."""
    u, thr = _bins_of(unit, thresholds)
    P = u.shape[0]
    n = np.zeros(thr.size + 1, dtype=np.int64)
    step = max(1, 4_000_000 // P)
    for r0 in range(0, P, step):
        pos = np.searchsorted(thr, _chord2_rows_host(u, r0, r0 + step), side="right")
        n += np.bincount(pos.reshape(-1), minlength=n.size)
    return n


def csr_hist_host(unit, thresholds, rowptr, col, val, status=None):
    """t of the module's docstring -> int64 [nthr + 1].  A row whose rowptr pair is descending or lies outside [0, nnz] is skipped,
    an entry of col outside [0, P) is skipped; both OR SBADINDEX into status[0] (a list or an array)."""
    u, thr = _bins_of(unit, thresholds)
    P = u.shape[0]
    rowptr, col, val = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64), np.asarray(val, dtype=np.int64)
    nnz = col.size
    if rowptr.shape != (P + 1,) or val.shape != col.shape or col.ndim != 1:
        raise ValueError(f"csr: rowptr {rowptr.shape}, col {col.shape}, val {val.shape} for {P} POIs")
    r0, r1 = rowptr[:-1], rowptr[1:]
    ok = (r0 >= 0) & (r1 >= r0) & (r1 <= nnz)
    lens = np.where(ok, r1 - r0, 0)
    rows = np.repeat(np.arange(P, dtype=np.int64), lens)
    e = np.repeat(r0 - (np.cumsum(lens) - lens), lens) + np.arange(int(lens.sum()), dtype=np.int64)      # the entries, row by row
    q = col[e]
    good = (q >= 0) & (q < P)
    a, q, e = rows[good], q[good], e[good]
    dx, dy, dz = (u[a, k] - u[q, k] for k in range(3))                  # _chord2_rows_host's expression, pair by pair
    pos = np.searchsorted(thr, ((dx * dx) + (dy * dy)) + (dz * dz), side="right")
    t = np.zeros(thr.size + 1, dtype=np.int64)
    np.add.at(t, pos, val[e])
    if status is not None and not (ok.all() and good.all()):
        status[0] |= SBADINDEX
    return t


def table_from_counts(pair_counts, transition_counts):
    """-> f32 [B]: f32(log((t + 1) / (T + B)) - log((n + 1) / (N + B))), evaluated in float64 and rounded once."""
    n, t = np.asarray(pair_counts), np.asarray(transition_counts)
    if n.ndim != 1 or n.shape != t.shape or n.size < 1 or n.dtype.kind not in "iu" or t.dtype.kind not in "iu":
        raise ValueError(f"table_from_counts: two integer histograms of one length, got {n.dtype} {n.shape} and {t.dtype} {t.shape}")
    if (n < 0).any() or (t < 0).any():
        raise ValueError("table_from_counts: a count is negative")
    B = n.size
    N, T = int(n.sum(dtype=np.int64)), int(t.sum(dtype=np.int64))
    n, t = n.astype(np.float64), t.astype(np.float64)
    return (np.log((t + 1.0) / (float(T) + B)) - np.log((n + 1.0) / (float(N) + B))).astype(np.float32)


def blend_host(scores, hist, tables, weight, label_offset):
    """The blend of the module's docstring -> f32 numpy [G, V].  scores [G, V] f32; hist [G, n] integer ids; tables a
    DistanceTables; weight the one f32 weight (a number or a sequence of one)."""
    t = tables
    s = np.array(scores, dtype=np.float32)
    G, V = s.shape
    hist = np.asarray(hist).reshape(G, -1)
    w = np.float32(np.asarray(weight, dtype=np.float64).reshape(-1)[0])
    u, table = np.asarray(t.unit, dtype=np.float64), np.asarray(t.table, dtype=np.float32)
    P, lo = int(t.P), int(label_offset)
    c_lo, c_hi = max(0, 1 - lo), min(V, P + 1 - lo)                    # the columns whose POI is one of 1 .. P
    if c_hi <= c_lo:
        return s
    for g in range(G):
        ids = hist[g][hist[g] != 0]
        a = int(ids[-1]) if len(ids) else 0
        if not 1 <= a <= P:
            continue
        pos = np.searchsorted(t.thresholds, _chord2_rows_host(u, a - 1, a)[0, c_lo + lo - 1:c_hi + lo - 1], side="right")
        term = (w * table[pos]).astype(np.float32)                      # a product rounded to f32, then a sum rounded to f32
        s[g, c_lo:c_hi] = (s[g, c_lo:c_hi] + term).astype(np.float32)
    return s


def _hist_of(rows, G, what):
    """rows of blend -> hist [G, n] int32 / int64 with unit column stride (a batch, a (hist, user) pair, or hist itself)"""
    hist = rows if isinstance(rows, torch.Tensor) else rows[0] if isinstance(rows, (tuple, list)) else rows.x
    hist = hist.reshape(hist.shape[0], -1)
    if hist.shape[0] != G:
        raise ValueError(f"{what}: {G} rows of scores, {hist.shape[0]} of hist")
    if hist.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"{what}: hist must be int32 or int64 ids, got {hist.dtype}")
    return hist.contiguous() if hist.shape[1] and hist.stride(1) != 1 else hist


class DistancePrior(Prior):
    """The fitted table of the module's docstring on one device, its weight (distance) and a status word (prior.Prior).  tune is
    Prior's, as every prior's: a grid of [L, 1] rows is one weight swept.

    P                      the POIs, as the baseline's and the bins'
    pair_bins              the geo.PairBins it was fitted on (shared, not copied): unit, thresholds
    pair_counts            n, numpy int64 [B]
    transition_counts      t, numpy int64 [B]
    table                  f32 [B] on the device
    status                 the fit's csr_hist ORs SBADINDEX into it; the blend flags nothing

    rows of blend: a collated batch (hist = Restriction.hist(batch)), a (hist [G, n], user [G]) pair as MarkovPrior.blend takes it
    (the users are not read), or hist alone; int32 / int64.  The launch is mobgt_geoprior_blend_rows."""

    NAME, WEIGHTS, LIB = "DistancePrior", WEIGHTS, _geoprior
    SKIPPED = ("CSR rows or entries", "a rowptr pair was descending or beyond nnz, or an entry of col was outside [0, P) -- the "
               "tables are not what MarkovBaseline.fit makes")
    HINTS = ("fit the baseline and the bins on the loop's device", "the baseline was not fitted on the model's universe")

    def __init__(self, pair_bins, pair_counts, transition_counts, table, distance=1.0, status=None):
        self.pair_bins, self.P = pair_bins, int(pair_bins.P)
        self.pair_counts, self.transition_counts = pair_counts, transition_counts
        self._host_table = np.ascontiguousarray(table, dtype=np.float32)
        self.table = torch.from_numpy(self._host_table.copy()).to(self.device)
        super().__init__([distance], status)

    @property
    def device(self):
        return self.pair_bins.unit.device

    @classmethod
    def fit(cls, mb, pair_bins, distance=1.0):
        """Count n and t, make the table.  On a GPU: two launch sequences (mobgt_geoprior_pair_hist, mobgt_geoprior_csr_hist) on
        the baseline's own tensors, one read-back of the 2 B counts and the status word, the table in numpy, one upload.  A CPU
        baseline and CPU bins are counted by the host forms.  A status that is not zero (a CSR that MarkovBaseline.fit did not
        make) is a ValueError."""
        what = "DistancePrior.fit"
        weight = check_weights([distance], what, WEIGHTS)
        pb = pair_bins
        if not isinstance(pb, PairBins):
            raise TypeError(f"{what}: pair_bins must be a geo.PairBins (geo.pair_bins(coords, ...)), got {type(pb).__name__}")
        if int(pb.P) != int(mb.P):
            raise ValueError(f"{what}: the baseline was fitted on {mb.P} POIs, the bins hold {pb.P}: both must describe one universe")
        if pb.device != mb.device:
            raise ValueError(f"{what}: the baseline is on {mb.device}, the bins on {pb.device}: fit on one device "
                             "(PairBins.to(device), MarkovBaseline.fit(..., device=...))")
        P, nthr = int(pb.P), int(pb.thresholds.numel())
        if tuple(pb.unit.shape) != (P, 3) or pb.unit.dtype != torch.float64 or pb.thresholds.dtype != torch.float64 or pb.thresholds.dim() != 1:
            raise ValueError(f"{what}: the bins must hold unit f64 [{P}, 3] and thresholds f64 [nthr], got {pb.unit.dtype} "
                             f"{tuple(pb.unit.shape)} and {pb.thresholds.dtype} {tuple(pb.thresholds.shape)}")
        thr = _checked_thresholds(pb.thresholds.detach().cpu().numpy())  # the count, and that they never decrease
        g = mb.graph
        if g.val.dtype != torch.int32 or g.col.dtype != torch.int32 or g.rowptr.dtype != torch.int64 or g.rowptr.numel() != P + 1:
            raise ValueError(f"{what}: the baseline's CSR must be rowptr int64 [{P + 1}], col int32, val int32")
        if mb.device.type != "cuda":
            status = [0]
            n = pair_hist_host(pb.unit.numpy(), thr)
            t = csr_hist_host(pb.unit.numpy(), thr, g.rowptr.numpy(), g.col.numpy(), g.val.numpy(), status=status)
            word = torch.tensor(status, dtype=torch.int32)
        else:
            from .ops import _p, _stream
            unit, thresholds = pb.unit.contiguous(), pb.thresholds.contiguous()
            rowptr, col, val = g.rowptr.contiguous(), g.col.contiguous(), g.val.contiguous()
            with torch.cuda.device(mb.device):
                counts = torch.empty(2, nthr + 1, dtype=torch.int64, device=mb.device)
                word = torch.zeros(1, dtype=torch.int32, device=mb.device)
                _geoprior.launch("mobgt_geoprior_pair_hist", _p(unit), P, _p(thresholds), nthr, _p(counts[0]), _stream())
                _geoprior.launch("mobgt_geoprior_csr_hist", _p(unit), P, _p(thresholds), nthr, _p(rowptr), _p(col), _p(val),
                                 int(col.numel()), _p(counts[1]), _p(word), _stream())
                n, t = counts.cpu().numpy()
        cls.refuse(int(word[0]), what)                                   # (before the table: a broken CSR's counts mean nothing)
        if int(n.sum()) != P * P:
            raise RuntimeError(f"{what}: the pair histogram holds {int(n.sum())} pairs, {P} POIs have {P * P}")
        return cls(pb, n, t, table_from_counts(n, t), float(weight[0]), status=word)

    def tables(self):
        """-> DistanceTables: unit, thresholds and the table as numpy arrays (one download, kept), what blend_host takes."""
        if self._host_tables is None:
            n = lambda v: v.detach().cpu().numpy()
            self._host_tables = DistanceTables(n(self.pair_bins.unit), n(self.pair_bins.thresholds), self._host_table, self.P)
        return self._host_tables

    def curve(self):
        """-> (upper edges km f64 [B], n int64 [B], t int64 [B], table f32 [B]) for inspection: bin b holds the pairs with
        thresholds[b - 1] <= c2 < thresholds[b], so its upper edge is thresholds[b] as a great-circle distance, inf for the last."""
        thr = self.tables().thresholds
        return np.append(chord2_to_km(thr), np.inf), self.pair_counts, self.transition_counts, self._host_table

    _rows = staticmethod(lambda rows, G, what: (("hist", _hist_of(rows, G, what)),))

    def _blend_host(self, scores, ids, w, label_offset):
        return blend_host(scores, ids[0], self.tables(), w, label_offset)

    def _launch(self, head, ids, w, _p, code, stream):
        pb = self.pair_bins
        _geoprior.launch("mobgt_geoprior_blend_rows", *head, _p(pb.unit), self.P, _p(pb.thresholds), int(pb.thresholds.numel()),
                         _p(self.table), _p(w), stream)
