"""The within-radius POI graph from coordinates: `graph_dist`, the 0/1 "within 3 km" matrix the distance GCN runs on.

The reference builds it with a Python double loop over all P^2 pairs (graphormer/foursquare_process.py:689-702, one LLs2Dist
call :15-23 per pair).  `radius_graph` decides the same pairs on the device (csrc_geo/radius.hip through _lib_geo) and leaves
the result there in the forms the GCN kernels read: the bit words of modelGNN.MaskAdj and the CSR of modelGNN.CsrAdj.
`radius_graph_host` is the same rule in numpy f64, blocked over rows: the CPU form and the tests' reference.

The rule (include/mobgt_geo.h): pair (i, j), i != j, is an edge iff 0 < |u_i - u_j|^2 <= 4 sin^2(r / 2R) in f64, u the unit
vectors of the two POIs, R = 6371 km.  It agrees with `0 < haversine <= r` except for pairs within rounding (~1e-9 km) of
the radius or of distance zero; POIs with identical coordinates are not neighbours, as in the reference.

The distance bins from coordinates: `poi_pos`, the distance-bin index of every POI pair.  The reference takes the
Freedman-Diaconis bin count from two percentiles and the maximum of a (P+1) x (P+1) f64 distance matrix (collator.py:301-308) and
digitizes the matrix against np.histogram's edges (collator.py:429-437).  `distance_bins` derives the same bin count, the same
edges and the int16 bin table DeviceCollator(bin_table=) reads from the unit vectors on the device (csrc_bins/bins.hip through
_lib_bins): order statistics of the squared chord by a radix select that stores nothing of size P^2, then a search of every
pair's squared chord among the edges mapped to squared chords.  `distance_bins_host` is the same rule in numpy.

Where no table of all pairs can exist (P = 100 000), `pair_bins` keeps the unit vectors and the thresholds on the device and
`batch_bins` runs the same search for the pairs of one batch only (csrc_pairbins/batch.hip through _pairbins): what
DeviceCollator(pair_bins=) launches.
`batch_bins_host` is that rule in numpy."""
import dataclasses
import math

import numpy as np
import torch

EARTH_RADIUS_KM = 6371.0                           # foursquare_process.py:16
FORMS = ("mask", "csr")


def chord2_max(radius_km):
    """4 sin^2(r / 2R): the squared chord between unit vectors at great-circle distance r."""
    return 4.0 * math.sin(float(radius_km) / (2.0 * EARTH_RADIUS_KM)) ** 2


def mask_pitch(P):
    """Words per row of MaskAdj.mask: whole groups of four 32-bit words."""
    return (int(P) + 127) // 128 * 4


def _coords(coords_deg, pad_row):
    c = coords_deg.detach().cpu().numpy() if isinstance(coords_deg, torch.Tensor) else np.asarray(coords_deg)
    c = np.ascontiguousarray(c, dtype=np.float64)
    if c.ndim != 2 or c.shape[1] != 2:
        raise ValueError(f"coords: expected [P, 2] latitude / longitude in degrees, got shape {c.shape}")
    if pad_row:
        c = np.ascontiguousarray(c[1:])                                # row 0 = the pad POI (DeviceCollator(coords=), recommend(coords=))
    if c.shape[0] < 1:
        raise ValueError("coords: no POI")
    if not np.all(np.isfinite(c)):
        raise ValueError("coords: latitude / longitude must be finite")
    return c


def _forms(forms):
    forms = (forms,) if isinstance(forms, str) else tuple(forms)
    if not forms or any(f not in FORMS for f in forms):
        raise ValueError(f"forms: a non-empty subset of {FORMS}, got {forms!r}")
    return forms


def unit_vectors_host(coords_deg):
    """[P, 2] degrees -> [P, 3] f64 (cos lat cos lon, cos lat sin lon, sin lat), radians = deg * pi / 180 (:17-20)."""
    lat, lon = coords_deg[:, 0] * math.pi / 180.0, coords_deg[:, 1] * math.pi / 180.0
    return np.stack([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)], 1)


class RadiusGraph:
    """A within-radius graph of P POIs (POI 1..P in row order) as tensors on one device.

    deg     int32 [P]           neighbours of each POI
    words   int32 [P, W] | None bits of A + I, MaskAdj's layout (form "mask")
    rowptr, col, val     | None CSR of (D+I)^-1 (A+I), columns ascending (form "csr")"""

    def __init__(self, P, radius_km, deg, words=None, rowptr=None, col=None, val=None):
        self.P, self.radius_km, self.deg = int(P), float(radius_km), deg
        self.words, self.rowptr, self.col, self.val = words, rowptr, col, val
        self.shape = (self.P, self.P)

    @property
    def forms(self):
        return tuple(f for f, t in zip(FORMS, (self.words, self.col)) if t is not None)

    @property
    def device(self):
        return self.deg.device

    def require(self, form):
        if form not in self.forms:
            raise ValueError(f"this RadiusGraph was built with forms={self.forms}: build it with {form!r} in `forms`")

    def scale(self):
        """f32 [P]: (float)(1.0 / (deg + 1.0)), the row scale of (D+I)^-1 (A+I)."""
        return (1.0 / (self.deg.to(torch.float64) + 1.0)).to(torch.float32)

    def mask_adj(self):
        """(mask, mask_t, scale), the tensors MaskAdj.from_dense01(A) returns; mask_t IS mask: the graph is symmetric."""
        self.require("mask")
        return self.words, self.words, self.scale()

    def csr_adj(self):
        """The six tensors CsrAdj.from_scipy(a_hat) returns for model_fqandtoyo.py:211-214's a_hat.  The transpose has the
        same structure (a symmetric graph); its values are the scale of each entry's COLUMN (the normalisation is per row)."""
        self.require("csr")
        return self.rowptr, self.col, self.val, self.rowptr, self.col, self.scale().index_select(0, self.col.long())

    def _host_structure(self):
        """(rowptr int64 [P + 1], col int32) of A + I on the host, columns ascending."""
        if self.col is not None:
            return self.rowptr.cpu().numpy(), self.col.cpu().numpy()
        P, cols, counts = self.P, [], []
        step = max(1, 4_000_000 // P)
        for r0 in range(0, P, step):
            by = np.ascontiguousarray(self.words[r0:r0 + step].cpu().numpy()).view(np.uint8)
            r, c = np.nonzero(np.unpackbits(by, axis=1, bitorder="little")[:, :P])
            cols.append(c.astype(np.int32))
            counts.append(np.bincount(r, minlength=by.shape[0]))
        rowptr = np.zeros(P + 1, dtype=np.int64)
        np.cumsum(np.concatenate(counts), out=rowptr[1:])
        return rowptr, np.concatenate(cols)

    def to_scipy(self):
        """The 0/1 graph_dist itself (no diagonal) as scipy CSR float32: what SparseUniverse.graph_dist holds."""
        from scipy import sparse
        rowptr, col = self._host_structure()
        P = self.P
        keep = col != np.repeat(np.arange(P, dtype=np.int32), np.diff(rowptr))
        return sparse.csr_matrix((np.ones(int(keep.sum()), dtype=np.float32), col[keep], rowptr - np.arange(P + 1)), shape=(P, P))

    def to_dense01(self):
        """The 0/1 graph_dist as a dense float32 [P, P] array: what Universe.graph_dist holds (small P only)."""
        return np.asarray(self.to_scipy().todense(), dtype=np.float32)


# ---- the device path ----------------------------------------------------------------------------------------------------------
def _launch(name, *args):
    from . import _lib_geo
    _lib_geo.launch(name, *args)


def _check(t, dtype, shape, what):
    if not (t.is_cuda and t.dtype == dtype and tuple(t.shape) == tuple(shape) and t.is_contiguous()):
        raise ValueError(f"{what}: expected a contiguous {dtype} tensor of shape {tuple(shape)} on the GPU, got {t.dtype} "
                         f"{tuple(t.shape)} on {t.device}")
    return t


def unit_vectors(coords_deg):
    """f64 [P, 2] on the device -> f64 [P, 3] (mobgt_geo_unit_vectors)."""
    from .ops import _p, _stream
    P = coords_deg.shape[0]
    _check(coords_deg, torch.float64, (P, 2), "coords_deg")
    out = torch.empty(P, 3, dtype=torch.float64, device=coords_deg.device)
    _launch("mobgt_geo_unit_vectors", _p(coords_deg), _p(out), P, _stream())
    return out


def radius_words(unit, c2max, words=None, deg=None):
    """-> (words int32 [P, W], deg int32 [P]) (mobgt_geo_radius_words); `words` / `deg`: buffers to write into."""
    from .ops import _p, _stream
    P = unit.shape[0]
    _check(unit, torch.float64, (P, 3), "unit")
    words = torch.empty(P, mask_pitch(P), dtype=torch.int32, device=unit.device) if words is None else words
    deg = torch.empty(P, dtype=torch.int32, device=unit.device) if deg is None else deg
    _check(words, torch.int32, (P, mask_pitch(P)), "words")
    _check(deg, torch.int32, (P,), "deg")
    _launch("mobgt_geo_radius_words", _p(unit), P, float(c2max), _p(words), _p(deg), _stream())
    return words, deg


def radius_count(unit, c2max, deg=None):
    """-> deg int32 [P] (mobgt_geo_radius_count)."""
    from .ops import _p, _stream
    P = unit.shape[0]
    _check(unit, torch.float64, (P, 3), "unit")
    deg = torch.empty(P, dtype=torch.int32, device=unit.device) if deg is None else deg
    _check(deg, torch.int32, (P,), "deg")
    _launch("mobgt_geo_radius_count", _p(unit), P, float(c2max), _p(deg), _stream())
    return deg


def row_offsets(deg):
    """rowptr int64 [P + 1] of A + I: the exclusive prefix sum of deg + 1."""
    rowptr = torch.zeros(deg.numel() + 1, dtype=torch.int64, device=deg.device)
    torch.cumsum(deg.to(torch.int64) + 1, 0, out=rowptr[1:])
    return rowptr


def radius_fill(unit, c2max, rowptr, col=None, val=None):
    """-> (col int32 [nnz], val f32 [nnz]) (mobgt_geo_radius_fill).  The kernel stores row i inside rowptr[i] .. rowptr[i + 1];
    that this stays inside `col` / `val` is checked here, on the host (one read-back of rowptr): rowptr starts at 0, never
    decreases and ends at the buffers' size."""
    from .ops import _p, _stream
    P = unit.shape[0]
    _check(unit, torch.float64, (P, 3), "unit")
    _check(rowptr, torch.int64, (P + 1,), "rowptr")
    first, last, sorted_ = int(rowptr[0]), int(rowptr[-1]), bool((rowptr[1:] >= rowptr[:-1]).all())
    if first != 0 or not sorted_ or last < P:
        raise ValueError(f"rowptr: not the prefix sum of deg + 1 (starts at {first}, ends at {last}, non-decreasing: {sorted_})")
    col = torch.empty(last, dtype=torch.int32, device=unit.device) if col is None else col
    val = torch.empty(last, dtype=torch.float32, device=unit.device) if val is None else val
    for name, t, dt in (("col", col, torch.int32), ("val", val, torch.float32)):
        if t.numel() != last:
            raise ValueError(f"{name}: {t.numel()} elements, rowptr ends at {last}")
        _check(t, dt, (last,), name)
    _launch("mobgt_geo_radius_fill", _p(unit), P, float(c2max), _p(rowptr), _p(col), _p(val), _stream())
    return col, val


def radius_graph(coords_deg, radius_km=3.0, device="cuda", forms=FORMS, pad_row=False):
    """coords [P, 2] latitude / longitude in degrees, POI 1..P in row order (or [P + 1, 2] with `pad_row`: row 0 is the pad
    POI, the table DeviceCollator(coords=) and recommend(coords=) take) -> RadiusGraph on `device`.
    forms=("csr",) never allocates the P x W words (1.25 GB at P = 100 000): a count launch, a prefix sum, a fill launch."""
    forms = _forms(forms)
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError("radius_graph runs on the GPU; the host form is radius_graph_host")
    c = _coords(coords_deg, pad_row)
    P, c2 = c.shape[0], chord2_max(radius_km)
    with torch.cuda.device(device):
        unit = unit_vectors(torch.tensor(c, device=device))
        words = rowptr = col = val = None
        if "mask" in forms:
            words, deg = radius_words(unit, c2)
        else:
            deg = radius_count(unit, c2)
        if "csr" in forms:
            rowptr = row_offsets(deg)
            col, val = radius_fill(unit, c2, rowptr)
    return RadiusGraph(P, radius_km, deg, words, rowptr, col, val)


# ---- the host form --------------------------------------------------------------------------------------------------------------
def radius_graph_host(coords_deg, radius_km=3.0, forms=FORMS, pad_row=False):
    """The same rule in numpy f64 -> RadiusGraph of CPU tensors.  Blocked over rows: never P x P at once."""
    forms = _forms(forms)
    c = _coords(coords_deg, pad_row)
    P, c2 = c.shape[0], chord2_max(radius_km)
    u = unit_vectors_host(c)
    W = mask_pitch(P)
    words = np.zeros((P, W), dtype=np.int32) if "mask" in forms else None
    deg = np.zeros(P, dtype=np.int32)
    cols = []
    step = max(1, 4_000_000 // P)
    for r0 in range(0, P, step):
        ur = u[r0:r0 + step]
        d2 = (ur[:, None, 0] - u[None, :, 0]) ** 2
        d2 += (ur[:, None, 1] - u[None, :, 1]) ** 2
        d2 += (ur[:, None, 2] - u[None, :, 2]) ** 2
        m = (d2 > 0.0) & (d2 <= c2)
        deg[r0:r0 + step] = m.sum(axis=1)
        m[np.arange(ur.shape[0]), np.arange(r0, r0 + ur.shape[0])] = True       # A + I
        if words is not None:
            by = np.packbits(m, axis=1, bitorder="little")
            words[r0:r0 + step].view(np.uint8)[:, :by.shape[1]] = by
        if "csr" in forms:
            cols.append(np.nonzero(m)[1].astype(np.int32))
    t = torch.from_numpy
    g = RadiusGraph(P, radius_km, t(deg), t(words) if words is not None else None)
    if "csr" in forms:
        g.rowptr, g.col = row_offsets(g.deg), t(np.concatenate(cols))
        g.val = torch.repeat_interleave(g.scale(), g.deg.long() + 1)
    return g


# ---- the distance bins ----------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class DistanceBins:
    """The distance bins of P POIs (POI 1..P in row order): what collator.py:301-308 and :429-437 compute from the distance matrix.

    num_bins    the Freedman-Diaconis bin count
    edges       f64 [num_bins + 1] km: np.histogram's edges, poi_pos = np.digitize(distance, edges)
    thresholds  f64 [num_bins + 1]: the edges as squared chords of unit vectors (the first 0, the last the farthest pair's own)
    table       int16 [(P+1), (P+1)] | None: poi_pos of every pair, row / column 0 = the pad POI (DeviceCollator(bin_table=))"""
    P: int
    num_bins: int
    edges: np.ndarray
    thresholds: np.ndarray
    table: object = None


def chord2_to_km(c2):
    """Squared chord of two unit vectors -> great-circle distance: 2 R arcsin(sqrt(c2) / 2)."""
    return 2.0 * EARTH_RADIUS_KM * np.arcsin(np.minimum(np.sqrt(np.asarray(c2, dtype=np.float64)) / 2.0, 1.0))


def _select(digit_counts, digit_bits, n, ranks, info=None):
    """The host loop of the radix select: the order statistics at 0-based `ranks` of a multiset of n non-negative f64, which
    order as their 64-bit patterns.  digit_counts(prefix, prefix_bits) -> int64 [2^digit_bits]: how many elements whose pattern
    starts with `prefix` have each next digit.  64 / digit_bits calls per rank; ranks that share a prefix share the call."""
    seen = {}
    out = np.empty(len(ranks), dtype=np.uint64)
    for q, rank in enumerate(ranks):
        rank = int(rank)
        if not 0 <= rank < n:
            raise ValueError(f"ranks: {rank} is not in 0 .. {n - 1}")
        prefix = below = 0
        for bits in range(0, 64, digit_bits):
            if (prefix, bits) not in seen:
                seen[prefix, bits] = np.cumsum(digit_counts(prefix, bits))
            cum = seen[prefix, bits]
            digit = int(np.searchsorted(cum, rank - below, side="right"))            # the first digit with cum > rank - below
            if digit >= cum.size or (bits == 0 and int(cum[-1]) != n):
                raise RuntimeError(f"radix select: the histogram below prefix {prefix:#x} ({bits} bits) holds {int(cum[-1])} "
                                   f"elements, rank {rank} of {n} is not among them")
            below += int(cum[digit - 1]) if digit else 0
            prefix = (prefix << digit_bits) | digit
        out[q] = prefix
    if info is not None:
        info["launches"] = info.get("launches", 0) + len(seen)
    return out.view(np.float64)


def _bins_from(P, order_stats, table):
    """The host side of collator.py:301-308: (num_bins, edges km, thresholds) from five order statistics of the squared chord.
    order_stats(ranks) -> f64 [len(ranks)]."""
    from ._lib_bins import MAX_THRESHOLDS
    n = P * P
    ranks, frac = [], []
    for q in (0.75, 0.25):                                             # np.percentile(x, [75, 25]), method "linear"
        v = q * (n - 1)
        k = math.floor(v)
        ranks += [k, min(k + 1, n - 1)]
        frac.append(v - k)
    ranks.append(n - 1)                                                # np.max(x); np.min(x) is the diagonal's 0
    c2 = np.asarray(order_stats(ranks), dtype=np.float64)
    km = chord2_to_km(c2)
    lerp = lambda a, b, t: a + (b - a) * t if t < 0.5 else b - (b - a) * (1.0 - t)
    iqr = lerp(km[0], km[1], frac[0]) - lerp(km[2], km[3], frac[1])
    if not (np.isfinite(iqr) and iqr > 0.0):
        raise ValueError(f"distance bins: the interquartile range of the pair distances is {iqr} km, the Freedman-Diaconis bin "
                         "width needs a positive one")
    binsize = 2.0 * iqr * np.power(float(P), -1 / 3)                   # len(x) = the rows of the matrix
    num_bins = int(np.ceil(km[4] / binsize))
    if table and num_bins + 1 > MAX_THRESHOLDS:
        raise ValueError(f"distance bins: {num_bins} bins do not fit the int16 table ({MAX_THRESHOLDS} thresholds at most); "
                         "table=False gives the edges")
    edges = np.linspace(0.0, km[4], num_bins + 1)                      # np.histogram(x, num_bins)[1]
    thresholds = 4.0 * np.sin(edges / (2.0 * EARTH_RADIUS_KM)) ** 2
    thresholds[0] = 0.0                                                # zero-distance pairs: bin 1
    thresholds[-1] = c2[4]                                             # the farthest pair: bin num_bins + 1, as np.digitize has it
    if np.any(np.diff(thresholds) < 0.0):
        raise ValueError("distance bins: the thresholds are not non-decreasing")
    return num_bins, edges, thresholds


def _launch_bins(name, *args):
    from . import _lib_bins
    _lib_bins.launch(name, *args)


def chord2_digit_counts(unit, prefix, prefix_bits, counts=None):
    """-> counts int64 [RADIX] on the device (mobgt_bins_chord2_digits): one level of the radix select."""
    from ._lib_bins import RADIX
    from .ops import _p, _stream
    P = unit.shape[0]
    _check(unit, torch.float64, (P, 3), "unit")
    counts = torch.empty(RADIX, dtype=torch.int64, device=unit.device) if counts is None else counts
    _check(counts, torch.int64, (RADIX,), "counts")
    _launch_bins("mobgt_bins_chord2_digits", _p(unit), P, int(prefix), int(prefix_bits), _p(counts), _stream())
    return counts


def chord2_order_stats(unit, ranks, info=None):
    """unit f64 [P, 3] on the device -> np f64 [len(ranks)]: the order statistics at the 0-based `ranks` of the multiset of the
    squared chords of all P^2 ordered pairs (the diagonal and both orders included), bit-exact.  At most 64 / DIGIT_BITS
    launches and 2 KB read-backs per rank; `info["launches"]` counts them."""
    from ._lib_bins import DIGIT_BITS, RADIX
    P = unit.shape[0]
    counts = torch.empty(RADIX, dtype=torch.int64, device=unit.device)
    with torch.cuda.device(unit.device):
        return _select(lambda prefix, bits: chord2_digit_counts(unit, prefix, bits, counts).cpu().numpy(), DIGIT_BITS, P * P, ranks,
                       info)


def bin_table(unit, thresholds, table=None):
    """-> table int16 [(P+1), (P+1)] on the device (mobgt_bins_table): np.searchsorted(thresholds, c2, side="right") of every
    pair, row / column 0 = the pad POI.  `thresholds`: f64 on the host; that they never decrease is checked here (the kernel
    cannot).  `table`: a buffer to write into."""
    from .ops import _p, _stream
    P = unit.shape[0]
    _check(unit, torch.float64, (P, 3), "unit")
    thr = _checked_thresholds(thresholds)
    table = torch.empty(P + 1, P + 1, dtype=torch.int16, device=unit.device) if table is None else table
    _check(table, torch.int16, (P + 1, P + 1), "table")
    with torch.cuda.device(unit.device):
        _launch_bins("mobgt_bins_table", _p(unit), P, _p(torch.tensor(thr, device=unit.device)), thr.size, _p(table), _stream())
    return table


def _bin_coords(coords_deg, pad_row):
    c = _coords(coords_deg, pad_row)
    if c.shape[0] < 2:
        raise ValueError(f"distance bins: {c.shape[0]} POI, the percentiles of the pair distances need at least 2")
    return c


def distance_bins(coords_deg, device="cuda", pad_row=False, table=True):
    """coords [P, 2] latitude / longitude in degrees, POI 1..P in row order (or [P + 1, 2] with `pad_row`: row 0 is the pad
    POI) -> DistanceBins: the reference's num_bins and edges (collator.py:301-308) and, with `table`, the int16 bin table
    (collator.py:429-437) on `device`.  Nothing of size P^2 exists on the host; table=False allocates nothing of size P^2 at
    all and has no limit on the bin count (P = 100 000: the edges for DeviceCollator(coords=, bin_edges=))."""
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError("distance_bins runs on the GPU; the host form is distance_bins_host")
    c = _bin_coords(coords_deg, pad_row)
    P = c.shape[0]
    with torch.cuda.device(device):
        unit = unit_vectors(torch.tensor(c, device=device))
        num_bins, edges, thr = _bins_from(P, lambda ranks: chord2_order_stats(unit, ranks), table)
        return DistanceBins(P, num_bins, edges, thr, bin_table(unit, thr) if table else None)


# ---- the distance bins of one batch's pairs ---------------------------------------------------------------------------------------
@dataclasses.dataclass
class PairBins:
    """What the search of one batch's pairs reads (DeviceCollator(pair_bins=)): the POIs' unit vectors and the bin edges as
    squared chords, on one device.

    unit        f64 [P, 3] tensor: row i is POI i + 1
    thresholds  f64 [num_bins + 1] tensor, non-decreasing: poi_pos = #{k : thresholds[k] <= c2}
    num_bins    the bin count: poi_pos of a real pair lies in 0 .. num_bins + 1"""
    P: int
    unit: torch.Tensor
    thresholds: torch.Tensor
    num_bins: int

    @property
    def device(self):
        return self.unit.device

    def to(self, device):
        return PairBins(self.P, self.unit.to(device), self.thresholds.to(device), self.num_bins)


def _checked_thresholds(thresholds):
    """-> contiguous f64 array; the count and that they never decrease are checked here, on the host (the kernels cannot)."""
    from ._lib_bins import MAX_THRESHOLDS, MIN_THRESHOLDS
    thr = np.ascontiguousarray(thresholds, dtype=np.float64)
    if thr.ndim != 1 or not MIN_THRESHOLDS <= thr.size <= MAX_THRESHOLDS:
        raise ValueError(f"thresholds: expected {MIN_THRESHOLDS} .. {MAX_THRESHOLDS} f64, got shape {thr.shape}")
    if np.isnan(thr).any() or np.any(np.diff(thr) < 0.0):
        raise ValueError("thresholds: not non-decreasing")
    return thr


def pair_bins(coords_deg, bins=None, edges=None, device="cuda", pad_row=False):
    """coords [P, 2] latitude / longitude in degrees, POI 1..P in row order (or [P + 1, 2] with `pad_row`) -> PairBins on `device`.
    Exactly one of: `bins`, a DistanceBins of the same POIs, whose thresholds are taken as they are (the last is the farthest
    pair's own squared chord); `edges`, plain bin edges in km (SparseUniverse.bin_edges), mapped through 4 sin^2(e / 2R) with the
    first forced to 0.  On a GPU the unit vectors are mobgt_geo_unit_vectors' (the ones distance_bins took its thresholds from);
    on the CPU unit_vectors_host's, for batch_bins_host."""
    if (bins is None) == (edges is None):
        raise ValueError("pair_bins: give exactly one of bins= (a DistanceBins) and edges= (bin edges in km)")
    c = _coords(coords_deg, pad_row)
    P = c.shape[0]
    if bins is not None:
        if bins.P != P:
            raise ValueError(f"pair_bins: bins were built for {bins.P} POIs, coords hold {P}")
        thr = np.asarray(bins.thresholds, dtype=np.float64)
    else:
        e = np.asarray(edges, dtype=np.float64)
        thr = 4.0 * np.sin(e / (2.0 * EARTH_RADIUS_KM)) ** 2
        if thr.ndim == 1 and thr.size:
            thr[0] = 0.0                                               # zero-distance pairs: bin 1
    thr = _checked_thresholds(thr)
    device = torch.device(device)
    if device.type == "cuda":
        with torch.cuda.device(device):
            unit = unit_vectors(torch.tensor(c, device=device))
    else:
        unit = torch.from_numpy(unit_vectors_host(c))
    return PairBins(P, unit, torch.tensor(thr, device=device), thr.size - 1)


def batch_bins(pair_bins, x, out=None):
    """-> poi_pos int16 [G, N, N] on the device (mobgt_bins_batch): #{k : thresholds[k] <= c2} for every pair of POIs of each row
    of `x` (int32 [G, N] or [G, N, 1] POI ids, 0 = pad), 0 for a pair with a pad or an id outside 1 .. P.  One launch on the
    current stream, no allocation when `out` is given (any int16-aligned view, such as BatchLayout's)."""
    from .ops import _p, _stream
    if x.dim() == 3 and x.shape[2] == 1:
        x = x[:, :, 0]
    if x.dim() != 2:
        raise ValueError(f"x: expected POI ids of shape [G, N] or [G, N, 1], got {tuple(x.shape)}")
    G, N = x.shape
    if pair_bins.unit.device.type != "cuda":
        raise ValueError("batch_bins runs on the GPU; the host form is batch_bins_host")
    _check(x, torch.int32, (G, N), "x")
    out = torch.empty(G, N, N, dtype=torch.int16, device=x.device) if out is None else out
    _check(out, torch.int16, (G, N, N), "out")
    from . import _pairbins
    _pairbins.launch("mobgt_bins_batch", _p(pair_bins.unit), pair_bins.P, _p(pair_bins.thresholds), pair_bins.thresholds.numel(), _p(x), G, N,
                 _p(out), _stream())
    return out


def batch_bins_host(unit, thresholds, x):
    """batch_bins in numpy -> int16 [G, N, N]: np.searchsorted(thresholds, c2, side="right") on _chord2_rows_host's expression
    for the pairs whose ids both lie in 1 .. P, 0 elsewhere.  The kernel's reference and the CPU form."""
    u = np.ascontiguousarray(unit, dtype=np.float64)
    thr = _checked_thresholds(thresholds)
    ids = np.asarray(x)
    ids = ids[:, :, 0] if ids.ndim == 3 else ids
    G, N = ids.shape
    ok = (ids >= 1) & (ids <= u.shape[0])
    out = np.zeros((G, N, N), dtype=np.int16)
    for g in range(G):
        ug = u[np.where(ok[g], ids[g].astype(np.int64) - 1, 0)]
        pos = np.searchsorted(thr, _chord2_rows_host(ug, 0, N), side="right")
        out[g] = np.where(ok[g][:, None] & ok[g][None, :], pos, 0)
    return out


# ---- the distance bins: the host form ---------------------------------------------------------------------------------------------
_HOST_DIGIT_BITS = 16


def _chord2_rows_host(u, r0, r1):
    """c2 of rows r0 .. r1 - 1 against every column: include/mobgt_bins.h's expression, every operation rounded once."""
    dx, dy, dz = (u[r0:r1, None, k] - u[None, :, k] for k in range(3))
    return ((dx * dx) + (dy * dy)) + (dz * dz)


def chord2_order_stats_host(unit, ranks):
    """chord2_order_stats in numpy: the same select with 16-bit digits, blocked over rows."""
    u = np.ascontiguousarray(unit, dtype=np.float64)
    P = u.shape[0]
    step = max(1, 4_000_000 // P)

    def digit_counts(prefix, bits):
        counts = np.zeros(1 << _HOST_DIGIT_BITS, dtype=np.int64)
        for r0 in range(0, P, step):
            key = _chord2_rows_host(u, r0, r0 + step).reshape(-1).view(np.uint64)
            if bits:
                key = key[(key >> np.uint64(64 - bits)) == np.uint64(prefix)]
            digit = (key >> np.uint64(64 - bits - _HOST_DIGIT_BITS)) & np.uint64((1 << _HOST_DIGIT_BITS) - 1)
            counts += np.bincount(digit.astype(np.int64), minlength=counts.size)
        return counts

    return _select(digit_counts, _HOST_DIGIT_BITS, P * P, ranks)


def distance_bins_host(coords_deg, pad_row=False, table=True, unit=None):
    """The same rule in numpy f64 -> DistanceBins with a CPU tensor as its table.  Blocked over rows: never P x P in f64 at once.
    `unit`: run on these [P, 3] unit vectors instead of unit_vectors_host(coords)."""
    c = _bin_coords(coords_deg, pad_row)
    P = c.shape[0]
    u = unit_vectors_host(c) if unit is None else np.ascontiguousarray(unit, dtype=np.float64)
    if u.shape != (P, 3):
        raise ValueError(f"unit: expected shape {(P, 3)}, got {u.shape}")
    num_bins, edges, thr = _bins_from(P, lambda ranks: chord2_order_stats_host(u, ranks), table)
    out = None
    if table:
        out = np.empty((P + 1, P + 1), dtype=np.int16)
        out[0, :] = out[:, 0] = np.searchsorted(thr, 0.0, side="right")
        step = max(1, 4_000_000 // P)
        for r0 in range(0, P, step):
            out[1 + r0:1 + r0 + step, 1:] = np.searchsorted(thr, _chord2_rows_host(u, r0, r0 + step), side="right")
        out = torch.from_numpy(out)
    return DistanceBins(P, num_bins, edges, thr, out)
