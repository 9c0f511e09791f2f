"""The within-radius POI graph from coordinates: `graph_dist`, the 0/1 "within 3 km" matrix the distance GCN runs on.

The reference builds it with a Python double loop over all P^2 pairs (graphormer/foursquare_process.py:689-702, one LLs2Dist
call :15-23 per pair).  `radius_graph` decides the same pairs on the device (csrc_geo/radius.hip through _lib_geo) and leaves
the result there in the forms the GCN kernels read: the bit words of modelGNN.MaskAdj and the CSR of modelGNN.CsrAdj.
`radius_graph_host` is the same rule in numpy f64, blocked over rows: the CPU form and the tests' reference.

The rule (include/mobgt_geo.h): pair (i, j), i != j, is an edge iff 0 < |u_i - u_j|^2 <= 4 sin^2(r / 2R) in f64, u the unit
vectors of the two POIs, R = 6371 km.  It agrees with `0 < haversine <= r` except for pairs within rounding (~1e-9 km) of
the radius or of distance zero; POIs with identical coordinates are not neighbours, as in the reference."""
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
