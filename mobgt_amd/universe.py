"""The POI table and the transition graphs from check-in sessions: the last inputs of `Graphormer.__init__` that came from the
reference's offline pandas run (graphormer/foursquare_process.py).

* the Graph_poi.csv columns `checkin_cnt`, `cat` and `check_freq` (build_users_locations_dict, :262-294);
* Graph_cat.csv, the adjacency of the category GCN (prepare_global_data, :654-668);
* Graph_adj.csv, the POI transition counts (:678-687).

All are counts over sessions -- (user, [L + 1, 3] rows of (poi, time slot, category)), what data.SessionDataset stores -- with
dense ids: POIs 1 .. P and categories 1 .. n_cat, numbered by first appearance (`first_seen_ids`, the reference's vid_list /
catid_list).  The rules (golden G13 pins them to the reference's own files):

    checkin_cnt[p - 1]       check-ins at POI p over ALL sessions, train and test
    poi_cat[p - 1]           the POI's category (0: no check-in); a POI seen with two categories is refused
    check_freq[p - 1]        check-ins, over all sessions, whose category is the POI's: cat_cnt[poi_cat] -- check-ins, not POIs
    graph_cat[a - 1, b - 1]  consecutive check-in pairs (k - 1, k) inside one TRAIN session with categories a -> b
    graph_adj[p - 1, q - 1]  the same for POIs p -> q: self transitions on the diagonal, nothing clipped, no pair spans two
                             sessions; all L transitions of a session count, the one into its target row included

`universe_counts` counts on the device (csrc_universe/counts.hip through _universe): one launch over the packed check-ins for the
small spaces, and for the P^2 space of POI pairs one 64-bit key per transition, torch.sort, and two launches that read the runs
of equal keys off as a CSR -- no P x P array exists.  `universe_counts_host` is the same rule in numpy: the CPU form and the
kernel's reference.  `build_universe` adds what geo builds from coordinates: check-ins and coordinates in, a synth.Universe for
Graphormer and the distance bins for its collator out."""
import dataclasses
import os

import numpy as np
import torch

POI_COLUMNS = ("POI ID", "checkin_cnt", "lat", "lon", "cat", "check_freq")
MAX_DENSE_P = 16384                                # TransitionGraph.to_dense: a dense [P, P] f32 array of 1 GiB at this P
MAX_CSV_P = MAX_DENSE_P                            # write_csvs: two dense [P, P] f64 frames of 2 GiB each at this P


def first_seen_ids(values):
    """Arbitrary hashable or integer ids -> (dense ids int64 in 1 .. K, numbered by first appearance; lookup: the K raw ids in
    that order, lookup[k - 1] is the raw id of k).  The reference's vid_list / catid_list numbering (:277-289).  Host numpy."""
    if isinstance(values, np.ndarray):
        if values.ndim != 1:
            raise ValueError(f"first_seen_ids: expected a flat sequence of ids, got shape {values.shape}")
        arr = values
    else:
        values = list(values)
        arr = np.asarray(values) if all(isinstance(v, (int, np.integer, str)) for v in values) else None
    if arr is not None and arr.size and (np.issubdtype(arr.dtype, np.integer) or arr.dtype.kind in "US"):
        uniq, first, inv = np.unique(arr, return_index=True, return_inverse=True)
        order = np.argsort(first, kind="stable")                       # the distinct ids by first appearance
        rank = np.empty(len(uniq), dtype=np.int64)
        rank[order] = np.arange(1, len(uniq) + 1)
        return rank[inv.reshape(-1)], uniq[order]
    seen, dense = {}, np.empty(len(values), dtype=np.int64)
    for i, v in enumerate(values):
        dense[i] = seen.setdefault(v, len(seen) + 1)
    lookup = np.empty(len(seen), dtype=object)
    lookup[:] = list(seen)
    return dense, lookup


class TransitionGraph:
    """Transition counts between P POIs (POI 1 .. P in row order) as a CSR on one device: Graph_adj without its P^2 zeros.

    rowptr  int64 [P + 1]
    col     int32 [nnz]   ascending inside a row
    val     int32 [nnz]   val[k] = the number of train transitions row -> col[k]"""

    def __init__(self, P, rowptr, col, val):
        self.P, self.rowptr, self.col, self.val = int(P), rowptr, col, val
        self.shape = (self.P, self.P)

    @property
    def nnz(self):
        return int(self.col.numel())

    @property
    def device(self):
        return self.rowptr.device

    def to_scipy(self):
        """scipy CSR float32 [P, P]."""
        from scipy import sparse
        return sparse.csr_matrix((self.val.cpu().numpy().astype(np.float32), self.col.cpu().numpy(), self.rowptr.cpu().numpy()),
                                 shape=self.shape)

    def to_dense(self):
        """Dense float32 [P, P]: what synth.Universe.graph_adj and Graph_adj.csv hold.  Refused above MAX_DENSE_P POIs."""
        if self.P > MAX_DENSE_P:
            raise ValueError(f"to_dense: {self.P} POIs, a dense [P, P] array is made up to {MAX_DENSE_P} POIs only; to_scipy() "
                             "gives the same counts as a CSR")
        return np.asarray(self.to_scipy().todense(), dtype=np.float32)


@dataclasses.dataclass
class UniverseCounts:
    """What `universe_counts` / `universe_counts_host` return: int32 tensors on one device.  T = the train transitions."""
    P: int
    n_cat: int
    T: int
    checkin_cnt: torch.Tensor      # [P]
    cat_cnt: torch.Tensor          # [n_cat]
    poi_cat: torch.Tensor          # [P], 0 = a POI without a check-in
    check_freq: torch.Tensor       # [P] = cat_cnt[poi_cat], 0 where poi_cat is 0
    graph_cat: torch.Tensor        # [n_cat, n_cat]
    graph_adj: TransitionGraph

    def poi_table(self, coords_deg):
        """coords [P, 2] latitude / longitude in degrees -> float64 [P, 6] in synth.Universe.poi_columns order (Graph_poi.csv)."""
        c = coords_deg.detach().cpu().numpy() if isinstance(coords_deg, torch.Tensor) else np.asarray(coords_deg)
        c = np.asarray(c, dtype=np.float64)
        if c.shape != (self.P, 2):
            raise ValueError(f"coords: expected [{self.P}, 2] latitude / longitude in degrees, got shape {c.shape}")
        col = lambda t: t.cpu().numpy().astype(np.float64)
        return np.stack([np.arange(1, self.P + 1, dtype=np.float64), col(self.checkin_cnt), c[:, 0], c[:, 1], col(self.poi_cat),
                         col(self.check_freq)], 1)


# ---- what both forms check on the host, before anything is launched ---------------------------------------------------------------
def _dataset(ds):
    from .prefixes import PrefixDataset
    if isinstance(ds, PrefixDataset):
        raise TypeError("the universe is counted over sessions, and a PrefixDataset holds every transition of a session once per "
                        "prefix that contains it: give its base, pds.base")
    if all(hasattr(ds, a) for a in ("seq", "offsets", "users")):
        return ds
    from .data import SessionDataset
    return SessionDataset(ds)


def _first_session(offsets, bad):
    """The session of the first check-in at which `bad` holds."""
    i = int(np.argmax(bad))
    return int(np.searchsorted(offsets, i, side="right")) - 1, i


def _prepare(ds, train, P, n_cat):
    """-> (seq int32 [M, 3], offsets int64 [S + 1], train mask bool [S], P, n_cat), every ValueError raised."""
    ds = _dataset(ds)
    seq, offsets = ds.seq, np.asarray(ds.offsets, dtype=np.int64)
    M, S = int(seq.shape[0]), len(offsets) - 1
    if M >= 2 ** 31:
        s = int(np.searchsorted(offsets, 2 ** 31 - 1, side="right")) - 1
        raise ValueError(f"session {s}: check-in number 2**31 of {M} lies in it, the kernels index check-ins with 31 bits "
                         "(M < 2**31): count the sessions in parts")
    t = np.asarray(train)
    if t.dtype == np.bool_:
        if t.shape != (S,):
            raise ValueError(f"train: a mask of {t.shape[0] if t.ndim == 1 else t.shape} flags for {S} sessions")
        mask = t
    else:
        if t.size and not np.issubdtype(t.dtype, np.integer):
            raise ValueError(f"train: a boolean mask of length {S} or integer session indices, got {t.dtype}")
        t = t.reshape(-1).astype(np.int64)
        if t.size and (t.min() < 0 or t.max() >= S):
            raise ValueError(f"train: session index {int(t[(t < 0) | (t >= S)][0])} is not in 0 .. {S - 1}")
        mask = np.zeros(S, dtype=bool)
        mask[t] = True
    for what, colno, given in (("POI", 0, P), ("category", 2, n_cat)):                    # (on seq as given: before any cast to int32)
        v = seq[:, colno]
        top = int(v.max()) if M else 0
        limit = min(top if given is None else int(given), 2 ** 31 - 1)
        if given is not None and limit < 1:
            raise ValueError(f"universe_counts: {what} count {limit}, at least 1 is needed")
        bad = (v < 1) | (v > limit)
        if bad.any():
            s, i = _first_session(offsets, bad)
            raise ValueError(f"session {s}: {what} id {int(v[i])} at check-in {i - int(offsets[s])} is not in 1 .. {limit} "
                             f"(dense ids: data.first_seen_ids)")
        if colno == 0:
            P = max(limit, 1)
        else:
            n_cat = max(limit, 1)
    seq = np.ascontiguousarray(seq, dtype=np.int32)
    return seq, offsets, mask, int(P), int(n_cat)


def _one_category(poi_cat_min, poi_cat_max):
    """numpy [P] each -> poi_cat, or the ValueError that names the first POI seen with two categories."""
    two = (poi_cat_max != 0) & (poi_cat_min != poi_cat_max)
    if two.any():
        p = int(np.argmax(two))
        raise ValueError(f"POI {p + 1} was seen with more than one category ({int(poi_cat_min[p])} .. {int(poi_cat_max[p])}): the "
                         "reference silently keeps the first; give every POI one category")
    return poi_cat_max


def _check_freq(cat_cnt, poi_cat):
    return torch.cat([cat_cnt.new_zeros(1), cat_cnt]).index_select(0, poi_cat.long())


# ---- the host form ----------------------------------------------------------------------------------------------------------------
def universe_counts_host(ds, train, P=None, n_cat=None):
    """The rules of the module's docstring in numpy (np.add.at, a scipy CSR for the adjacency) -> UniverseCounts of CPU tensors.
    `ds`: a data.SessionDataset of EVERY session, train and test (or the sessions themselves); `train`: a boolean mask over the
    sessions or the indices of the train sessions.  `P` / `n_cat` default to the largest ids present."""
    from scipy import sparse
    seq, offsets, mask, P, n_cat = _prepare(ds, train, P, n_cat)
    M = seq.shape[0]
    poi, cat = seq[:, 0].astype(np.int64), seq[:, 2].astype(np.int64)
    checkin_cnt = np.bincount(poi - 1, minlength=P).astype(np.int32)
    cat_cnt = np.bincount(cat - 1, minlength=n_cat).astype(np.int32)
    lo, hi = np.full(P, np.iinfo(np.int32).max, dtype=np.int64), np.zeros(P, dtype=np.int64)
    np.minimum.at(lo, poi - 1, cat)
    np.maximum.at(hi, poi - 1, cat)
    poi_cat = _one_category(lo, hi).astype(np.int32)
    sid = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    inner = np.ones(M, dtype=bool)
    inner[offsets[:-1][offsets[:-1] < M]] = False                     # a session's first check-in follows nothing
    k = np.nonzero(inner & mask[sid])[0] if M else np.zeros(0, dtype=np.int64)
    graph_cat = np.zeros((n_cat, n_cat), dtype=np.int32)
    np.add.at(graph_cat, (cat[k - 1] - 1, cat[k] - 1), 1)
    adj = sparse.coo_matrix((np.ones(len(k), dtype=np.int32), (poi[k - 1] - 1, poi[k] - 1)), shape=(P, P)).tocsr()
    adj.sum_duplicates()
    adj.sort_indices()
    t = torch.from_numpy
    cat_cnt_t, poi_cat_t = t(cat_cnt), t(poi_cat)
    graph = TransitionGraph(P, t(adj.indptr.astype(np.int64)), t(adj.indices.astype(np.int32)), t(adj.data.astype(np.int32)))
    return UniverseCounts(P, n_cat, len(k), t(checkin_cnt), cat_cnt_t, poi_cat_t, _check_freq(cat_cnt_t, poi_cat_t), t(graph_cat), graph)


# ---- the device path --------------------------------------------------------------------------------------------------------------
def transition_csr(keys, P):
    """keys int64 [T] on the device, each (p - 1) * P + (q - 1) -> TransitionGraph: torch.sort, a launch that marks where the
    runs of equal keys begin (mobgt_universe_run_heads), torch.cumsum, a launch that writes rowptr / col / val
    (mobgt_universe_run_fill).  One read-back: nnz."""
    from . import _universe
    from .ops import _p, _stream
    T, dev = keys.numel(), keys.device
    rowptr = torch.empty(P + 1, dtype=torch.int64, device=dev)
    if T:
        keys = torch.sort(keys).values
        head = torch.empty(T, dtype=torch.int32, device=dev)
        _universe.launch("mobgt_universe_run_heads", _p(keys), T, _p(head), _stream())
        pos = torch.cumsum(head, 0, dtype=torch.int64)
        nnz = int(pos[-1])
    else:
        pos, nnz = keys, 0
    col = torch.empty(nnz, dtype=torch.int32, device=dev)
    val = torch.empty(nnz, dtype=torch.int32, device=dev)
    _universe.launch("mobgt_universe_run_fill", _p(keys), _p(pos), T, P, nnz, _p(rowptr), _p(col), _p(val), _stream())
    return TransitionGraph(P, rowptr, col, val)


def universe_counts(ds, train, P=None, n_cat=None, device="cuda"):
    """universe_counts_host on the device -> UniverseCounts of tensors on `device`, element for element the same integers.
    Everything is validated on the host before anything is launched; every failure is a ValueError naming the first offending
    session.  Host work: one np.repeat (the session of every check-in) and one cumsum over the sessions (where each train
    session's keys go); the check-ins travel as they are packed, 12 bytes each."""
    from . import _universe
    from .ops import _p, _stream
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError("universe_counts runs on the GPU; the host form is universe_counts_host")
    seq, offsets, mask, P, n_cat = _prepare(ds, train, P, n_cat)
    if P > _universe.MAX_P or n_cat > _universe.MAX_CAT:
        raise ValueError(f"universe_counts: P = {P} / n_cat = {n_cat} exceed the kernel's limits ({_universe.MAX_P}, {_universe.MAX_CAT})")
    M, S = seq.shape[0], len(offsets) - 1
    lengths = np.diff(offsets)
    trans = np.where(mask, np.maximum(lengths - 1, 0), 0)
    ends = np.cumsum(trans)
    T = int(ends[-1]) if S else 0
    slot0 = np.where(mask, ends - trans, -1).astype(np.int32)
    sid = np.repeat(np.arange(S, dtype=np.int32), lengths)
    with torch.cuda.device(device):
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        d_seq, d_sid, d_first, d_slot0 = up(seq), up(sid), up(offsets[:-1].astype(np.int32)), up(slot0)
        i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=device)
        checkin_cnt, cat_cnt, lo, hi, graph_cat, status = i32(P), i32(n_cat), i32(P), i32(P), i32(n_cat, n_cat), i32(1)
        keys = torch.empty(T, dtype=torch.int64, device=device)
        _universe.launch("mobgt_universe_counts", _p(d_seq), _p(d_sid), M, _p(d_first), _p(d_slot0), S, P, n_cat, _p(checkin_cnt),
                         _p(cat_cnt), _p(lo), _p(hi), _p(graph_cat), _p(keys), T, _p(status), _stream())
        bits = int(status[0])
        if bits:
            raise ValueError(f"universe_counts: the kernel skipped check-ins (status {bits}: an id outside 1 .. P / 1 .. n_cat or a "
                             "session index that does not match the offsets), which the host checks should have refused")
        poi_cat = torch.from_numpy(_one_category(lo.cpu().numpy(), hi.cpu().numpy())).to(device)
        graph = transition_csr(keys, P)
    return UniverseCounts(P, n_cat, T, checkin_cnt, cat_cnt, poi_cat, _check_freq(cat_cnt, poi_cat), graph_cat, graph)


# ---- check-ins and coordinates in, a Graphormer's universe out ----------------------------------------------------------------------
@dataclasses.dataclass
class BuiltUniverse:
    """`universe`: a synth.Universe for Graphormer(universe=) -- poi_table [P, 6] f64, graph_cat f32, graph_dist = the
    geo.RadiusGraph, graph_adj = the TransitionGraph, distance = None (pass num_bins = bins.num_bins + 2 to the model);
    `bins`: the geo.DistanceBins for the collator (bin_table=bins.table, or geo.pair_bins(coords, bins=bins));
    `counts`: the UniverseCounts; `coords`: [P, 2] f64 degrees."""
    universe: object
    bins: object
    counts: UniverseCounts
    coords: np.ndarray

    def write_csvs(self, directory):
        """Graph_poi.csv, Graph_cat.csv, Graph_adj.csv and Graph_dist.csv in `directory`, in the form the reference's model
        reads them (pd.read_csv): no index column, the graphs' headers 1 .. K as foursquare_process.py:670-752 writes them,
        Graph_poi's header synth.Universe.poi_columns.  The two POI graphs are written as dense [P, P] frames: refused above
        MAX_CSV_P POIs."""
        import pandas as pd
        P = self.counts.P
        if P > MAX_CSV_P:
            raise ValueError(f"write_csvs: {P} POIs, the dense [P, P] frames of Graph_adj.csv and Graph_dist.csv are written up to "
                             f"{MAX_CSV_P} POIs only; the graphs themselves are universe.graph_adj / universe.graph_dist")
        os.makedirs(directory, exist_ok=True)
        t = self.universe.poi_table
        poi = pd.DataFrame({name: t[:, k] if name in ("lat", "lon") else t[:, k].astype(np.int64) for k, name in enumerate(POI_COLUMNS)})
        poi.to_csv(os.path.join(directory, "Graph_poi.csv"), index=False)
        for name, m in (("Graph_cat.csv", self.universe.graph_cat), ("Graph_adj.csv", self.universe.graph_adj.to_dense()),
                        ("Graph_dist.csv", self.universe.graph_dist.to_dense01())):
            m = np.asarray(m, dtype=np.float64)
            pd.DataFrame(m, columns=np.arange(1, m.shape[1] + 1)).to_csv(os.path.join(directory, name), index=False)


def build_universe(ds, train, coords_deg, radius_km=3.0, device="cuda", forms=("mask", "csr"), table=True, P=None, n_cat=None):
    """Every session (a data.SessionDataset, train and test), which of them train, and coords [P, 2] latitude / longitude in
    degrees (POI 1 .. P in row order) -> BuiltUniverse: the counts of universe_counts, the within-radius graph of
    geo.radius_graph (`radius_km`, `forms`) and the distance bins of geo.distance_bins (`table`), all built on `device`.
    P defaults to the rows of coords."""
    from . import geo, synth
    ds = _dataset(ds)
    c = geo._coords(coords_deg, False)
    P = c.shape[0] if P is None else int(P)
    if c.shape[0] != P:
        raise ValueError(f"coords: {c.shape[0]} rows for P = {P} POIs")
    counts = universe_counts(ds, train, P=P, n_cat=n_cat, device=device)
    graph = geo.radius_graph(c, radius_km, device=device, forms=forms)
    bins = geo.distance_bins(c, device=device, table=table)
    users = np.asarray(ds.users)
    uni = synth.Universe(P=P, n_cat=counts.n_cat, n_user=int(users.max()) + 1 if users.size else 0, poi_table=counts.poi_table(c),
                         graph_adj=counts.graph_adj, graph_dist=graph, graph_cat=counts.graph_cat.cpu().numpy().astype(np.float32),
                         distance=None, poi_columns=POI_COLUMNS)
    return BuiltUniverse(uni, bins, counts, c)
