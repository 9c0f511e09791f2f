"""The Markov baseline of next-POI prediction: counting transitions, scored on the same samples, with the same metrics and the
same tie rule as a Graphormer under train.EvalLoop -- exact target ranks and top-k lists.

Inputs.  A data.SessionDataset `ds` of EVERY session, with dense POI ids 1 .. P and users >= 0; `train`, a bool mask or an index
array over the sessions, as universe_counts takes it; P, default the largest id present.

Tables.  All are counted over the TRAIN sessions only, so nothing of a test session leaks.  UniverseCounts.checkin_cnt is NOT
used: it counts all sessions, train and test.

    cg(a, b)     the consecutive row pairs a -> b inside one train session.  All L transitions of a session count, the one into
                 its target row included; self transitions count.  Exactly UniverseCounts.graph_adj.
    cu(u, a, b)  the same pairs, counted separately per user u: the reference's per-user `transfer` matrix before its row
                 normalisation (graphormer/train.py:391-470), which does not change an order within a row.
    pop(p)       the rows of train sessions with POI p.
    pop_rank     a permutation of the POIs: the 0-based position of p when the POIs are ordered by pop descending, equal counts
                 lower id first -- the project's tie rule, lower POI first.

A sample is a (session s, cut c) pair as PrefixStats / PrefixDataset hold them: user u = users[s], previous POI a = poi(r_{c-1}),
target t = poi(r_c), history r_0 .. r_{c-1}.  A plain SessionDataset is the samples (s, L_s).

The order.  Candidate p in 1 .. P has the key K(p) = (cu(u, a, p), cg(a, p), -pop_rank(p)).  Keys compare lexicographically,
larger first.  pop_rank is a permutation, so the order is strict and total: there are no ties, every target has a rank, and the
ACC position and the MRR position coincide.  `order` selects how much of the key is used:

    "user"        the full key
    "global"      cu is taken as 0
    "popularity"  cu and cg are taken as 0

Results.  rank(q) = #{p : K(p) > K(t)}, 0-based; revisit(q) = 1 if t is among the history POIs, else 0; the list: ids[q, j] is the
POI of rank j for j < min(k, P), and -1 beyond.

Sparse form for the device.  G_a is row a of the cg CSR; every (u, a, .) entry of cu is also an entry of G_a.  The kernels
(csrc_baseline/baseline.hip through _baseline) evaluate

    rank = #{p in G_a : K(p) > K(t)} + [cg(a, t) == 0] * (pop_rank(t) - #{p in G_a : pop_rank(p) < pop_rank(t)})

and build a list from the best entries of G_a followed by the most popular POIs outside it: no [rows, P] array is made.

Differences from the reference's markov() (graphormer/train.py:391-470).  The reference restricts the candidates to the user's own
train POIs; it replaces a prediction at the last index of that list by np.random.randint; it takes its top 5 from an unstable
argsort; it has no back-off, so a previous POI it never saw scores nothing; and it averages per user.  Its output cannot be
reproduced bit for bit, so there is no golden.  Here the back-off (cg, then popularity) makes every sample scoreable, and the
averages are over samples, as EvalLoop's are.

`ranks_host` / `topk_host` are the rule as a plain definition (dict counters straight from the sessions, one np.lexsort over all P
candidates per sample): the kernels' reference and the CPU form."""
import numpy as np
import torch

from . import _baseline, metrics

ORDERS = {"user": 0, "global": 1, "popularity": 2}                     # (= _baseline.ORDER_*)
DEVICE_MAX_L = _baseline.MAX_L                                          # (the header's: include/mobgt_baseline.h)
MAX_K = _baseline.MAX_K
_KS = (1, 5, 10, 20)


# ---- what every form checks on the host -------------------------------------------------------------------------------------------
def _prepare(ds, train, P, what):
    """-> (seq int32 [M, 3], offsets int64 [S + 1], users int64 [S], train mask bool [S], P, U), every TypeError / ValueError
    raised.  The rules universe._prepare shares are worded as there."""
    from .data import SessionDataset
    from .prefixes import PrefixDataset
    from .universe import _first_session
    if isinstance(ds, PrefixDataset):
        raise TypeError(f"{what}: the tables are counted over sessions, and a PrefixDataset holds every transition of a session once "
                        "per prefix that contains it: give its base, pds.base")
    if not isinstance(ds, SessionDataset):
        raise TypeError(f"{what}: the sessions must be a data.SessionDataset, got {type(ds).__name__} (data.SessionDataset(sessions) "
                        "validates and packs them)")
    seq, offsets, users = ds.seq, np.asarray(ds.offsets, dtype=np.int64), np.asarray(ds.users, dtype=np.int64)
    M, S = int(seq.shape[0]), len(offsets) - 1
    if M >= 2 ** 31:
        s = int(np.searchsorted(offsets, 2 ** 31 - 1, side="right")) - 1
        raise ValueError(f"session {s}: check-in number 2**31 of {M} lies in it, the kernels index check-ins with 31 bits "
                         "(M < 2**31): count the sessions in parts")
    t = np.asarray(train)
    if t.dtype == np.bool_:
        if t.shape != (S,):
            raise ValueError(f"train: a mask of {t.shape[0] if t.ndim == 1 else t.shape} flags for {S} sessions")
        mask = np.ascontiguousarray(t)
    else:
        if t.size and not np.issubdtype(t.dtype, np.integer):
            raise ValueError(f"train: a boolean mask of length {S} or integer session indices, got {t.dtype}")
        t = t.reshape(-1).astype(np.int64)
        if t.size and (t.min() < 0 or t.max() >= S):
            raise ValueError(f"train: session index {int(t[(t < 0) | (t >= S)][0])} is not in 0 .. {S - 1}")
        mask = np.zeros(S, dtype=bool)
        mask[t] = True
    if P is not None and (not isinstance(P, (int, np.integer)) or isinstance(P, bool)):
        raise TypeError(f"{what}: P must be an integer, got {type(P).__name__}")
    v = seq[:, 0]
    top = int(v.max()) if M else 0
    limit = min(top if P is None else int(P), 2 ** 31 - 1)
    if P is not None and limit < 1:
        raise ValueError(f"{what}: POI count {limit}, at least 1 is needed")
    bad = (v < 1) | (v > limit)
    if bad.any():
        s, i = _first_session(offsets, bad)
        raise ValueError(f"session {s}: POI id {int(v[i])} at check-in {i - int(offsets[s])} is not in 1 .. {limit} "
                         f"(dense ids: data.first_seen_ids)")
    P = max(limit, 1)
    if S and users.min() < 0:
        s = int(np.argmax(users < 0))
        raise ValueError(f"session {s}: user {int(users[s])} is negative, the per-user table is keyed by users >= 0")
    U = int(users.max()) + 1 if S else 0
    if U * P * P >= 2 ** 63:
        raise ValueError(f"{what}: {U} users x {P} x {P} POI pairs do not fit the 63-bit key of the per-user table "
                         "(U * P * P < 2**63): renumber the users densely")
    return np.ascontiguousarray(seq, dtype=np.int32), offsets, users, mask, int(P), U


def _order(order):
    if order not in ORDERS:
        raise ValueError(f"order must be one of {', '.join(repr(o) for o in ORDERS)}, got {order!r}")
    return ORDERS[order]


def _samples(samples, P, what):
    """A PrefixDataset or a SessionDataset -> (its base SessionDataset, session int32 [Q], cut int32 [Q]); the POI ids of the base
    are checked against P."""
    from .data import SessionDataset
    from .prefixes import PrefixDataset
    from .universe import _first_session
    if isinstance(samples, PrefixDataset):
        base, session, cut = samples.base, samples.session, samples.cut
    elif isinstance(samples, SessionDataset):
        base = samples
        session, cut = np.arange(len(base), dtype=np.int32), (np.diff(base.offsets) - 1).astype(np.int32)
    else:
        raise TypeError(f"{what}: the samples must be a data.PrefixDataset or a data.SessionDataset, got {type(samples).__name__}")
    v = base.seq[:, 0]
    bad = (v < 1) | (v > P)
    if bad.any():
        s, i = _first_session(base.offsets, bad)
        raise ValueError(f"{what}: session {s} of the samples: POI id {int(v[i])} at check-in {i - int(base.offsets[s])} is not in "
                         f"1 .. {P}, the POIs the baseline was fitted with")
    if int(base.seq.shape[0]) >= 2 ** 31:
        raise ValueError(f"{what}: {int(base.seq.shape[0])} check-ins, the kernels index them with 31 bits (M < 2**31)")
    return base, np.ascontiguousarray(session, dtype=np.int32), np.ascontiguousarray(cut, dtype=np.int32)


def _k(k):
    if not isinstance(k, (int, np.integer)) or isinstance(k, bool) or not 1 <= k <= MAX_K:
        raise ValueError(f"k must be an integer in 1 .. {MAX_K} (one lane of a wave per position), got {k!r}")
    return int(k)


# ---- the rule as a plain definition -----------------------------------------------------------------------------------------------
def _host(ds, train, samples, order, k, P):
    """-> (rank int32 [Q], revisit uint8 [Q], ids int32 [Q, k] or None for k = None)."""
    seq, offsets, users, mask, P, _ = _prepare(ds, train, P, "ranks_host")
    mode = _order(order)
    base, session, cut = _samples(samples, P, "ranks_host")
    cg, cu, pop = {}, {}, [0] * (P + 1)                                # cg[a][b], cu[(u, a)][b], pop[p]
    poi, off = seq[:, 0].tolist(), offsets.tolist()
    for s in np.nonzero(mask)[0].tolist():
        u = int(users[s])
        rows = poi[off[s]:off[s + 1]]
        for p in rows:
            pop[p] += 1
        for a, b in zip(rows[:-1], rows[1:]):
            row = cg.setdefault(a, {})
            row[b] = row.get(b, 0) + 1
            row = cu.setdefault((u, a), {})
            row[b] = row.get(b, 0) + 1
    by_pop = sorted(range(1, P + 1), key=lambda p: (-pop[p], p))     # equal counts: lower id first
    pop_rank = np.empty(P, dtype=np.int64)
    pop_rank[np.asarray(by_pop, dtype=np.int64) - 1] = np.arange(P)
    Q = len(session)
    rank, revisit = np.zeros(Q, dtype=np.int32), np.zeros(Q, dtype=np.uint8)
    ids = None if k is None else np.full((Q, k), -1, dtype=np.int32)
    bpoi, boff, busers = base.seq[:, 0], base.offsets, base.users
    for q in range(Q):
        s, c = int(session[q]), int(cut[q])
        first = int(boff[s])
        a, t, u = int(bpoi[first + c - 1]), int(bpoi[first + c]), int(busers[s])
        kg, ku = np.zeros(P, dtype=np.int64), np.zeros(P, dtype=np.int64)
        if mode <= ORDERS["global"]:
            for b, n in cg.get(a, {}).items():
                kg[b - 1] = n
        if mode == ORDERS["user"]:
            for b, n in cu.get((u, a), {}).items():
                ku[b - 1] = n
        best_first = np.lexsort((pop_rank, -kg, -ku))                  # (the last key is the first compared)
        rank[q] = int(np.nonzero(best_first == t - 1)[0][0])
        revisit[q] = int(t in bpoi[first:first + c])
        if ids is not None:
            m = min(k, P)
            ids[q, :m] = best_first[:m] + 1
    return rank, revisit, ids


def ranks_host(ds, train, samples, order="user", P=None):
    """The rule of the module's docstring, sample by sample -> (rank int32 [Q], revisit uint8 [Q]) numpy.  `ds`, `train`, `P`: what
    the tables are counted over, as MarkovBaseline.fit takes them; `samples`: a PrefixDataset or a SessionDataset."""
    rank, revisit, _ = _host(ds, train, samples, order, None, P)
    return rank, revisit


def topk_host(ds, train, samples, order="user", k=20, P=None):
    """The list of the module's docstring -> ids int32 [Q, k] numpy: 1-based POIs, best first, -1 from position P on."""
    return _host(ds, train, samples, order, _k(k), P)[2]


# ---- the fitted tables ------------------------------------------------------------------------------------------------------------
def _metrics_of(rank, sel=None):
    """Ranks (a device or host int tensor [Q]) -> the dict of metrics.finalize over the samples `sel` selects (all of them)."""
    r = rank if sel is None else rank[sel]
    r = r.double()
    acc = torch.zeros(len(metrics.ACC_FIELDS), dtype=torch.float64, device=r.device)
    acc[0] = r.numel()
    gain = 1.0 / torch.log2(r + 2.0)
    for i, k in enumerate(_KS):
        hit = r < k
        acc[1 + i] = hit.sum()
        acc[5 + i] = gain[hit].sum()
    acc[9] = (1.0 / (r + 1.0)).sum()
    return metrics.finalize(acc)


class MarkovBaseline:
    """The fitted tables of the module's docstring on one device.

    P, U            POIs 1 .. P; the per-user table is keyed for users 0 .. U - 1 (U = the largest user of `ds` + 1)
    graph           universe.TransitionGraph: the cg CSR (rowptr int64 [P + 1], col / val int32 [nnz])
    ukey, uval      the cu table: int64 [nnzU] sorted distinct keys (u * P + a - 1) * P + (b - 1), int32 [nnzU] counts
    pop             int32 [P] rows of train sessions at each POI
    pop_rank        int32 [P] the permutation of the docstring; pop_order int32 [P] is its inverse"""

    def __init__(self, P, U, graph, ukey, uval, pop, pop_rank, pop_order, fitted_on):
        self.P, self.U, self.graph, self.ukey, self.uval = P, U, graph, ukey, uval
        self.pop, self.pop_rank, self.pop_order = pop, pop_rank, pop_order
        self._fitted_on = fitted_on                                    # (ds, train mask): what the host form counts over

    @property
    def device(self):
        return self.pop_rank.device

    @classmethod
    def fit(cls, ds, train, P=None, device="cuda"):
        """Count the tables over the train sessions of `ds`.  On a GPU: one upload of seq, offsets, users and the mask, torch index
        arithmetic for the keys, universe.transition_csr for cg, torch.sort + torch.unique_consecutive for cu and one stable
        descending torch.sort for pop_rank.  `device="cpu"` builds the same tables in numpy."""
        from .universe import TransitionGraph, transition_csr
        device = torch.device(device)
        seq, offsets, users, mask, P, U = _prepare(ds, train, P, "MarkovBaseline.fit")
        M, S = seq.shape[0], len(offsets) - 1
        lengths = np.diff(offsets)
        if device.type != "cuda":
            poi = seq[:, 0].astype(np.int64)
            sid = np.repeat(np.arange(S), lengths)
            rows = mask[sid] if M else np.zeros(0, dtype=bool)
            inner = np.ones(M, dtype=bool)
            inner[offsets[:-1][offsets[:-1] < M]] = False             # a session's first check-in follows nothing
            at = np.nonzero(inner & rows)[0]
            a, b = poi[at - 1] - 1, poi[at] - 1
            gkey, gval = np.unique(a * P + b, return_counts=True)
            rowptr = np.searchsorted(gkey // P, np.arange(P + 1)).astype(np.int64)
            ukey, uval = np.unique((users[sid[at]] * P + a) * P + b, return_counts=True)
            pop = np.bincount(poi[rows] - 1, minlength=P)
            pop_order = np.argsort(-pop, kind="stable")
            pop_rank = np.empty(P, dtype=np.int64)
            pop_rank[pop_order] = np.arange(P)
            t, i32 = torch.from_numpy, lambda v: torch.from_numpy(v.astype(np.int32))
            graph = TransitionGraph(P, t(rowptr), i32(gkey % P), i32(gval))
            return cls(P, U, graph, t(ukey.astype(np.int64)), i32(uval), i32(pop), i32(pop_rank), i32(pop_order), (ds, mask))
        with torch.cuda.device(device):
            up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(device)
            d_seq, d_first, d_len, d_users, d_mask = up(seq), up(offsets[:-1]), up(lengths), up(users), up(mask)
            poi = d_seq[:, 0].long()
            sid = torch.repeat_interleave(torch.arange(S, device=device), d_len, output_size=M)
            rows = d_mask[sid]
            inner = torch.ones(M, dtype=torch.bool, device=device)
            inner[d_first[d_first < M]] = False
            at = torch.nonzero(inner & rows).reshape(-1)
            a, b = poi[at - 1] - 1, poi[at] - 1
            graph = transition_csr(a * P + b, P)
            ukey, uval = torch.unique_consecutive(torch.sort((d_users[sid[at]] * P + a) * P + b).values, return_counts=True)
            pop = torch.bincount(poi[rows] - 1, minlength=P)
            pop_order = torch.sort(pop, descending=True, stable=True).indices
            pop_rank = torch.empty(P, dtype=torch.int64, device=device)
            pop_rank[pop_order] = torch.arange(P, device=device)
            return cls(P, U, graph, ukey, uval.int(), pop.int(), pop_rank.int(), pop_order.int(), (ds, mask))

    # ---- the two launches
    def _upload(self, samples, what):
        base, session, cut = _samples(samples, self.P, what)
        if len(cut) and int(cut.max()) > DEVICE_MAX_L:
            q = int(np.argmax(cut > DEVICE_MAX_L))
            raise ValueError(f"{what}: sample {q} (session {int(session[q])}) has a history of {int(cut[q])} check-ins, the device "
                             f"forms take up to {DEVICE_MAX_L}, as the collator does; the host form is baseline.ranks_host")
        up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(self.device)
        return (up(base.seq), up(np.asarray(base.offsets, dtype=np.int64)), up(np.asarray(base.users, dtype=np.int64)),
                len(base), int(base.seq.shape[0]), up(session), up(cut), len(session))

    def _tables(self):
        from .ops import _p
        g = self.graph
        return (_p(g.rowptr), _p(g.col), _p(g.val), g.nnz, _p(self.ukey), _p(self.uval), int(self.ukey.numel()), self.U)

    @staticmethod
    def _checked(status, out, what):
        bits = int(status[0])
        if bits:
            failed = torch.nonzero(out.reshape(out.shape[0], -1)[:, 0] < 0).reshape(-1)
            where = f", the first of them sample {int(failed[0])}" if failed.numel() else ""
            raise ValueError(f"{what}: the kernel skipped samples or table entries (status {bits}){where}: an index was out of range "
                             "when the kernel read it, which the host checks should have refused")

    def ranks(self, samples, order="user"):
        """-> (rank int32 [Q], revisit uint8 [Q]) tensors on the baseline's device.  `samples`: a PrefixDataset or a SessionDataset
        whose POI ids lie in 1 .. P (checked on the host; the ValueError names the first offending session).  A user without a
        row in the per-user table backs off to cg and popularity.  One upload of the samples, one launch
        (mobgt_baseline_ranks), one read-back of the status word; a status that is not zero is a ValueError."""
        mode = _order(order)
        if self.device.type != "cuda":
            rank, revisit = ranks_host(*self._fitted_on, samples, order, P=self.P)
            return torch.from_numpy(rank), torch.from_numpy(revisit)
        from .ops import _p, _stream
        with torch.cuda.device(self.device):
            d_seq, d_off, d_users, S, M, d_session, d_cut, Q = self._upload(samples, "MarkovBaseline.ranks")
            rank = torch.empty(Q, dtype=torch.int32, device=self.device)
            revisit = torch.empty(Q, dtype=torch.uint8, device=self.device)
            status = torch.empty(1, dtype=torch.int32, device=self.device)
            _baseline.launch("mobgt_baseline_ranks", _p(d_seq), _p(d_off), _p(d_users), S, M, _p(d_session), _p(d_cut), Q,
                             *self._tables(), _p(self.pop_rank), self.P, mode, _p(rank), _p(revisit), _p(status), _stream())
            self._checked(status, rank, "MarkovBaseline.ranks")
        return rank, revisit

    def recommend(self, samples, k=20, order="user"):
        """-> ids int32 [Q, k] on the baseline's device: the k best POIs of every sample, best first, -1 from position P on.
        1 <= k <= 64.  One launch (mobgt_baseline_topk)."""
        mode, k = _order(order), _k(k)
        if self.device.type != "cuda":
            return torch.from_numpy(topk_host(*self._fitted_on, samples, order, k, P=self.P))
        from .ops import _p, _stream
        with torch.cuda.device(self.device):
            d_seq, d_off, d_users, S, M, d_session, d_cut, Q = self._upload(samples, "MarkovBaseline.recommend")
            ids = torch.empty(Q, k, dtype=torch.int32, device=self.device)
            status = torch.empty(1, dtype=torch.int32, device=self.device)
            _baseline.launch("mobgt_baseline_topk", _p(d_seq), _p(d_off), _p(d_users), S, M, _p(d_session), _p(d_cut), Q,
                             *self._tables(), _p(self.pop_rank), _p(self.pop_order), self.P, mode, k, _p(ids), _p(status), _stream())
            self._checked(status, ids, "MarkovBaseline.recommend")
        return ids

    def prior(self, user=1.0, transition=1.0, popularity=1.0):
        """-> prior.MarkovPrior on the baseline's device: f32 log-counts of cu, cg and pop with these weights, to be added to a
        model's scores (EvalLoop / PredictLoop(prior=...), Graphormer.metric_step / recommend_step(prior=...)).  The rule is the
        docstring of mobgt_amd/prior.py."""
        from .prior import MarkovPrior
        return MarkovPrior.from_baseline(self, user, transition, popularity)

    def distance_prior(self, pair_bins, distance=1.0):
        """-> geoprior.DistancePrior on the baseline's device: the log of how much more often than chance a train transition lands
        in each distance bin of `pair_bins` (a geo.PairBins of the same POIs, on the same device), with this weight, to be added
        to a model's scores alone or in a prior.Stack beside prior().  The rule is the docstring of mobgt_amd/geoprior.py."""
        from .geoprior import DistancePrior
        return DistancePrior.fit(self, pair_bins, distance)

    def evaluate(self, samples, order="user", split_revisits=False):
        """-> the dict of metrics.finalize (acc@1/5/10/20, ndcg@1/5/10/20, mrr, n) over the samples, computed from the ranks in f64
        torch: hit rank < k, gain 1 / log2(rank + 2), reciprocal rank 1 / (rank + 1).  The order is strict, so the ACC and the MRR
        position are the same number.  `split_revisits`: also "new" and "revisit", dicts of the same keys over the samples whose
        target is not / is among their history POIs.  Keys and meaning are train.EvalLoop's."""
        rank, revisit = self.ranks(samples, order)
        out = _metrics_of(rank)
        if split_revisits:
            out["new"], out["revisit"] = _metrics_of(rank, revisit == 0), _metrics_of(rank, revisit != 0)
        return out
