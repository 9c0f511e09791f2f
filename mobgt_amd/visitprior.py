"""A fitted per-user visit-frequency and recency prior on a model's next-POI scores: how often this user has been at a POI, and how
many of the user's check-ins ago the last time was, as two f32 tables over a CSR by user, added to the [G, V] scores that
Graphormer.metric_step / recommend_step rank -- on the device, in one launch (csrc_visitprior/visitprior.hip through _visitprior),
inside the loops' captured graphs.  People go back to the places they have been: prior.MarkovPrior's user term cu(u, a, p) counts
only where this user made exactly the transition a -> p before, so the user's favourite cafe scores nothing when today's anchor
is new; these two terms score it whatever the anchor is.

Inputs.  As MarkovBaseline.fit takes them: a data.SessionDataset `ds` of EVERY session (a PrefixDataset is refused: it holds every
check-in once per prefix), `train` a boolean mask or an index array over the sessions, dense POIs 1 .. P, users >= 0 and
U = the largest user + 1.

Counts: exact integers over the TRAIN sessions only.  The train rows of user u, in dataset order -- session index ascending, the
rows of a session in their order -- are numbered 0 .. N_u - 1.  For the output of data.sessionize, which splits every user's
sessions by time and keeps each user's sessions in time order, this is the user's log order; a hand-made dataset is numbered as
it is packed.  All rows of a train session count, the target row included, as for pop in baseline.py.

    n(u, p)    = how many of those rows have POI p
    last(u, p) = the largest number among those rows
    age(u, p)  = N_u - 1 - last(u, p), in 0 .. N_u - 1: 0 for the POI of the user's last train check-in

Storage: a CSR by user (VisitCounts).

    rowptr int64 [U + 1];  col int32 [nnz], the 0-based POI, strictly ascending inside a row;  cnt, age int32 [nnz];  tot int32 [U] = N_u

Tables: two f32 [nnz] tables, made on the host in numpy and rounded once (tables_from_counts); the same bits are uploaded for the
device and kept for the host, so no transcendental runs in a kernel.

    F[e] = prior.log_table(max cnt)[cnt[e]]                      = f32(log1p(cnt[e]))
    R[e] = f32(log((N_u + 1) / (age[e] + 1)))  in float64        (u the row of e)

Both are > 0 for every entry (cnt >= 1; age + 1 <= N_u), and inside a row R is largest for the POI visited last.  sessionize's
first train_split of a user's sessions are train, so "how recently" is counted from the end of what was trained on, and is the
same for every test sample of the user.

Blend.  The weights are ("visits", "recency").  Row g of the scores has u = user[g] - user_offset (batch.user is user + 1, as for
MarkovPrior).  If 0 <= u < U, every entry e of row u has the column c = col[e] + 1 - label_offset (model.label_offset); if c lies
in [0, V):

        v = scores[g, c]
        v = f32(v + f32(w_visits  * F[e]))
        v = f32(v + f32(w_recency * R[e]))
        out[g, c] = v

    visits first, then recency; every product and every sum rounded to f32 on its own, no FMA.  Every other element is copied bit
    for bit: -0.0, NaN payloads and +-inf survive.  A term with weight 0 is still added (x + 0 * T: a score of -0.0 becomes +0.0,
    and nothing else changes).  The history ids are not read: the prior has no anchor, so a sample with an empty history is scored
    too.  Entries whose column falls outside [0, V) are skipped silently: V and P need not agree.
  * Tables that are not what fit makes: a rowptr pair that is descending or beyond nnz makes the row count as empty, an entry of
    col outside [0, P) is skipped, and both raise SBADINDEX in the status word.  A row whose col does not ascend strictly is
    refused by VisitPrior's constructor; the kernel relies on the order for speed only, never for safety: no value read from a
    buffer is used as an index before it is range-checked, and no entry is applied outside the columns its workgroup owns.
  * The weights live in `prior.weights`, f32 [2] in device memory, read by the kernel; set_weights copies into it, so a captured
    graph that blends stays valid when the weights change.

`visit_counts_host`, `tables_from_counts` and `blend_host` are this rule in numpy: the kernels' references and the CPU forms.
prior.Stack(mb.prior(), mb.distance_prior(pb), cp, VisitPrior.fit(ds, train)) blends all four priors, one launch each.  `rows` of
a VisitPrior's blend is what MarkovPrior's is -- a collated batch (or any object with .x and .user) or a (hist, user) pair -- so a
stack with MarkovPrior keeps taking pairs.  The stack of four has 8 weights: fit_weights(scale_model=True) would fit 9 features and
is refused (priorfit.MAX_K = 8); fit_weights(scale_model=False) fits the 8 exactly."""
import collections

import numpy as np
import torch

from . import _visitprior
from .prior import MarkovPrior, Prior, check_weights, log_table

WEIGHTS = ("visits", "recency")                                         # the order of a weights row
SBADINDEX, SBADVALUE = _visitprior.SBADINDEX, _visitprior.SBADVALUE
KEY_LIMIT = 2 ** _visitprior.KEY_BITS

VisitCounts = collections.namedtuple("VisitCounts", "rowptr col cnt age tot U P")
VisitCounts.__doc__ = "numpy: rowptr int64 [U + 1], col int32 [nnz], cnt int32 [nnz], age int32 [nnz], tot int32 [U]; ints U, P"
VisitTables = collections.namedtuple("VisitTables", "rowptr col freq rec U P")
VisitTables.__doc__ = "numpy: rowptr int64 [U + 1], col int32 [nnz], freq (F) f32 [nnz], rec (R) f32 [nnz]; ints U, P"


def _prepare(ds, train, P, what):
    """baseline._prepare and this module's own limit -> (seq, offsets, users, mask, P, U)"""
    from .baseline import _prepare as prepare
    seq, offsets, users, mask, P, U = prepare(ds, train, P, what)
    if U * P >= KEY_LIMIT or U >= 2 ** 31:
        raise ValueError(f"{what}: {U} users x {P} POIs do not fit the key of the per-user table (U * P < 2**{_visitprior.KEY_BITS}, "
                         "U < 2**31): renumber the users densely")
    return seq, offsets, users, mask, P, U


def _numbering(offsets, users, mask, U):
    """-> (tot int32 [U] = N_u, ord0 int64 [S]: the number of a train session's first row among its user's train rows, 0 for
    the others): one stable sort and one cumsum over the sessions"""
    lengths = np.diff(offsets)
    mine = np.nonzero(mask)[0]
    order = mine[np.argsort(users[mine], kind="stable")]                # the train sessions by user, dataset order inside a user
    n = lengths[order]
    before = np.cumsum(n) - n                                           # rows of train sessions before this one, over all users
    tot = np.bincount(users[mine], weights=lengths[mine], minlength=U).astype(np.int64) if U else np.zeros(0, dtype=np.int64)
    starts = np.cumsum(tot) - tot                                       # ... before this user's first
    ord0 = np.zeros(len(lengths), dtype=np.int64)
    ord0[order] = before - starts[users[order]]
    return tot.astype(np.int32), ord0


def visit_counts_host(ds, train, P=None, what="visit_counts_host"):
    """The counts of the module's docstring -> VisitCounts.  ds, train, P: as MarkovBaseline.fit takes them; what: the caller's
    name in a refusal."""
    seq, offsets, users, mask, P, U = _prepare(ds, train, P, what)
    lengths = np.diff(offsets)
    tot, ord0 = _numbering(offsets, users, mask, U)
    sid = np.repeat(np.arange(len(lengths)), lengths)
    rows = np.nonzero(mask[sid])[0] if len(sid) else np.zeros(0, dtype=np.int64)
    s = sid[rows]
    number = ord0[s] + rows - offsets[:-1][s]
    key = users[s] * P + seq[rows, 0].astype(np.int64) - 1
    by_key = np.argsort(key, kind="stable")                             # the numbers ascend inside a run of equal keys
    key, number = key[by_key], number[by_key]
    uniq, first, cnt = np.unique(key, return_index=True, return_counts=True)
    last = number[first + cnt - 1] if len(uniq) else np.zeros(0, dtype=np.int64)
    owner = uniq // P
    rowptr = np.searchsorted(owner, np.arange(U + 1)).astype(np.int64)
    age = tot.astype(np.int64)[owner] - 1 - last
    return VisitCounts(rowptr, (uniq % P).astype(np.int32), cnt.astype(np.int32), age.astype(np.int32), tot, U, P)


def tables_from_counts(rowptr, cnt, age, tot):
    """-> (F f32 [nnz], R f32 [nnz]) of the module's docstring: F a gather from prior.log_table, R evaluated in float64 and rounded
    once."""
    rowptr, cnt, age, tot = (np.asarray(v) for v in (rowptr, cnt, age, tot))
    if any(v.ndim != 1 or v.dtype.kind not in "iu" for v in (rowptr, cnt, age, tot)) or cnt.shape != age.shape or len(rowptr) != len(tot) + 1:
        raise ValueError(f"tables_from_counts: integer rowptr [U + 1], cnt and age [nnz] and tot [U], got shapes {rowptr.shape}, {cnt.shape}, "
                         f"{age.shape}, {tot.shape}")
    width = np.diff(rowptr)
    if len(rowptr) < 1 or rowptr[0] != 0 or rowptr[-1] != len(cnt) or (width < 0).any():
        raise ValueError(f"tables_from_counts: rowptr must ascend from 0 to nnz = {len(cnt)}")
    n = np.repeat(tot.astype(np.int64), width)
    if (cnt < 1).any() or (age < 0).any() or (age >= n).any():
        raise ValueError("tables_from_counts: every entry needs cnt >= 1 and 0 <= age < N_u")
    freq = log_table(int(cnt.max()) if len(cnt) else 0)[cnt.astype(np.int64)]
    rec = np.log((n.astype(np.float64) + 1.0) / (age.astype(np.float64) + 1.0)).astype(np.float32)
    return freq, rec


def blend_host(scores, user, tables, weights, label_offset, user_offset=1, status=None):
    """The blend of the module's docstring -> f32 numpy [G, V].  scores [G, V] f32; user [G] (or [G, 1]) integers; tables a
    VisitTables; weights (w_visits, w_recency); status: a list or array whose [0] gets the SBADINDEX bit ORed in."""
    t = tables
    s = np.array(scores, dtype=np.float32)
    G, V = s.shape
    user = np.asarray(user).reshape(G)
    wv, wr = (np.float32(w) for w in np.asarray(weights, dtype=np.float64).reshape(-1))
    rowptr, col = np.asarray(t.rowptr), np.asarray(t.col)
    freq, rec = np.asarray(t.freq, dtype=np.float32), np.asarray(t.rec, dtype=np.float32)
    P, U, lo, nnz, bad = int(t.P), int(t.U), int(label_offset), len(col), 0
    for g in range(G):
        u = int(user[g]) - int(user_offset)
        if not 0 <= u < U:
            continue
        r0, r1 = int(rowptr[u]), int(rowptr[u + 1])
        if r0 < 0 or r1 < r0 or r1 > nnz:
            bad |= SBADINDEX
            continue
        q = col[r0:r1].astype(np.int64)
        good = (q >= 0) & (q < P)
        if not good.all():
            bad |= SBADINDEX
        c = q + 1 - lo
        at = np.nonzero(good & (c >= 0) & (c < V))[0]
        c, e = c[at], r0 + at
        v = (s[g, c] + (wv * freq[e]).astype(np.float32)).astype(np.float32)   # a product rounded to f32, then a sum rounded to f32
        s[g, c] = (v + (wr * rec[e]).astype(np.float32)).astype(np.float32)
    if status is not None:
        status[0] |= bad
    return s


class VisitPrior(Prior):
    """The fitted tables of the module's docstring on one device, their weights (visits, recency) and a status word (prior.Prior).

    P, U                   the POIs 1 .. P; the users 0 .. U - 1
    rowptr, col            int64 [U + 1], int32 [nnz] on the device
    cnt, age, tot          numpy int32 [nnz], [nnz], [U]: the counts the tables were made from
    freq, rec              F and R, f32 [nnz] on the device
    status                 the blend ORs SBADINDEX into it (a CPU prior's blend too)

    The constructor refuses tables the rule has no result for -- a rowptr that does not ascend from 0 to nnz, a col outside
    [0, P) or not strictly ascending inside a row -- with a ValueError: one torch check on the tables' device and one read-back.

    rows of blend: what MarkovPrior's are -- a collated batch (user = batch.user = user + 1; batch.x is passed on and not read)
    or a (hist [G, n], user [G]) pair of int32 / int64 tensors.  The launch is mobgt_visitprior_blend_rows."""

    NAME, WEIGHTS, LIB = "VisitPrior", WEIGHTS, _visitprior
    SKIPPED = ("table rows or entries", "a rowptr pair was descending or beyond nnz, or an entry of col was outside [0, P) -- the "
               "tables are not what VisitPrior.fit makes")
    HINTS = ("fit the prior on the loop's device (VisitPrior.fit(..., device=...))", "the prior was not fitted on the model's universe")

    def __init__(self, P, rowptr, col, cnt, age, tot, freq, rec, visits=1.0, recency=1.0, status=None):
        what = "VisitPrior"
        for name, v, dtype in (("rowptr", rowptr, torch.int64), ("col", col, torch.int32)):
            if not isinstance(v, torch.Tensor) or v.dtype != dtype or v.dim() != 1:
                got = f"{v.dtype} {tuple(v.shape)}" if isinstance(v, torch.Tensor) else type(v).__name__
                raise TypeError(f"{what}: {name} must be a {dtype} tensor of one dimension, got {got}")
        if rowptr.device != col.device:
            raise ValueError(f"{what}: rowptr is on {rowptr.device}, col on {col.device}: the tables live on one device")
        self.P, self.U, self.rowptr, self.col = int(P), int(rowptr.numel()) - 1, rowptr.contiguous(), col.contiguous()
        nnz = int(col.numel())
        self.cnt, self.age, self.tot = (np.ascontiguousarray(v, dtype=np.int32) for v in (cnt, age, tot))
        self._host_freq, self._host_rec = (np.ascontiguousarray(v, dtype=np.float32).reshape(-1) for v in (freq, rec))
        if self.U < 0 or self.P < 1 or self.U * self.P >= KEY_LIMIT or not len(self.cnt) == len(self.age) == len(self._host_freq) == len(self._host_rec) == nnz \
                or len(self.tot) != self.U:
            raise ValueError(f"{what}: rowptr [U + 1], tot [U] and col, cnt, age, freq, rec [nnz] with P >= 1 and U * P < 2**{_visitprior.KEY_BITS}; got "
                             f"U + 1 = {self.U + 1}, P = {self.P}, nnz = {nnz} and {len(self.tot)}, {len(self.cnt)}, {len(self.age)}, "
                             f"{len(self._host_freq)}, {len(self._host_rec)} entries")
        # what the kernel relies on for speed: one check on the tables' device, one read-back
        start = torch.zeros(nnz + 1, dtype=torch.bool, device=col.device)
        start[rowptr.clamp(0, nnz)] = True                              # (safe whatever rowptr holds)
        framed = (rowptr[0] == 0) & (rowptr[-1] == nnz) & (rowptr[1:] >= rowptr[:-1]).all()
        ascending = ((col[1:] > col[:-1]) | start[1:nnz]).all()
        inside = ((col >= 0) & (col < self.P)).all()
        framed, ascending, inside = torch.stack([framed, ascending, inside]).tolist()
        if not framed:
            raise ValueError(f"{what}: rowptr must ascend from 0 to nnz = {nnz}")
        if not inside:
            raise ValueError(f"{what}: an entry of col is outside [0, P) = [0, {self.P})")
        if not ascending:
            raise ValueError(f"{what}: col must ascend strictly inside every row (the blend finds a chunk's entries by bisection)")
        both = torch.from_numpy(np.stack([self._host_freq, self._host_rec])).to(self.device)      # one upload
        self.freq, self.rec = both[0], both[1]
        super().__init__([visits, recency], status)

    @property
    def device(self):
        return self.col.device

    @classmethod
    def fit(cls, ds, train, P=None, visits=1.0, recency=1.0, device="cuda"):
        """Count n and age over the train sessions of `ds`, make the tables.

        ds: a data.SessionDataset of EVERY session (a PrefixDataset is refused); train: a boolean mask over the sessions or the
        indices of the train sessions; P: default the largest POI id present.  Ids outside 1 .. P, negative users and
        U * P >= 2**62 are a ValueError on the host before any launch.

        On a GPU: one upload of the packed check-ins and of four arrays over the sessions (one cumsum and one stable sort on the
        host give every train session its first key slot and its starting number; N_u comes from the same pass), one launch that
        writes a 64-bit key and a number per train check-in (mobgt_visitprior_keys), torch.sort(stable=True), a launch that marks
        where the runs of equal keys begin (mobgt_universe_run_heads, the transition graph's), torch.cumsum, one read-back of
        nnz, one launch that writes rowptr, col, cnt and age (mobgt_visitprior_fill), one read-back of cnt and age and one of
        rowptr and the status word (tot is the host's already), the tables in numpy, one upload.  Element for element what
        visit_counts_host gives.  A CPU device is counted by visit_counts_host.  A
        status that is not zero is a ValueError before the tables are made."""
        what = "VisitPrior.fit"
        weights = check_weights([visits, recency], what, WEIGHTS)
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device.type != "cuda":
            c = visit_counts_host(ds, train, P, what)
            freq, rec = tables_from_counts(c.rowptr, c.cnt, c.age, c.tot)
            return cls(c.P, torch.from_numpy(c.rowptr), torch.from_numpy(c.col), c.cnt, c.age, c.tot, freq, rec, float(weights[0]), float(weights[1]))
        from . import _universe
        from .ops import _p, _stream
        seq, offsets, users, mask, P, U = _prepare(ds, train, P, what)
        M, S = int(seq.shape[0]), len(offsets) - 1
        lengths = np.diff(offsets)
        tot, ord0 = _numbering(offsets, users, mask, U)
        rows = np.where(mask, lengths, 0)
        ends = np.cumsum(rows)
        T = int(ends[-1]) if S else 0
        slot0 = np.where(mask, ends - rows, -1).astype(np.int64)
        sid = np.repeat(np.arange(S, dtype=np.int32), lengths)
        with torch.cuda.device(device):
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
            d_seq, d_sid, d_first, d_slot0, d_ord0, d_users, d_tot = up(seq), up(sid), up(offsets[:-1]), up(slot0), up(ord0), up(users), up(tot)
            keys = torch.empty(T, dtype=torch.int64, device=device)
            number = torch.empty(T, dtype=torch.int32, device=device)
            word = torch.zeros(1, dtype=torch.int32, device=device)
            rowptr = torch.empty(U + 1, dtype=torch.int64, device=device)
            _visitprior.launch("mobgt_visitprior_keys", _p(d_seq), _p(d_sid), M, _p(d_first), _p(d_slot0), _p(d_ord0), _p(d_users), S, P, U,
                               _p(keys), _p(number), T, _p(word), _stream())
            if T:
                keys, by_key = torch.sort(keys, stable=True)
                number = number[by_key]
                head = torch.empty(T, dtype=torch.int32, device=device)
                _universe.launch("mobgt_universe_run_heads", _p(keys), T, _p(head), _stream())
                pos = torch.cumsum(head, 0, dtype=torch.int64)
                nnz = int(pos[-1])
            else:
                pos, nnz = keys, 0
            out = torch.empty(3, nnz, dtype=torch.int32, device=device)    # col, cnt, age
            _visitprior.launch("mobgt_visitprior_fill", _p(keys), _p(number), _p(pos), T, P, U, nnz, _p(d_tot), _p(rowptr), _p(out[0]), _p(out[1]),
                               _p(out[2]), _p(word), _stream())
            counts = out[1:].cpu().numpy()                              # (synchronises: the status word is final)
            cls.refuse(int(word[0]), what)                              # (before the tables: counts with skipped rows mean nothing)
            freq, rec = tables_from_counts(rowptr.cpu().numpy(), counts[0], counts[1], tot)
            return cls(P, rowptr, out[0], counts[0], counts[1], tot, freq, rec, float(weights[0]), float(weights[1]), status=word)

    def tables(self):
        """-> VisitTables: rowptr, col and the two tables as numpy arrays (one download, kept), what blend_host takes."""
        if self._host_tables is None:
            self._host_tables = VisitTables(self.rowptr.detach().cpu().numpy(), self.col.detach().cpu().numpy(), self._host_freq, self._host_rec,
                                            self.U, self.P)
        return self._host_tables

    def counts(self):
        """-> VisitCounts: the integers the tables were made from, numpy."""
        t = self.tables()
        return VisitCounts(t.rowptr, t.col, self.cnt, self.age, self.tot, self.U, self.P)

    _rows = staticmethod(MarkovPrior._rows)

    def _blend_host(self, scores, ids, w, label_offset):
        status = [0]
        res = blend_host(scores, ids[1], self.tables(), w, label_offset, status=status)
        self.status |= status[0]
        return res

    def _launch(self, head, ids, w, _p, code, stream):
        user = ids[1]
        _visitprior.launch("mobgt_visitprior_blend_rows", *head, _p(user), code(user), max(user.stride(0), 1), 1, _p(self.rowptr), _p(self.col),
                           _p(self.freq), _p(self.rec), int(self.col.numel()), self.U, self.P, _p(w), _p(self.status), stream)
