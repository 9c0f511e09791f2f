"""A fitted category-transition and time-of-day prior on a model's next-POI scores: how much more often than its marginal a
category follows the anchor's category, and how much more often it follows a check-in at the anchor's time of day, as two f32
tables over the categories, added to the [G, V] scores that Graphormer.metric_step / recommend_step rank -- on the device, in one
launch (csrc_ctxprior/ctxprior.hip through _ctxprior), inside the loops' captured graphs.  prior.MarkovPrior scores a POI the
anchor never led to by popularity only, geoprior.DistancePrior by how far away it is; these two terms tell a bar from an office
after a restaurant, and at 8 in the morning from 10 at night.

Sizes.  C = n_cat categories, numbered 1 .. C.  S = n_slots time slots, numbered 0 .. S - 1; slot 0 is a real slot (checkins.py
makes slots as (t mod 86400) div 1800).  poi_cat[p - 1] in 0 .. C is the category of POI p, 0 a POI without a check-in:
UniverseCounts.poi_cat, counted over ALL sessions (a POI with two categories is refused there).

Counts: two exact integer tables over the TRAIN sessions only.  The pairs are the consecutive rows (k - 1, k) inside one session;
the pair into the target row is included and no pair spans two sessions -- the pairs of graph_cat and graph_adj.

    gc[a - 1, b - 1] = the pairs whose categories are a -> b: UniverseCounts.graph_cat, reused, not counted again    [C, C]
    st[s, b - 1]     = the pairs whose FIRST row has slot s and whose second row has category b                      [S, C] int64

A pair whose slot lies outside [0, S) or whose destination category lies outside 1 .. C is skipped and flagged (SBADVALUE), a
session whose offsets pair is descending or outside [0, M] is skipped and flagged (SBADINDEX); fit checks both on the host first,
the status bits are the kernel's own defence.

The slot is that of the PREVIOUS check-in, not of the target: neither the model nor the collator sees the target's time, and a
prior that used it would score with information the model does not get.

Tables.  With m[b] = sum_a gc[a, b] and M = sum(m):

    base[b]  = log((m[b] + 1) / (M + C))
    Tc[a, b] = f32( log((gc[a, b] + 1) / (sum_b gc[a, :] + C)) - base[b] )      [C, C]
    Tt[s, b] = f32( log((st[s, b] + 1) / (sum_b st[s, :] + C)) - base[b] )      [S, C]

each the log of how much more often than its marginal a category follows this category, or this slot; the add-one terms keep
empty cells finite.  The popularity of a POI inside its category is MarkovPrior's popularity term: the terms complement each
other and count nothing twice.  Both tables are evaluated in numpy float64 on the host and rounded once (tables_from_counts);
the same f32 bits are uploaded for the device and kept for the host: no transcendental runs in a kernel.

Blend.  Row g of the scores has the node ids hist[g, 0:n], and time[g, 0:n] and cat[g, 0:n] at the same positions: batch.x,
batch.time and batch.cat, which the collators leave as raw integers [G, N, 1].
  * The anchor position j is the LAST position whose id is not 0 -- the other priors' anchor, the one near="last" documents: the
    last history check-in for graphs made from sessions (nodes ordered by their last visit, time and cat those of that visit), not
    necessarily for a hand-made dict.  No such position, or an id hist[g, j] outside 1 .. P: the row is copied.
  * ca = cat[g, j], ta = time[g, j]: the raw integer slot, not int(time_normal * 48).
  * Column c is POI p = c + label_offset (model.label_offset).  For 1 <= p <= P let k = poi_cat[p - 1]; for 1 <= k <= C:

        v = scores[g, c]
        if 1 <= ca <= C:   v = f32(v + f32(w_category * Tc[ca - 1, k - 1]))
        if 0 <= ta <  S:   v = f32(v + f32(w_time     * Tt[ta,     k - 1]))
        out[g, c] = v

    category first, then time; every product and every sum rounded to f32 on its own, no FMA.  Every other element is copied
    bit for bit: -0.0, NaN payloads and +-inf survive.  A term with weight 0 is still added (x + 0 * T: a score of -0.0 becomes
    +0.0 where the table entry is not negative, and nothing else changes).  No value read from a buffer is used as an index
    before it is checked against what it indexes.
  * The weights are ("category", "time"): `prior.weights`, f32 [2] in device memory, read by the kernel; set_weights copies into
    it, so a captured graph that blends stays valid when the weights change.

`slot_hist_host`, `tables_from_counts` and `blend_host` are this rule in numpy: the kernels' references and the CPU forms.
prior.Stack(mb.prior(), mb.distance_prior(pb), ContextPrior.fit(ds, train)) blends all three priors, one launch each.  `rows` of a
ContextPrior's blend is a collated batch (or any object with .x, .time, .cat) or a (hist, time, cat) triple; MarkovPrior takes a
batch or a (hist, user) pair only, so a stack that holds both is given a batch (an object with .x, .user, .time, .cat)."""
import collections

import numpy as np
import torch

from . import _ctxprior
from .prior import Prior, check_weights

WEIGHTS = ("category", "time")                                          # the order of a weights row
SBADINDEX, SBADVALUE = _ctxprior.SBADINDEX, _ctxprior.SBADVALUE
MAX_CAT, MAX_SLOTS = _ctxprior.MAX_CAT, _ctxprior.MAX_SLOTS

ContextTables = collections.namedtuple("ContextTables", "poi_cat cat_table slot_table P n_cat n_slots")
ContextTables.__doc__ = "numpy: poi_cat int32 [P], cat_table f32 [n_cat, n_cat], slot_table f32 [n_slots, n_cat]; ints P, n_cat, n_slots"


def slot_hist_host(seq, offsets, train, n_slots, n_cat, status=None):
    """st of the module's docstring -> int64 [n_slots, n_cat].  seq [M, 3] rows (poi, slot, category); offsets [S + 1]; train [S]
    flags (not 0: a train session).  A session whose offsets pair is descending or lies outside [0, M] is skipped and ORs
    SBADINDEX into status[0] (a list or an array); a pair whose slot is outside [0, n_slots) or whose destination category is
    outside 1 .. n_cat is skipped and ORs SBADVALUE."""
    seq = np.asarray(seq)
    if seq.ndim != 2 or seq.shape[1] != 3:
        raise ValueError(f"slot_hist_host: seq must be [M, 3] rows of (poi, slot, category), got shape {seq.shape}")
    offsets, train = np.asarray(offsets, dtype=np.int64).reshape(-1), np.asarray(train).reshape(-1) != 0
    S, C, M = int(n_slots), int(n_cat), seq.shape[0]
    if offsets.size != train.size + 1 or S < 1 or C < 1:
        raise ValueError(f"slot_hist_host: {offsets.size} offsets for {train.size} sessions, n_slots = {S}, n_cat = {C}")
    o0, o1 = offsets[:-1], offsets[1:]
    ok = (o0 >= 0) & (o1 >= o0) & (o1 <= M)
    pairs = np.where(ok & train, np.maximum(o1 - o0 - 1, 0), 0)
    k = np.repeat(o0 + 1 - (np.cumsum(pairs) - pairs), pairs) + np.arange(int(pairs.sum()), dtype=np.int64)   # the second rows, session by session
    slot, b = seq[k - 1, 1].astype(np.int64), seq[k, 2].astype(np.int64)
    good = (slot >= 0) & (slot < S) & (b >= 1) & (b <= C)
    st = np.bincount(slot[good] * C + b[good] - 1, minlength=S * C).astype(np.int64).reshape(S, C)
    if status is not None:
        status[0] |= (0 if ok.all() else SBADINDEX) | (0 if good.all() else SBADVALUE)
    return st


def tables_from_counts(graph_cat, slot_cat):
    """-> (Tc f32 [C, C], Tt f32 [S, C]) of the module's docstring, evaluated in float64 and rounded once."""
    gc, st = np.asarray(graph_cat), np.asarray(slot_cat)
    if gc.ndim != 2 or gc.shape[0] != gc.shape[1] or gc.shape[0] < 1 or st.ndim != 2 or st.shape[0] < 1 or st.shape[1] != gc.shape[0] \
            or gc.dtype.kind not in "iu" or st.dtype.kind not in "iu":
        raise ValueError(f"tables_from_counts: integer counts [C, C] and [S, C], got {gc.dtype} {gc.shape} and {st.dtype} {st.shape}")
    if (gc < 0).any() or (st < 0).any():
        raise ValueError("tables_from_counts: a count is negative")
    C = gc.shape[0]
    gc, st = gc.astype(np.int64), st.astype(np.int64)
    m = gc.sum(axis=0)
    base = np.log((m.astype(np.float64) + 1.0) / (float(int(m.sum())) + C))

    def lift(counts):
        rows = counts.sum(axis=1).astype(np.float64)
        return (np.log((counts.astype(np.float64) + 1.0) / (rows[:, None] + C)) - base[None, :]).astype(np.float32)
    return lift(gc), lift(st)


def blend_host(scores, hist, time, cat, tables, weights, label_offset):
    """The blend of the module's docstring -> f32 numpy [G, V].  scores [G, V] f32; hist, time, cat [G, n] integers (or [G, n, 1]);
    tables a ContextTables; weights (w_category, w_time)."""
    t = tables
    s = np.array(scores, dtype=np.float32)
    G, V = s.shape
    hist, time, cat = (np.asarray(v).reshape(G, -1) for v in (hist, time, cat))
    if not hist.shape == time.shape == cat.shape:
        raise ValueError(f"blend_host: hist {hist.shape}, time {time.shape} and cat {cat.shape} must hold one entry per position")
    wc, wt = (np.float32(w) for w in np.asarray(weights, dtype=np.float64).reshape(-1))
    Tc, Tt = np.asarray(t.cat_table, dtype=np.float32), np.asarray(t.slot_table, dtype=np.float32)
    P, C, S, lo = int(t.P), int(t.n_cat), int(t.n_slots), int(label_offset)
    c_lo, c_hi = max(0, 1 - lo), min(V, P + 1 - lo)                    # the columns whose POI is one of 1 .. P
    if c_hi <= c_lo:
        return s
    k = np.asarray(t.poi_cat)[c_lo + lo - 1:c_hi + lo - 1].astype(np.int64)
    known = (k >= 1) & (k <= C)
    k = k[known] - 1
    for g in range(G):
        at = np.nonzero(hist[g] != 0)[0]
        if not len(at) or not 1 <= int(hist[g, at[-1]]) <= P:
            continue
        ca, ta = int(cat[g, at[-1]]), int(time[g, at[-1]])
        v = s[g, c_lo:c_hi][known]
        if 1 <= ca <= C:                                                # a product rounded to f32, then a sum rounded to f32
            v = (v + (wc * Tc[ca - 1, k]).astype(np.float32)).astype(np.float32)
        if 0 <= ta < S:
            v = (v + (wt * Tt[ta, k]).astype(np.float32)).astype(np.float32)
        s[g, c_lo:c_hi][known] = v
    return s


def _rows_of(rows, G, what):
    """rows of blend -> (hist, time, cat), each [G, n] int32 / int64 with unit column stride, time and cat of one dtype and one
    row stride (a batch or any object with .x, .time, .cat, or a (hist, time, cat) triple)"""
    if isinstance(rows, (tuple, list)):
        if len(rows) != 3:
            raise ValueError(f"{what}: rows must be a batch (.x, .time, .cat) or a (hist, time, cat) triple, got {len(rows)} entries "
                             "(a (hist, user) pair carries no slots or categories)")
        hist, time, cat = rows
    else:
        missing = [a for a in ("x", "time", "cat") if not hasattr(rows, a)]
        if missing:
            raise TypeError(f"{what}: rows must be a batch (.x, .time, .cat) or a (hist, time, cat) triple; {type(rows).__name__} has no "
                            f".{', .'.join(missing)}")
        hist, time, cat = rows.x, rows.time, rows.cat
    hist, time, cat = (v.reshape(v.shape[0], -1) for v in (hist, time, cat))
    if hist.shape[0] != G or time.shape != hist.shape or cat.shape != hist.shape:
        raise ValueError(f"{what}: {G} rows of scores; hist {tuple(hist.shape)}, time {tuple(time.shape)}, cat {tuple(cat.shape)}")
    for name, v in (("hist", hist), ("time", time), ("cat", cat)):
        if v.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"{what}: {name} must be int32 or int64, got {v.dtype}")
    if time.dtype != cat.dtype:
        time, cat = time.long(), cat.long()
    n = hist.shape[1]
    if n and hist.stride(1) != 1:
        hist = hist.contiguous()
    if n and (time.stride(1) != 1 or cat.stride(1) != 1 or max(time.stride(0), n) != max(cat.stride(0), n)):
        time, cat = time.contiguous(), cat.contiguous()
    return hist, time, cat


class ContextPrior(Prior):
    """The fitted tables of the module's docstring on one device, their weights (category, time) and a status word (prior.Prior).

    P, n_cat, n_slots      the POIs and the categories, as the UniverseCounts'; the time slots
    graph_cat              gc, numpy int64 [n_cat, n_cat] (the UniverseCounts' own counts)
    slot_cat               st, numpy int64 [n_slots, n_cat]
    poi_cat                int32 [P] on the device (the UniverseCounts' own tensor: shared, not copied)
    cat_table, slot_table  Tc f32 [n_cat, n_cat], Tt f32 [n_slots, n_cat] on the device
    status                 the fit's slot_hist ORs SBADINDEX / SBADVALUE into it; the blend flags nothing

    rows of blend: a collated batch or any object with .x, .time, .cat (hist = batch.x, the raw slots batch.time, the categories
    batch.cat), or a (hist, time, cat) triple of [G, n] (or [G, n, 1]) int32 / int64 tensors.  A (hist, user) pair as
    MarkovPrior.blend takes it is refused: it carries neither; a stack that holds both priors is given a batch.  The launch is
    mobgt_ctxprior_blend_rows."""

    NAME, WEIGHTS, LIB = "ContextPrior", WEIGHTS, _ctxprior
    SKIPPED = ("sessions or pairs", "an offsets pair was descending or beyond the check-ins, a slot was outside [0, n_slots) or a "
               "category outside 1 .. n_cat -- which the host checks should have refused")
    HINTS = ("fit the prior on the loop's device (ContextPrior.fit(..., device=...))", "the counts were not taken over the model's universe")

    def __init__(self, poi_cat, graph_cat, slot_cat, cat_table, slot_table, category=1.0, time=1.0, status=None):
        self.poi_cat, self.P = poi_cat, int(poi_cat.numel())
        self.graph_cat, self.slot_cat = graph_cat, slot_cat
        self.n_slots, self.n_cat = (int(v) for v in slot_cat.shape)
        self._host_cat_table = np.ascontiguousarray(cat_table, dtype=np.float32)
        self._host_slot_table = np.ascontiguousarray(slot_table, dtype=np.float32)
        self.cat_table = torch.from_numpy(self._host_cat_table.copy()).to(self.device)
        self.slot_table = torch.from_numpy(self._host_slot_table.copy()).to(self.device)
        super().__init__([category, time], status)

    @property
    def device(self):
        return self.poi_cat.device

    @classmethod
    def fit(cls, ds, train, counts=None, n_slots=None, category=1.0, time=1.0, device="cuda"):
        """Count st, take gc and poi_cat from `counts`, make the tables.

        ds: a data.SessionDataset of EVERY session (or anything the universe's counts take; a PrefixDataset is refused: it holds
        every transition once per prefix); train: a boolean mask over the sessions or the indices of the train sessions.
        counts: the UniverseCounts of the same ds and train on `device` (None: data.universe_counts(ds, train, device=device),
        universe_counts_host for a CPU device); its graph_cat, poi_cat, P and n_cat are the prior's.  n_slots: default the
        largest slot of ds.seq[:, 1] plus 1.  A negative slot, a slot >= n_slots, or sizes beyond MAX_SLOTS / MAX_CAT are a
        ValueError on the host before any launch.

        On a GPU: one launch sequence (mobgt_ctxprior_slot_hist) over the packed check-ins, one read-back of the counts and the
        status word, the tables in numpy, one upload.  A CPU device is counted by slot_hist_host.  A status that is not zero is a
        ValueError before the tables are made."""
        from . import universe
        what = "ContextPrior.fit"
        weights = check_weights([category, time], what, WEIGHTS)
        ds = universe._dataset(ds)
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if counts is None:
            counts = universe.universe_counts(ds, train, device=device) if device.type == "cuda" else universe.universe_counts_host(ds, train)
        if not isinstance(counts, universe.UniverseCounts):
            raise TypeError(f"{what}: counts must be a data.UniverseCounts (data.universe_counts(ds, train)), got {type(counts).__name__}")
        if counts.poi_cat.device != device:
            raise ValueError(f"{what}: the counts are on {counts.poi_cat.device}, the prior is fitted on {device}: count and fit on one "
                             "device (data.universe_counts(ds, train, device=...))")
        seq, offsets, mask, P, C = universe._prepare(ds, train, counts.P, counts.n_cat)
        M, n_sessions = int(seq.shape[0]), len(offsets) - 1
        slots = seq[:, 1]
        top = int(slots.max()) if M else 0
        S = top + 1 if n_slots is None else int(n_slots)
        bad = (slots < 0) | (slots >= S)
        if bad.any():
            s, i = universe._first_session(offsets, bad)
            raise ValueError(f"session {s}: time slot {int(slots[i])} at check-in {i - int(offsets[s])} is not in 0 .. {S - 1}"
                             + ("" if n_slots is None else f" (n_slots = {S})"))
        if not 1 <= S <= MAX_SLOTS or C > MAX_CAT:
            raise ValueError(f"{what}: n_slots = {S} / n_cat = {C} outside the kernels' limits (1 .. {MAX_SLOTS}, 1 .. {MAX_CAT})")
        gc = counts.graph_cat.detach().cpu().numpy().astype(np.int64)
        if gc.shape != (C, C) or counts.poi_cat.dtype != torch.int32 or tuple(counts.poi_cat.shape) != (P,):
            raise ValueError(f"{what}: the counts must hold graph_cat [{C}, {C}] and poi_cat int32 [{P}], got {gc.shape} and "
                             f"{counts.poi_cat.dtype} {tuple(counts.poi_cat.shape)}")
        if device.type != "cuda":
            status = [0]
            st = slot_hist_host(seq, offsets, mask, S, C, status=status)
            word = torch.tensor(status, dtype=torch.int32)
        else:
            from .ops import _p, _stream
            with torch.cuda.device(device):
                up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
                d_seq, d_offsets, d_train = up(seq), up(offsets), up(mask.astype(np.uint8))
                cells = torch.empty(S, C, dtype=torch.int64, device=device)
                word = torch.zeros(1, dtype=torch.int32, device=device)
                _ctxprior.launch("mobgt_ctxprior_slot_hist", _p(d_seq), M, _p(d_offsets), n_sessions, _p(d_train), S, C, _p(cells),
                                 _p(word), _stream())
                st = cells.cpu().numpy()
        cls.refuse(int(word[0]), what)                                   # (before the tables: counts with skipped pairs mean nothing)
        if int(st.sum()) != int(gc.sum()):
            raise RuntimeError(f"{what}: the slot histogram holds {int(st.sum())} pairs, graph_cat {int(gc.sum())}: the counts are not "
                               "those of this ds and train")
        Tc, Tt = tables_from_counts(gc, st)
        return cls(counts.poi_cat.contiguous(), gc, st, Tc, Tt, float(weights[0]), float(weights[1]), status=word)

    def tables(self):
        """-> ContextTables: poi_cat and the two tables as numpy arrays (one download, kept), what blend_host takes."""
        if self._host_tables is None:
            self._host_tables = ContextTables(self.poi_cat.detach().cpu().numpy(), self._host_cat_table, self._host_slot_table, self.P,
                                              self.n_cat, self.n_slots)
        return self._host_tables

    def lift(self, kind):
        """-> (counts int64, table f32) of kind "category" ([n_cat, n_cat]: row a - 1 the category left, column b - 1 the
        category entered) or "time" ([n_slots, n_cat]: row s the slot left), for inspection: table[r, b] > 0 where category b + 1
        follows row r more often than its marginal."""
        if kind not in WEIGHTS:
            raise ValueError(f"ContextPrior.lift: kind must be one of {', '.join(WEIGHTS)}, got {kind!r}")
        return (self.graph_cat, self._host_cat_table) if kind == "category" else (self.slot_cat, self._host_slot_table)

    _rows = staticmethod(lambda rows, G, what: tuple(zip(("hist", "time", "cat"), _rows_of(rows, G, what))))

    def _blend_host(self, scores, ids, w, label_offset):
        return blend_host(scores, *ids, self.tables(), w, label_offset)

    def _launch(self, head, ids, w, _p, code, stream):
        _, time, cat = ids
        _ctxprior.launch("mobgt_ctxprior_blend_rows", *head, _p(time), _p(cat), code(time), max(time.stride(0), time.shape[1]),
                         _p(self.poi_cat), self.P, _p(self.cat_table), _p(self.slot_table), self.n_cat, self.n_slots, _p(w), stream)
