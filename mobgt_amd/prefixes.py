"""Every prefix of a check-in session as a sample.

The reference makes ONE sample of a session: all check-ins but the last are the history, the last is the target
(gen_pickles.py:760-761).  Its own Markov baseline scores every step of every session (graphormer/train.py:436-446), and so does
most next-POI work.  `PrefixDataset` is that protocol over a data.SessionDataset, without materialising a prefix.

The rule.  A session has rows r_0 .. r_L, L >= 1.  For min_history = h >= 1 it yields the samples c = h .. L: sample c has
history r_0 .. r_{c-1} and target r_c.  c = L is the session's own sample (the prefix dataset contains the base dataset); a
session with L < h yields nothing.  Samples are ordered session-major in base order, c ascending inside a session.  Per sample

    n_c    = the distinct POIs among r_0 .. r_{c-1}      (shape buckets, max_node, the length-balanced dealing)
    mult_c = how often the most visited POI occurs there (the bound on edge counts in SessionCollator.limit_violation)

With occ_j = the number of i <= j with poi_i == poi_j these are n_c = #{j < c: occ_j == 1} and mult_c = max_{j < c} occ_j: an
inclusive sum-scan and an inclusive max-scan along the session, exact integers.

`prefix_stats` runs it on the device (csrc_prefixes/prefixes.hip through _prefixes); `prefix_stats_host` is the same rule as a
plain loop: the CPU form and the kernel's reference."""
import collections

import numpy as np
import torch

from . import _prefixes

PrefixStats = collections.namedtuple("PrefixStats", "session cut n mult")
PrefixStats.__doc__ = """The Q samples of a prefix dataset, numpy int32 [Q] each: the base session of sample q, its cut c (rows 0 .. c
of the session, row c the target), n and mult of its history."""

DEVICE_MAX_L = _prefixes.MAX_L                     # (the header's: the POI column of a session in 16 KB of LDS)


# ---- what both forms check on the host ----------------------------------------------------------------------------------------------
def _prepare(ds, min_history, sessions, what):
    """-> (min_history as an int, keep: bool [S] or None for every session), every TypeError / ValueError raised."""
    from .data import SessionDataset
    if not isinstance(ds, SessionDataset):
        hint = ": give its .base" if isinstance(ds, PrefixDataset) else " (data.SessionDataset(sessions) validates and packs them)"
        raise TypeError(f"{what}: the base must be a data.SessionDataset, got {type(ds).__name__}{hint}")
    if not isinstance(min_history, (int, np.integer)) or isinstance(min_history, bool) or min_history < 1:
        raise ValueError(f"{what}: min_history must be an integer >= 1 (a sample needs a history), got {min_history!r}")
    S = len(ds)
    if sessions is None:
        return int(min_history), None
    t = np.asarray(sessions)
    if t.dtype == np.bool_:
        if t.shape != (S,):
            raise ValueError(f"{what}: sessions is a mask of {t.shape[0] if t.ndim == 1 else t.shape} flags for {S} sessions")
        return int(min_history), np.ascontiguousarray(t)
    if t.size and not np.issubdtype(t.dtype, np.integer):
        raise ValueError(f"{what}: sessions is a boolean mask of length {S} or integer session indices, got {t.dtype}")
    t = t.reshape(-1).astype(np.int64)
    if t.size and (t.min() < 0 or t.max() >= S):
        raise ValueError(f"{what}: session index {int(t[(t < 0) | (t >= S)][0])} is not in 0 .. {S - 1}")
    keep = np.zeros(S, dtype=bool)
    keep[t] = True
    if int(keep.sum()) != t.size:
        twice = np.sort(t)
        raise ValueError(f"{what}: session index {int(twice[1:][twice[1:] == twice[:-1]][0])} is given more than once")
    return int(min_history), keep


def _counts(offsets, keep, h):
    """The sample count of every session: L - h + 1 where it is kept and L >= h, else 0 (numpy int64 [S])."""
    L = np.diff(offsets) - 1
    cnt = np.maximum(L - h + 1, 0)
    return cnt if keep is None else np.where(keep, cnt, 0)


# ---- the host form ------------------------------------------------------------------------------------------------------------------
def prefix_stats_host(ds, min_history=1, sessions=None):
    """The rule of the module's docstring as a plain loop over the check-ins -> PrefixStats.  `ds`: a data.SessionDataset;
    `sessions`: a bool mask [S] or an integer index array of the base sessions that yield samples (None: all of them)."""
    h, keep = _prepare(ds, min_history, sessions, "prefix_stats_host")
    poi, offsets = ds.seq[:, 0].tolist(), ds.offsets.tolist()
    session, cut, n, mult = [], [], [], []
    for s in range(len(ds)):
        if keep is not None and not keep[s]:
            continue
        a, L = offsets[s], offsets[s + 1] - offsets[s] - 1
        seen, most = {}, 0
        for c in range(1, L + 1):                                      # the history r_0 .. r_{c-1}: one row more than before
            p = poi[a + c - 1]
            seen[p] = seen.get(p, 0) + 1
            most = max(most, seen[p])
            if c >= h:
                session.append(s)
                cut.append(c)
                n.append(len(seen))
                mult.append(most)
    return PrefixStats(*(np.asarray(v, dtype=np.int32) for v in (session, cut, n, mult)))


# ---- the device path ----------------------------------------------------------------------------------------------------------------
def _launch(d_seq, d_offsets, d_pcum, d_keep, S, M, Q, h, out):
    """The one launch: `out` is int32 [4 Q + 1] on the device -- session, cut, n, mult and the status word."""
    from .ops import _p, _stream
    part = lambda k: out.data_ptr() + 4 * k * Q
    _prefixes.launch("mobgt_prefixes_stats", _p(d_seq), _p(d_offsets), _p(d_pcum), _p(d_keep), S, M, Q, h, part(0), part(1), part(2),
                     part(3), part(4), _stream())


def _first_bad_session(offsets, pcum, keep, h, M, Q):
    """The first session the kernel refuses, by the kernel's own checks on what it was given (numpy copies of the device arrays)."""
    a, b, p0, p1 = offsets[:-1], offsets[1:], pcum[:-1], pcum[1:]
    cnt = _counts(offsets, keep, h)
    bad = (a < 0) | (b < a) | (b > M) | (p0 < 0) | (p1 < p0) | (p1 > Q) | (p1 - p0 != cnt) | ((cnt > 0) & (b - a - 1 > DEVICE_MAX_L))
    return int(np.argmax(bad)) if bad.any() else -1


def prefix_stats(ds, min_history=1, sessions=None, device="cuda"):
    """prefix_stats_host on the device -> the same PrefixStats, integer for integer.  Everything about the arguments is validated
    on the host before anything is launched.  Behind the call: one upload of seq and offsets (and of the mask, if there is one),
    the sample count of every session and its cumulative sum in torch, one launch (mobgt_prefixes_stats: a fill, the short form
    for histories of at most 64 rows, the long form for the rest) and one read-back of the four arrays with the status word.  A
    status word that is not zero is a ValueError naming the first session the kernel skipped.

    Without a GPU (`device="cpu"`) this is prefix_stats_host.  A dataset that holds a history longer than 4096 rows
    (_prefixes.MAX_L, the collator's limit too) takes the host form for the WHOLE call."""
    device = torch.device(device)
    if device.type != "cuda":
        return prefix_stats_host(ds, min_history, sessions)
    h, keep = _prepare(ds, min_history, sessions, "prefix_stats")
    S, M = len(ds), int(ds.seq.shape[0])
    cnt = _counts(ds.offsets, keep, h)
    Q = int(cnt.sum())
    if M >= 2 ** 31:
        raise ValueError(f"prefix_stats: {M} check-ins, the kernel indexes them with 31 bits (M < 2**31): list the sessions in parts")
    if S and int((np.diff(ds.offsets) - 1)[cnt > 0].max(initial=0)) > DEVICE_MAX_L:
        return prefix_stats_host(ds, min_history, sessions)
    with torch.cuda.device(device):
        d_seq, d_offsets = torch.from_numpy(ds.seq).to(device), torch.from_numpy(ds.offsets).to(device)
        d_keep = None if keep is None else torch.from_numpy(keep.view(np.uint8)).to(device)
        d_cnt = (d_offsets[1:] - d_offsets[:-1] - h).clamp_(min=0)    # (L - h + 1 with L = rows - 1)
        if d_keep is not None:
            d_cnt *= d_keep
        d_pcum = torch.zeros(S + 1, dtype=torch.int64, device=device)
        torch.cumsum(d_cnt, 0, out=d_pcum[1:])
        out = torch.empty(4 * Q + 1, dtype=torch.int32, device=device)
        _launch(d_seq, d_offsets, d_pcum, d_keep, S, M, Q, h, out)
        host = out.cpu().numpy()
        bits = int(host[4 * Q])
        if bits:
            s = _first_bad_session(d_offsets.cpu().numpy(), d_pcum.cpu().numpy(), keep, h, M, Q)
            raise ValueError(f"prefix_stats: the kernel skipped sessions (status {bits}), the first of them session {s}: its offsets "
                             "or output positions were out of range when the kernel read them, which the host checks should have refused")
    return PrefixStats(*(host[k * Q:(k + 1) * Q] for k in range(4)))


# ---- the dataset --------------------------------------------------------------------------------------------------------------------
class PrefixDataset:
    """The prefixes of a data.SessionDataset as a dataset of their own, for SessionCollator and the loops: pds[i] is the
    SessionRecord of sample i -- user, the rows 0 .. c of its session (a VIEW of base.seq: nothing is copied, no prefix is
    materialised), n and mult of the history rows 0 .. c - 1.

    `ds` must be a SessionDataset.  `min_history`: the shortest history that makes a sample.  `sessions`: a bool mask [S] or an
    integer index array of the base sessions that yield samples -- `res.train` and `~res.train` of data.sessionize are the
    intended uses; the order of the samples is the base's whatever the order of the indices.  `device`: where prefix_stats runs.

    Attributes: base, min_history; session, cut, n, mult (int32 [Q]); users (int64 [Q]); last (bool [Q], derived on access: true
    where the cut is the session's own, the base dataset's sample -- `pds.last` selects the reference's protocol out of a per-step
    evaluation); max_n.  24 bytes per sample on top of the base; materialised prefixes would cost 12 (c + 1) bytes per sample."""

    def __init__(self, ds, min_history=1, sessions=None, device="cuda"):
        stats = prefix_stats(ds, min_history, sessions, device)
        self.base, self.min_history = ds, int(min_history)
        self.session, self.cut, self.n, self.mult = (np.ascontiguousarray(v, dtype=np.int32) for v in stats)
        self.users = np.ascontiguousarray(ds.users[self.session], dtype=np.int64)

    def __len__(self):
        return len(self.session)

    def __getitem__(self, i):
        from .data import SessionRecord
        i = int(i)
        if not -len(self) <= i < len(self):
            raise IndexError(i)
        i %= len(self)
        o = self.base.offsets[self.session[i]]
        return SessionRecord(int(self.users[i]), self.base.seq[o:o + int(self.cut[i]) + 1], int(self.n[i]), int(self.mult[i]))

    @property
    def last(self):
        return self.cut == (np.diff(self.base.offsets) - 1)[self.session]

    @property
    def max_n(self):
        """The longest trajectory graph of the dataset (nodes)."""
        return int(self.n.max()) if len(self) else 0
