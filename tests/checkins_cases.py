"""Inputs of the check-in log tests (test_host_checkins.py, test_gpu_checkins.py): golden G14 (both copies) and crafted logs at the
sizes and thresholds where the cut can go wrong.  A case is (columns dict: user, poi, cat, t and perhaps lat / lon; parameters
dict).  `host(name)` is data.sessionize_host of a case: computed once, shared, never modified."""
import functools
import os

import numpy as np

from mobgt_amd import data

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g14_checkins.npz")
WAVE = 64
SMALL = dict(trace_min=1, global_visit=1, session_min=2, sessions_min=1, train_split=1.0)       # (nothing filtered unless the case says so)
FIELDS = ("seq", "offsets", "users", "n", "mult")


@functools.lru_cache(maxsize=None)
def g14():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def g14_log(copy):
    z = g14()
    order = np.arange(len(z["t"])) if copy == "sorted" else z["perm"]
    return {k: z[k][order] for k in ("user", "poi", "cat", "t", "lat", "lon")}


class Log:
    """A log under construction: user(name, times, pois=...) appends a user's records in log order."""

    def __init__(self):
        self.rows = []

    def user(self, name, times, pois=None, cats=None):
        times = np.asarray(times, dtype=np.int64)
        pois = np.arange(len(times)) % 7 + 1 if pois is None else np.broadcast_to(pois, times.shape)
        cats = np.asarray(pois) % 3 + 1 if cats is None else np.broadcast_to(cats, times.shape)
        self.rows += [(name, int(p), int(c), int(t)) for p, c, t in zip(pois, cats, times)]
        return self

    def columns(self, interleave=None):
        rows = self.rows
        if interleave is not None:                                     # a stable mix of the users: each keeps its own order
            key = np.random.RandomState(interleave).rand(len(rows))
            names = [r[0] for r in rows]
            slots = {n: sorted(key[[i for i, m in enumerate(names) if m == n]]) for n in set(names)}
            seen = {n: 0 for n in slots}
            keyed = []
            for r in rows:
                keyed.append((slots[r[0]][seen[r[0]]], r))
                seen[r[0]] += 1
            rows = [r for _, r in sorted(keyed, key=lambda kr: kr[0])]
        return dict(user=np.array([r[0] for r in rows]), poi=np.array([r[1] for r in rows], dtype=np.int64),
                    cat=np.array([r[2] for r in rows], dtype=np.int64), t=np.array([r[3] for r in rows], dtype=np.int64))


def steps(n, step=900, t0=1_000_000):
    return t0 + step * np.arange(n)


def _chunk_edges():
    """Users with 0, 1, 63, 64, 65, 128 and 129 remaining records (plus a filtered record at the front, in the middle and at the
    end of each): the chunk edges of the wave, the carried t and the carried session length."""
    log = Log()
    for k, n in enumerate([0, 1, 63, 64, 65, 128, 129]):
        t = 2_000_000 * (k + 1) + np.cumsum(np.random.RandomState(k).choice([700, 900, 300, 90000], size=n + 3, p=[0.5, 0.3, 0.1, 0.1]))
        pois = np.arange(n + 3) % 5 + 1
        pois[[0, (n + 3) // 2, -1]] = 100 + k                          # three visits of a POI nobody else visits: filtered
        log.user(f"u{n}", t, pois)
    return log.columns(interleave=1), dict(SMALL, global_visit=4)


def _all_filtered():
    log = Log().user("a", steps(30)).user("gone", steps(12), pois=np.arange(12) + 50).user("b", steps(20, 1000))
    return log.columns(interleave=2), dict(SMALL, global_visit=2)


def _session_max(m):
    def case():
        rng = np.random.RandomState(m)
        log = Log()
        for k in range(6):
            log.user(f"u{k}", 10_000_000 * k + np.cumsum(rng.choice([700, 60, 90000], size=90 + 17 * k, p=[0.8, 0.15, 0.05])))
        return log.columns(interleave=3), dict(SMALL, session_max=m, session_min=2)
    return case


def _under_min_gap_after_full():
    """11 records fill a session; 40 more follow at 60 s steps: each would be dropped, but the session is full at the first, which
    starts a session of one; nothing appends to it, so every 60 s record after it is dropped, until seven records at 900 s steps
    append to it (the first of them 900 s after the last dropped one).  With session_max = 1 a session is full at 2."""
    t = np.concatenate([steps(11), steps(11)[-1] + 60 * np.arange(1, 41), steps(11)[-1] + 2400 + 900 * np.arange(1, 8)])
    return Log().user("a", t).user("b", t + 5).columns(interleave=4), dict(SMALL)


def _under_min_gap_session_max_1():
    cols, p = _under_min_gap_after_full()
    return cols, dict(p, session_max=1)


def _thresholds():
    log = Log()
    for k, g in enumerate([86400, 86399, 86401, 600, 599, 601]):
        log.user(f"g{g}", np.concatenate([steps(4), steps(4)[-1] + g + 900 * np.arange(5)]))
    return log.columns(interleave=5), dict(SMALL)


def _shuffled():
    rng = np.random.RandomState(6)
    log = Log()
    for k in range(5):
        log.user(f"u{k}", rng.permutation(1_000_000 + np.cumsum(rng.choice([700, 900, 90000], size=150, p=[0.6, 0.3, 0.1])))
                 if k % 2 else 1_000_000 + np.cumsum(rng.choice([700, -700, 90000], size=150, p=[0.6, 0.3, 0.1])))
    return log.columns(interleave=6), dict(SMALL)


def _trace_and_visit_edges():
    """Users with trace_min - 1 and trace_min records, POIs with global_visit - 1 and global_visit visits."""
    log = Log()
    log.user("nine", steps(9), pois=1).user("ten", steps(10), pois=1)
    log.user("big", steps(40), pois=np.r_[np.full(9, 2), np.full(10, 3), np.full(21, 1)])           # POI 2: 9 visits, POI 3: 10
    return log.columns(interleave=7), dict(trace_min=10, global_visit=10, session_min=2, sessions_min=1, train_split=1.0)


def _ties():
    log = Log()
    for name, n in (("c", 20), ("a", 30), ("d", 20), ("b", 30), ("e", 20), ("f", 31)):
        log.user(name, steps(n))
    return log.columns(interleave=8), dict(SMALL)


def _split_counts():
    """2, 3, 5, 10 and 15 sessions per user: floor(0.8 n) = 1, 2, 4, 8, 12 in float64 (0.8 * 5 and 0.8 * 10 and 0.8 * 15 are not
    exact products)."""
    log = Log()
    for n in (2, 3, 5, 10, 15):
        log.user(f"s{n}", np.concatenate([100_000 * s + steps(3 + s % 2) for s in range(n)]))
    return log.columns(interleave=9), dict(SMALL, train_split=0.8)


def _multi_category():
    log = Log().user("a", steps(12), pois=np.arange(12) % 3 + 1, cats=np.arange(12) % 4 + 1)
    log.user("b", steps(12, 1000), pois=np.arange(12) % 4 + 1, cats=7 - np.arange(12) % 5)
    return log.columns(interleave=10), dict(SMALL)


def _empty_result():
    return Log().user("a", steps(8)).user("b", steps(6)).columns(), dict(DEFAULTS_ONLY)


def _no_records():
    z = np.zeros(0, dtype=np.int64)
    return dict(user=z, poi=z, cat=z, t=z), {}


DEFAULTS_ONLY = {}
CASES = {"chunk_edges": _chunk_edges, "all_filtered": _all_filtered, "session_max_1": _session_max(1), "session_max_10": _session_max(10),
         "session_max_15": _session_max(15), "under_min_gap_after_full": _under_min_gap_after_full,
         "under_min_gap_session_max_1": _under_min_gap_session_max_1, "thresholds": _thresholds, "shuffled": _shuffled,
         "trace_and_visit_edges": _trace_and_visit_edges, "ties": _ties, "split_counts": _split_counts, "multi_category": _multi_category,
         "empty_result": _empty_result, "no_records": _no_records,
         "g14_sorted": lambda: (g14_log("sorted"), {}), "g14_shuffled": lambda: (g14_log("shuffled"), {})}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def host(name):
    cols, params = case(name)
    return data.sessionize_host(**cols, **params)


def assert_same(a, b):
    """Two Sessionized, field for field."""
    for f in FIELDS:
        x, y = getattr(a.dataset, f), getattr(b.dataset, f)
        assert x.dtype == y.dtype and np.array_equal(x, y), f
    for f in ("train", "user_ids", "poi_ids", "cat_ids", "kept", "users_order"):
        x, y = getattr(a, f), getattr(b, f)
        assert x.dtype == y.dtype and np.array_equal(x, y), f
    assert (a.coords_deg is None) == (b.coords_deg is None)
    if a.coords_deg is not None:
        assert a.coords_deg.dtype == b.coords_deg.dtype and np.array_equal(a.coords_deg, b.coords_deg)


def sessions_of(res):
    """{raw user id: [session lengths]} of a result."""
    out = {}
    for u, n in zip(res.user_ids[res.dataset.users], np.diff(res.dataset.offsets)):
        out.setdefault(str(u), []).append(int(n))
    return out
