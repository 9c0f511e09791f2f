"""Inputs of the universe-count tests (test_host_universe.py, test_gpu_universe.py): golden G13 and crafted packed sessions at
the sizes where a counting kernel can go wrong, each with the property that makes a wrong count visible.  A case is
(ds, train mask, P, n_cat): `ds` holds seq / offsets / users as data.SessionDataset does, built packed (a 100 000-check-in
session is one array, not a Python list).  `host(name)` is data.universe_counts_host of a case: computed once, shared, never
modified.  `loop_counts` is the rule as plain loops over sessions, for the cases small enough to loop over."""
import functools
import os
import types

import numpy as np

from mobgt_amd import _universe, data

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g13_universe.npz")
CHUNK, WAVE = _universe.CHUNK, 64
THRESHOLD = _universe.LDS_MAX_CAT


def packed(lengths, poi, cat, users=None):
    lengths = np.asarray(lengths, dtype=np.int64)
    poi = np.asarray(poi, dtype=np.int32)
    assert lengths.sum() == len(poi) == len(cat)
    seq = np.stack([poi, np.arange(len(poi), dtype=np.int32) % 48, np.asarray(cat, dtype=np.int32)], 1)
    return types.SimpleNamespace(seq=seq, offsets=np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64),
                                 users=np.zeros(len(lengths), dtype=np.int64) if users is None else np.asarray(users, dtype=np.int64))


@functools.lru_cache(maxsize=None)
def g13():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def g13_sessions():
    z = g13()
    return [(int(u), z["seq"][a:b].astype(np.int32)) for u, a, b in zip(z["users"], z["offsets"][:-1], z["offsets"][1:])]


def _g13():
    z = g13()
    return data.SessionDataset(g13_sessions()), z["train"], None, None


def _empty():
    return packed([], [], []), np.zeros(0, dtype=bool), None, None


def _two_checkins():
    return packed([2], [3, 5], [2, 1]), np.ones(1, dtype=bool), None, None


def _no_train():
    rng = np.random.RandomState(3)
    lengths = rng.randint(2, 7, size=40)
    poi = rng.randint(1, 21, size=lengths.sum())
    return packed(lengths, poi, (poi - 1) % 5 + 1), np.zeros(40, dtype=bool), None, None


def boundary_lengths():
    """2- and 3-check-in sessions over three chunks of the kernel: one session starts exactly at the first chunk edge, one lies
    across the second, and session ends fall on every lane of a wave."""
    rng = np.random.RandomState(5)
    first = rng.permutation([3] * 1364 + [2] * 2)                      # sums to CHUNK: a session starts at check-in CHUNK
    second = rng.permutation([3] * 1331 + [2] * 51)                    # sums to CHUNK - 1: the next session straddles 2 * CHUNK
    third = rng.choice([2, 3], size=1500)
    lengths = np.concatenate([first, second, [3], third])
    offsets = np.concatenate([[0], np.cumsum(lengths)])
    assert CHUNK == 4096 and CHUNK in offsets and 2 * CHUNK not in offsets and 2 * CHUNK - 1 in offsets
    assert offsets[-1] > 2 * CHUNK + 1000 and set(offsets % WAVE) == set(range(WAVE))
    return lengths


def _boundaries():
    """Inside a session the POIs ascend by one, so every transition inside a session is x -> x + 1; the first POI of the next
    session is never the last POI of this one plus one: a pair across a session boundary occurs nowhere inside a session, and
    one leaked transition puts a count where the truth has none.  Train and test sessions alternate."""
    lengths = boundary_lengths()
    rng = np.random.RandomState(6)
    P, poi, last = 40, [], -5
    for n in lengths:
        b = int(rng.randint(1, P - 2))
        if b == last + 1:
            b = b + 1 if b + 1 <= P - 3 else 1
        poi += list(range(b, b + n))
        last = b + n - 1
    poi = np.array(poi)
    ends = np.cumsum(lengths)[:-1]
    assert poi.max() <= P and (poi[ends] != poi[ends - 1] + 1).all()
    return packed(lengths, poi, (poi - 1) % 7 + 1), np.arange(len(lengths)) % 2 == 0, P, 7


def _one_poi_100k():
    """One train session of 100 000 check-ins at POI 2, category 1: a diagonal count of 99 999 does not fit 16 bits."""
    return packed([100000], np.full(100000, 2), np.ones(100000)), np.ones(1, dtype=bool), 3, 2


def _one_transition_70k():
    """The transition 5 -> 9 in 70 000 train sessions of two check-ins: one run of 70 000 equal keys."""
    poi = np.tile([5, 9], 70000)
    return packed(np.full(70000, 2), poi, np.tile([2, 1], 70000)), np.ones(70000, dtype=bool), 12, 3


def _categories(n_cat):
    """Random sessions over three chunks with every one of n_cat categories in use (POI p has category (p - 1) % n_cat + 1)."""
    rng = np.random.RandomState(100 + n_cat)
    P = max(2 * n_cat, 50)
    lengths = rng.randint(2, 10, size=1600)
    poi = rng.randint(1, P + 1, size=lengths.sum())
    poi[:P] = np.arange(1, P + 1)
    assert lengths.sum() > 2 * CHUNK
    return packed(lengths, poi, (poi - 1) % n_cat + 1), rng.rand(1600) < 0.7, P, n_cat


def _key_width():
    """P = 100 000, transitions among POIs 99 990 .. 100 000 and POI 1: keys up to 10^10 - 1, which 32 bits cannot hold."""
    rng = np.random.RandomState(9)
    pool = np.array([1] + list(range(99990, 100001)))
    lengths = rng.randint(2, 8, size=90)
    poi = pool[rng.randint(0, len(pool), size=lengths.sum())]
    keys = (poi[:-1].astype(np.int64) - 1) * 100000 + poi[1:] - 1
    assert keys.max() >= 2 ** 32 and keys.min() < 2 ** 31                # (a truncated key names another pair)
    return packed(lengths, poi, poi % 3 + 1), rng.rand(90) < 0.8, 100000, 3


def _one_poi_universe():
    lengths = [2, 5, 3, 2, 9]
    return packed(lengths, np.ones(sum(lengths)), np.ones(sum(lengths))), np.array([True, False, True, True, False]), 1, 1


CASES = {
    "g13": _g13, "empty": _empty, "two_checkins": _two_checkins, "no_train": _no_train, "boundaries": _boundaries,
    "one_poi_100k": _one_poi_100k, "one_transition_70k": _one_transition_70k, "n_cat_1": lambda: _categories(1),
    "n_cat_threshold": lambda: _categories(THRESHOLD), "n_cat_threshold_plus_1": lambda: _categories(THRESHOLD + 1),
    "n_cat_600": lambda: _categories(600), "n_cat_max": lambda: _categories(_universe.MAX_CAT), "key_width": _key_width, "P_1": _one_poi_universe,
}
LOOPED = ("g13", "empty", "two_checkins", "no_train", "boundaries", "n_cat_1", "n_cat_threshold_plus_1", "key_width", "P_1")


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def host(name):
    ds, train, P, n_cat = case(name)
    return data.universe_counts_host(ds, train, P=P, n_cat=n_cat)


def loop_counts(ds, train, P, n_cat):
    """The rule of the issue's table as loops over sessions and check-ins -> (checkin_cnt, cat_cnt, graph_cat, {(p, q): count})."""
    checkin_cnt, cat_cnt = np.zeros(P, dtype=np.int64), np.zeros(n_cat, dtype=np.int64)
    graph_cat, adj = np.zeros((n_cat, n_cat), dtype=np.int64), {}
    for s in range(len(ds.offsets) - 1):
        rows = ds.seq[ds.offsets[s]:ds.offsets[s + 1]]
        for k, (p, _, c) in enumerate(rows):
            checkin_cnt[p - 1] += 1
            cat_cnt[c - 1] += 1
            if k > 0 and train[s]:
                graph_cat[rows[k - 1][2] - 1, c - 1] += 1
                adj[int(rows[k - 1][0]), int(p)] = adj.get((int(rows[k - 1][0]), int(p)), 0) + 1
    return checkin_cnt, cat_cnt, graph_cat, adj


def csr_dict(graph):
    """TransitionGraph -> {(p, q): count}, after the shape checks every CSR must pass."""
    rowptr, col, val = graph.rowptr.cpu().numpy(), graph.col.cpu().numpy(), graph.val.cpu().numpy()
    assert rowptr.dtype == np.int64 and col.dtype == np.int32 and val.dtype == np.int32
    assert rowptr.shape == (graph.P + 1,) and rowptr[0] == 0 and rowptr[-1] == len(col) == len(val) and (np.diff(rowptr) >= 0).all()
    rows = np.repeat(np.arange(graph.P), np.diff(rowptr))
    same_row = rows[1:] == rows[:-1]
    assert (np.diff(col)[same_row] > 0).all()                          # strictly ascending inside every row
    assert len(col) == 0 or (col.min() >= 0 and col.max() < graph.P and val.min() >= 1)
    return {(int(r) + 1, int(c) + 1): int(v) for r, c, v in zip(rows, col, val)}
