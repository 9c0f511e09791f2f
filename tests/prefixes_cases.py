"""Inputs of the prefix-dataset tests (test_host_prefixes.py, test_gpu_prefixes.py): crafted packed sessions at the history lengths
where the kernels of csrc_prefixes/prefixes.hip change their path -- 64 rows are one wave's chunk, 4096 the longest history --
and golden G12's sessions.  A case is a data.SessionDataset built with from_packed.  `brute(name)` lists every prefix of a case by
brute force (data._as_record of the truncated session); `expected` cuts that list down to a min_history and a choice of sessions;
`host` is data.prefix_stats_host.  All are computed once, shared and never modified."""
import functools
import os

import numpy as np

from mobgt_amd import data

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INT32_MIN, INT32_MAX = np.iinfo(np.int32).min, np.iinfo(np.int32).max
MIN_HISTORIES = (1, 3, 64, 65)


def dataset(pois):
    """One session per entry of `pois` (the POI of every row, the target's included) -> SessionDataset, n and mult by np.unique."""
    rows, offsets, users, n, mult = [], [0], [], [], []
    for s, p in enumerate(pois):
        p = np.asarray(p, dtype=np.int64)
        assert len(p) >= 2
        rows.append(np.stack([p, np.arange(len(p)) % 48, np.abs(p) % 5 + 1], 1))
        offsets.append(offsets[-1] + len(p))
        users.append(s % 7)
        _, cnt = np.unique(p[:-1], return_counts=True)
        n.append(len(cnt))
        mult.append(int(cnt.max()))
    seq = np.concatenate(rows).astype(np.int32) if rows else np.zeros((0, 3), dtype=np.int32)
    return data.SessionDataset.from_packed(seq, np.asarray(offsets, dtype=np.int64), np.asarray(users, dtype=np.int64),
                                           np.asarray(n, dtype=np.int32), np.asarray(mult, dtype=np.int32))


def _drawn(rng, L, ids):
    """A session of L history rows and a target, POIs drawn from 1 .. ids."""
    return rng.randint(1, ids + 1, size=L + 1)


def _lengths():
    """Every history length at a chunk edge beside one on the other side of it: the four sessions of a workgroup of the short form
    are 1 | 64 | 2 | 129, 15 | 128 | 16 | 129, ...; the long form meets its sessions between short ones."""
    rng = np.random.RandomState(1)
    Ls = [1, 64, 2, 129, 15, 128, 16, 129, 63, 1, 64, 16, 65, 2, 127, 15, 128, 63, 129, 16, 65, 127]
    return dataset([_drawn(rng, L, 3 + L // 4) for L in Ls])


def _long_4096():
    """ONE session of 4096 history rows between short ones.  POI 9001 is at rows 63 and 64 only, POI 9002 at rows 0 and 4095 only:
    repeats that straddle the first chunk edge and the whole session."""
    rng = np.random.RandomState(2)
    p = _drawn(rng, 4096, 700)
    p[[63, 64]] = 9001
    p[[0, 4095]] = 9002
    return dataset([_drawn(rng, 9, 4), p, _drawn(rng, 16, 5), _drawn(rng, 70, 9)])


def _same_poi():
    return dataset([np.full(L + 1, 5) for L in (1, 5, 64, 65, 200)])                       # n = 1, mult = c


def _distinct():
    return dataset([np.arange(L + 1) * 3 + 1 for L in (1, 7, 64, 65, 130)])                # n = c, mult = 1


def _alternating():
    return dataset([np.arange(L + 1) % 2 + 10 for L in (2, 9, 64, 129)])


def _straddle():
    """Distinct POIs but for one repeat across a chunk edge: rows 63 and 64, and in another session rows 127 and 128."""
    a, b = np.arange(201) + 1, np.arange(140) + 1
    a[64] = a[63]
    b[128] = b[127]
    return dataset([a, np.arange(4) + 1, b])


def _extreme_ids():
    rng = np.random.RandomState(3)
    ids = np.array([INT32_MIN, -1, 0, INT32_MAX], dtype=np.int64)
    return dataset([ids[rng.randint(0, 4, size=L + 1)] for L in (10, 70, 3, 64)] + [ids, ids[::-1]])


def _many():
    """257 short sessions: the last workgroup of the short form is partly filled (64 whole workgroups and one wave)."""
    rng = np.random.RandomState(4)
    return dataset([_drawn(rng, int(L), 6) for L in rng.randint(1, 17, size=257)])


def g12():
    z = np.load(os.path.join(GOLDEN, "g12_sessions.npz"))
    o = z["offsets"]
    return data.SessionDataset([(int(z["users"][i]), z["checkins"][o[i]:o[i + 1]]) for i in range(len(z["users"]))])


CASES = {"lengths": _lengths, "long_4096": _long_4096, "same_poi": _same_poi, "distinct": _distinct, "alternating": _alternating,
         "straddle": _straddle, "extreme_ids": _extreme_ids, "many": _many, "empty": lambda: dataset([]),
         "one": lambda: dataset([[4, 4, 2, 4]]), "g12": g12}

# sessions= of the "lengths" case (22 sessions): a mask dropping the first session, the last, all; an index array, not in order
SELECTIONS = {"all_but_first": lambda S: np.arange(S) != 0, "all_but_last": lambda S: np.arange(S) != S - 1,
              "none": lambda S: np.zeros(S, dtype=bool), "indices": lambda S: np.array([12, 3, S - 1, 1, 7])}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def brute(name):
    """Every prefix of every session of a case (min_history 1): (session, cut, n, mult) int32, from data._as_record of the
    session cut after row k, for every k."""
    ds = case(name)
    out = []
    for s in range(len(ds)):
        user, c = ds[s].user, ds[s].checkins
        for k in range(1, len(c)):
            r = data._as_record((user, c[:k + 1]))
            out.append((s, k, r.n, r.mult))
    return tuple(np.asarray(col, dtype=np.int32) for col in (zip(*out) if out else ([], [], [], [])))


def expected(name, min_history=1, sessions=None):
    session, cut, n, mult = brute(name)
    take = cut >= min_history
    if sessions is not None:
        keep = np.zeros(len(case(name)), dtype=bool)
        keep[sessions] = True
        take &= keep[session]
    return data.PrefixStats(session[take], cut[take], n[take], mult[take])


@functools.lru_cache(maxsize=None)
def host(name, min_history=1):
    return data.prefix_stats_host(case(name), min_history)


def assert_same(a, b):
    """Two PrefixStats, array for array."""
    for f, x, y in zip(data.PrefixStats._fields, a, b):
        assert x.dtype == y.dtype == np.int32 and x.shape == y.shape and np.array_equal(x, y), f


def truncated(pds, ids=None):
    """The samples of a PrefixDataset as explicit sessions: (user, a COPY of rows 0 .. c of the base session) pairs."""
    ids = range(len(pds)) if ids is None else ids
    base = pds.base
    return [(base[int(pds.session[i])].user, base[int(pds.session[i])].checkins[:int(pds.cut[i]) + 1].copy()) for i in ids]
