"""Inputs of the Markov-baseline tests (test_host_baseline.py, test_gpu_baseline.py): crafted sessions, each case built to hit one
edge of the kernels of csrc_baseline/baseline.hip -- 64 entries of a row, 64 history rows and 64 entries of pop_order are one
wave's step, four samples are one workgroup.  A case is (ds, train, samples): a data.SessionDataset of every session, the train
mask, and the samples (a data.PrefixDataset over the other sessions, or a data.SessionDataset of its own).  `host(name, order)` and
`host_lists(name, order, k)` are baseline.ranks_host / topk_host: computed once, shared and never modified."""
import collections
import functools

import numpy as np

from mobgt_amd import baseline, data

ORDERS = ("user", "global", "popularity")
KS = (1, 20, 64)
Case = collections.namedtuple("Case", "ds train samples")


def dataset(sessions):
    """(user, the POI of every row, the target's included) pairs -> SessionDataset, n and mult by np.unique."""
    rows, offsets, users, n, mult = [], [0], [], [], []
    for u, p in sessions:
        p = np.asarray(p, dtype=np.int64)
        assert len(p) >= 2
        rows.append(np.stack([p, np.arange(len(p)) % 48, p % 5 + 1], 1))
        offsets.append(offsets[-1] + len(p))
        users.append(u)
        _, cnt = np.unique(p[:-1], return_counts=True)
        n.append(len(cnt))
        mult.append(int(cnt.max()))
    seq = np.concatenate(rows).astype(np.int32) if rows else np.zeros((0, 3), dtype=np.int32)
    return data.SessionDataset.from_packed(seq, np.asarray(offsets, dtype=np.int64), np.asarray(users, dtype=np.int64),
                                           np.asarray(n, dtype=np.int32), np.asarray(mult, dtype=np.int32))


def _case(train, test, prefixes=True):
    """Train and test sessions -> Case.  prefixes: the samples are every prefix of the test sessions (a PrefixDataset over the
    whole dataset); else the test sessions as a SessionDataset of their own, one sample each."""
    ds = dataset(train + test)
    mask = np.arange(len(ds)) < len(train)
    return Case(ds, mask, data.PrefixDataset(ds, sessions=~mask, device="cpu") if prefixes else dataset(test))


# ---- a miniature whose ranks are written out in test_host_baseline.py ---------------------------------------------------------------
MINI_TRAIN = [(0, [1, 2]), (0, [1, 2]), (0, [1, 3]), (1, [1, 3]), (1, [1, 3]), (1, [1, 4]), (1, [1, 5]), (0, [1, 4])]
MINI_P = 6
# cg(1, .) = {2: 2, 3: 3, 4: 2, 5: 1}; pop = {1: 8, 2: 2, 3: 3, 4: 2, 5: 1, 6: 0}: by popularity 1 3 2 4 5 6 (2 before 4: lower id)
# cu(0, 1, .) = {2: 2, 3: 1, 4: 1}; cu(1, 1, .) = {3: 2, 4: 1, 5: 1}
MINI_LISTS = {                                                          # (user, previous POI, order) -> every POI, best first
    (0, 1, "user"): [2, 3, 4, 5, 1, 6],                                 # 3 before 4: equal cu decided by cg
    (1, 1, "user"): [3, 4, 5, 2, 1, 6],
    (7, 1, "user"): [3, 2, 4, 5, 1, 6],                                 # a user absent from training backs off
    (0, 1, "global"): [3, 2, 4, 5, 1, 6],                               # 2 before 4: equal cg, equal pop, lower id
    (0, 2, "user"): [1, 3, 2, 4, 5, 6],                                 # an empty row: pure popularity
    (1, 1, "popularity"): [1, 3, 2, 4, 5, 6],
}


def mini_samples(user, prev):
    """The six samples (user, [prev, t]) for t = 1 .. 6."""
    return [(user, [prev, t]) for t in range(1, MINI_P + 1)]


def _mini():
    test = [s for (u, a) in ((0, 1), (1, 1), (7, 1), (0, 2)) for s in mini_samples(u, a)]
    return _case(MINI_TRAIN, test, prefixes=False)


# ---- rows of every length at which a kernel changes its path ------------------------------------------------------------------------
ROW_LENGTHS = (1, 63, 64, 65, 129, 200, 0, 2, 19, 20, 21)              # of hub POIs 1 .. 11
ROWS_P = 270


def _rows():
    """Hub POI h = 1 .. 11 is followed by ROW_LENGTHS[h - 1] distinct POIs drawn from 12 .. P, one two-row train session per
    transition and repeat (counts 1 .. 3, so equal cu, cg and pop abound), users 0 .. 4 in turn: POI 1's only transition is user
    0's, the first range of the user table; user 4's session (P, 12) is its last.  Hub 7 has an empty row.  The test sessions
    (x, h, t) put t at the first and at the last entry of the row, at a POI absent from it, and at the hub itself; their users
    are 0 .. 4 and 9, who is absent from training.  Every prefix is a sample."""
    rng = np.random.RandomState(11)
    train, test, i = [], [], 0
    for h, n in enumerate(ROW_LENGTHS, start=1):
        succ = np.sort(rng.choice(np.arange(12, ROWS_P + 1), size=n, replace=False))
        for b in succ:
            for _ in range(rng.randint(1, 4)):
                train.append((i % 5, [h, int(b)]))
                i += 1
        absent = int(np.setdiff1d(np.arange(12, ROWS_P + 1), succ)[rng.randint(0, ROWS_P - 11 - n)])
        targets = ([int(succ[0]), int(succ[-1]), int(succ[len(succ) // 2])] if n else []) + [absent, h]
        for j, t in enumerate(targets):
            test.append(((0, 1, 2, 3, 4, 9)[(h + j) % 6], [int(rng.randint(12, ROWS_P + 1)), h, t]))
    train.append((4, [ROWS_P, 12]))
    test += [(4, [5, ROWS_P, 12]), (4, [5, ROWS_P, 13]), (0, [7, 1, int(train[0][1][1])]), (3, [1, 1, 12])]
    return _case(train, test)


def _fill():
    """Row 40 holds 63 entries, POI 40 itself among them, and these are exactly the 63 most popular POIs: a list of 64 takes its
    last POI from position 63 of pop_order, after skipping every entry before it."""
    others = [p for p in range(1, 64) if p != 40]                      # 62 POIs beside 40
    train = [(0, [40, 40])] + [(p % 3, [40, p]) for p in others]
    test = [(0, [3, 40, 90]), (1, [40, 40, 2]), (5, [99, 40, 64])]
    return _case(train, test)


def _history():
    """Plain sessions as samples: history lengths 1, 64, 65 and 4096; the target's POI (80) is nowhere in the history, or only at
    row 63, or only at row 64."""
    rng = np.random.RandomState(12)
    train = [(int(u), rng.randint(1, 81, size=int(n)).tolist()) for u, n in zip(rng.randint(0, 4, 60), rng.randint(2, 9, 60))]
    test = []
    for L in (1, 64, 65, 4096):
        for at in (None, 63, 64):
            if at is not None and at >= L:
                continue
            p = rng.randint(1, 80, size=L + 1)
            p[L] = 80
            if at is not None:
                p[at] = 80
            test.append((int(rng.randint(0, 5)), p.tolist()))
    return _case(train, test, prefixes=False)


def _random(seed, P, users, n_train, n_test, test_rows, test_low=1):
    """Sessions of Zipf-drawn POIs 1 .. P (the test sessions': test_low .. P)."""
    rng = np.random.RandomState(seed)
    draw = lambda n, low: (int(rng.randint(0, users)), (rng.zipf(1.6, size=n) % (P - low + 1) + low).tolist())
    return [draw(int(rng.randint(2, 13)), 1) for _ in range(n_train)], [draw(test_rows(rng), test_low) for _ in range(n_test)]


def _q41():
    """41 samples, one per test session: ten whole workgroups and one wave."""
    train, test = _random(13, 40, 5, 120, 41, lambda rng: 2)
    return _case(train, test)


def _walks():
    """Every prefix of 25 test sessions of up to 19 history rows over 30 POIs.  POI 1 is in no test session, so that it is no
    sample's target: metrics.restricted_sums, which test_host_baseline.py ties `evaluate` to, follows the reference's get_acc in
    ending its hit counts at the first row whose target is column 0."""
    train, test = _random(14, 30, 6, 80, 25, lambda rng: int(rng.randint(2, 20)), test_low=2)
    return _case(train, test)


def _empty():
    """Q = 0: no session is left for the samples."""
    train, _ = _random(15, 10, 3, 12, 0, None)
    return _case(train, [])


def _untrained():
    """Nothing is trained on: every table is empty (nnz = nnzU = 0), every POI has popularity 0 and the order is the ids'."""
    c = _case([], [(0, [3, 1, 2]), (2, [5, 5, 4, 1])])
    return c


CASES = {"mini": _mini, "rows": _rows, "fill": _fill, "history": _history, "q41": _q41, "walks": _walks, "empty": _empty,
         "untrained": _untrained, "p1": lambda: _case([(0, [1, 1])], [(0, [1, 1, 1]), (3, [1, 1])]),
         "p5": lambda: _case([(0, [1, 2, 3, 2, 5]), (1, [2, 2, 4])], [(0, [2, 3, 4]), (1, [5, 1, 2, 2])])}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def host(name, order):
    c = case(name)
    return baseline.ranks_host(c.ds, c.train, c.samples, order)


@functools.lru_cache(maxsize=None)
def host_lists(name, order, k):
    c = case(name)
    return baseline.topk_host(c.ds, c.train, c.samples, order, k)


def previous_and_target(samples):
    """(base SessionDataset, a, t) of every sample: int64 [Q] each."""
    base, session, cut = baseline._samples(samples, 2 ** 31 - 1, "test")
    at = base.offsets[session] + cut
    return base, base.seq[at - 1, 0].astype(np.int64), base.seq[at, 0].astype(np.int64)
