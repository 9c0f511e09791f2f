"""Inputs and plain-loop definitions of the visit-prior tests (test_host_visitprior.py, test_gpu_visitprior.py), numpy only and
sharing nothing with the package: a dict-counter fit, a per-element blend, packed check-in logs with every shape of user the fit
has to get right, hand-made tables whose rows hit every branch of the blend, and a seeded log in which every user keeps going
back to a few slowly drifting favourites."""
import numpy as np

F = np.float32


# ---- the rule, as loops ----------------------------------------------------------------------------------------------------------------
def loop_counts(seq, offsets, users, train, P):
    """-> (rowptr, col, cnt, age, tot) as lists: a dict per user, filled row by row in dataset order"""
    U = int(max(users)) + 1 if len(users) else 0
    seen = [dict() for _ in range(U)]                                   # user -> {0-based POI: [n, last]}
    tot = [0] * U
    for s in range(len(users)):
        if not train[s]:
            continue
        u = int(users[s])
        for i in range(int(offsets[s]), int(offsets[s + 1])):
            q = int(seq[i][0]) - 1
            assert 0 <= q < P
            entry = seen[u].setdefault(q, [0, -1])
            entry[0] += 1
            entry[1] = tot[u]
            tot[u] += 1
    rowptr, col, cnt, age = [0], [], [], []
    for u in range(U):
        for q in sorted(seen[u]):
            col.append(q)
            cnt.append(seen[u][q][0])
            age.append(tot[u] - 1 - seen[u][q][1])
        rowptr.append(len(col))
    return rowptr, col, cnt, age, tot


def loop_blend(scores, user, rowptr, col, freq, rec, U, P, weights, label_offset, user_offset=1):
    """-> (f32 [G, V], status bit 1 raised or not): element by element, every product and sum an np.float32 of its own"""
    out = np.array(scores, dtype=F)
    G, V = out.shape
    wv, wr = F(weights[0]), F(weights[1])
    bad = 0
    for g in range(G):
        u = int(user[g]) - user_offset
        if not 0 <= u < U:
            continue
        r0, r1 = int(rowptr[u]), int(rowptr[u + 1])
        if r0 < 0 or r1 < r0 or r1 > len(col):
            bad = 1
            continue
        for e in range(r0, r1):
            q = int(col[e])
            if q < 0 or q >= P:
                bad = 1
                continue
            c = q + 1 - label_offset
            if 0 <= c < V:
                v = F(out[g, c] + F(wv * F(freq[e])))
                out[g, c] = F(v + F(wr * F(rec[e])))
    return out, bad


# ---- packed logs -------------------------------------------------------------------------------------------------------------------------
def pack(sessions):
    """[(user, [POIs])] -> (seq int32 [M, 3], offsets int64 [S + 1], users int64 [S]); slot and category are not read by the prior"""
    offsets = np.concatenate([[0], np.cumsum([len(p) for _, p in sessions])]).astype(np.int64)
    seq = np.zeros((int(offsets[-1]), 3), dtype=np.int32)
    if len(seq):
        seq[:, 0] = np.concatenate([np.asarray(p, dtype=np.int64) for _, p in sessions])
        seq[:, 1], seq[:, 2] = np.arange(len(seq)) % 48, 1
    return seq, offsets, np.asarray([u for u, _ in sessions], dtype=np.int64)


def dataset(seq, offsets, users):
    """A data.SessionDataset over packed arrays as they are.  Not through its constructor: that refuses a session of one row, which
    has no history to collate -- but the fit counts rows, and must count that one too."""
    from mobgt_amd.data import SessionDataset
    ds = SessionDataset.__new__(SessionDataset)
    ds.seq, ds.offsets, ds.users = seq, offsets, users
    ds.n = ds.mult = np.ones(len(users), dtype=np.int32)
    return ds


LOG_P = 2 * 1024 + 3                                                    # (2 * CHUNK + 3: the GPU test checks it against the header)
THREADS = 256


def _mixed():
    """Users 0, 6 and 12 (the first, a middle and the last id) have no train session; user 1 has a one-row train session; user 2
    has more train rows than a workgroup has threads; user 3 only ever visits POI 7; user 4 visits all P POIs (and POI 1 twice);
    users 7 .. 9 are interleaved, train and held-out sessions alternating; user 10 is random."""
    rng = np.random.RandomState(31)
    P = LOG_P
    s, train = [], []

    def add(u, pois, tr):
        s.append((u, [int(p) for p in pois]))
        train.append(tr)
    add(0, [3, 4, 5], False)
    add(1, [9], True)
    add(12, [1, 2], False)
    for _ in range(3):
        add(2, rng.randint(1, 40, size=THREADS // 2), True)
    add(3, [7] * 5, True)
    add(6, [8, 8, 9], False)
    add(3, [7, 7], True)
    add(4, np.concatenate([rng.permutation(P) + 1, [1]]), True)
    for k in range(12):
        add(7 + k % 3, rng.randint(1, 12, size=2 + k % 4), k % 4 != 1)
    add(10, rng.randint(1, P + 1, size=60), True)
    add(2, rng.randint(1, 40, size=10), False)
    add(10, rng.randint(1, P + 1, size=30), True)
    add(1, [9, 10, 9], False)
    return s, np.asarray(train), P


def _random(seed, users, sessions, P):
    rng = np.random.RandomState(seed)
    s = [(int(rng.randint(users)), rng.randint(1, P + 1, size=rng.randint(2, 12)).tolist()) for _ in range(sessions)]
    return s, rng.rand(sessions) < 0.7, P


def logs():
    """-> {name: (sessions, train flags, P)}"""
    mixed, flags, P = _mixed()
    return {"mixed": (mixed, flags, P), "nothing in train": (mixed, np.zeros(len(mixed), dtype=bool), P),
            "everything in train": (mixed, np.ones(len(mixed), dtype=bool), P), "no sessions": ([], np.zeros(0, dtype=bool), 5),
            "one user, one POI": ([(0, [1, 1])], np.ones(1, dtype=bool), 1), "random": _random(5, 40, 300, 37),
            "few POIs": _random(6, 7, 200, 3)}


# ---- tables whose rows hit every branch of the blend ---------------------------------------------------------------------------------
def tables(P, chunk, widths, seed=0):
    """-> (rowptr int64 [U + 1], col int32 [nnz], freq f32 [nnz], rec f32 [nnz], U) of U = 11 users: 0 without entries, 1 with one
    entry, 2 with all P POIs, 3 with the POIs around every edge -- column 0, the chunks' first and last columns and the last
    column of every width of `widths`, for both label offsets, and the columns just beyond -- 4 with POI 0 only, 5 with POI P - 1
    only, 6 without entries, 7 random with more entries than a workgroup has threads, 8 random and short, 9 and 10 random with
    exactly as many entries as a workgroup has threads and one more (the blend takes a row of up to that many whole and
    searches a longer one).  freq and rec are positive, of very different sizes."""
    rng = np.random.RandomState(900 + seed)
    edges = sorted({q for b in (0, chunk, 2 * chunk, *widths) for q in range(b - 3, b + 2) if 0 <= q < P})
    rows = [[], [P // 2], list(range(P)), edges, [0], [P - 1], [],
            sorted(rng.choice(P, size=min(P, THREADS + 70), replace=False).tolist()), sorted(rng.choice(P, size=min(P, 5), replace=False).tolist()),
            sorted(rng.choice(P, size=min(P, THREADS), replace=False).tolist()), sorted(rng.choice(P, size=min(P, THREADS + 1), replace=False).tolist())]
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    col = np.asarray([q for r in rows for q in r], dtype=np.int32)
    freq = np.log1p(rng.randint(1, 50, size=len(col)).astype(np.float64)).astype(F)
    rec = np.exp(rng.uniform(-9, 3, size=len(col))).astype(F)
    return rowptr, col, freq, rec, len(rows)


def users_of_rows(G, U, dtype=np.int32):
    """user ids (user + 1) of G rows: G = 16 walks through every user of `tables`, user 2 twice, and through 0 (no user), U + 1
    (beyond the table) and, for int64, 2**40"""
    far = 2 ** 40 if np.dtype(dtype).itemsize == 8 else 2 ** 31 - 1
    walk = [3, 1, 4, 0, 2, U + 1, 3, 5, far, 6, 7, 8, 9, U, -5, 10]
    return np.asarray([walk[g % len(walk)] for g in range(G)], dtype=dtype)


# ---- a log of habits ---------------------------------------------------------------------------------------------------------------------
def favourites_log(seed=0, users=30, P=400, sessions=40, favourites=8, share=0.6, drift=0.5, held_out=0.3):
    """A seeded log in which a user draws `share` of the check-ins from `favourites` POIs of their own -- the lower ranked ones
    more often -- and the rest by a heavy-tailed popularity; before every session one favourite is replaced with probability
    `drift`, so the favourites drift slowly: about 14 of a user's 28 train sessions begin with a new favourite, which is what makes
    how recently a POI was visited say something its visit count does not.  A user's sessions are consecutive, in time order,
    3 .. 9 check-ins each, and the last `held_out` of them are held out.  -> (sessions as (user, int64 [L, 3] rows (poi, slot, category)), train mask)"""
    rng = np.random.RandomState(seed)
    pop = rng.zipf(1.5, size=P).clip(max=100).astype(np.float64)
    pop /= pop.sum()
    taste = 1.0 / np.arange(1, favourites + 1)
    taste /= taste.sum()
    out, mask = [], []
    for u in range(users):
        mine = rng.choice(P, size=favourites, replace=False)
        for k in range(sessions):
            if rng.rand() < drift:
                mine[rng.randint(favourites)] = rng.randint(P)
            n = int(rng.randint(3, 10))
            own = rng.rand(n) < share
            pois = np.where(own, mine[rng.choice(favourites, size=n, p=taste)], rng.choice(P, size=n, p=pop)) + 1
            rows = np.stack([pois, (np.arange(n) + rng.randint(48)) % 48, 1 + pois % 12], 1).astype(np.int64)
            out.append((u, rows))
            mask.append(k < sessions - int(round(held_out * sessions)))
    return out, np.asarray(mask)


def held_out_prefixes(sessions, mask):
    """-> (hist int64 [n, 1]: the last history check-in, user int64 [n]: user + 1, y int64 [n]: the target POI), every prefix of
    every held-out session"""
    hist, user, y = [], [], []
    for (u, rows), tr in zip(sessions, mask):
        if tr:
            continue
        for k in range(1, len(rows)):
            hist.append([int(rows[k - 1, 0])])
            user.append(u + 1)
            y.append(int(rows[k, 0]))
    return np.asarray(hist, dtype=np.int64), np.asarray(user, dtype=np.int64), np.asarray(y, dtype=np.int64)


def mrr(scores, y, label_offset=1):
    """The mean reciprocal rank of the targets, equal scores ranked lower POI first"""
    total = 0.0
    for g in range(len(y)):
        t = int(y[g]) - label_offset
        row = scores[g]
        rank = int((row > row[t]).sum()) + int((row[:t] == row[t]).sum())
        total += 1.0 / (rank + 1)
    return total / len(y)
