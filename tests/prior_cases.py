"""Inputs of the Markov-prior tests (test_host_prior.py, test_gpu_prior.py), numpy only: a miniature whose blended rows are written
out by hand, generated tables whose CSR rows have 0, 1, 63, 64, 65 and 200 entries with entries on either side of the kernel's
chunk boundary, rows of samples that hit every branch of the rule, and seeded random-walk sessions for the forms that count."""
import numpy as np

CHUNK = 2048                                                            # (= _prior.CHUNK: test_host_prior.py asserts it)
F = np.float32


def L(count):
    """f32(log1p(count)): an entry of the log tables"""
    return F(np.log1p(np.float64(count)))


# ---- a miniature: 5 POIs, 2 users ----------------------------------------------------------------------------------------------------
MINI_P = 5
MINI_TRAIN = [(0, [1, 2, 3]), (0, [1, 2, 1]), (1, [1, 3, 3]), (1, [4, 1, 2])]
# what those sessions count to (POI 5 is never visited):
MINI_CG = {1: {2: 3, 3: 1}, 2: {1: 1, 3: 1}, 3: {3: 1}, 4: {1: 1}}
MINI_CU = {(0, 1): {2: 2}, (0, 2): {1: 1, 3: 1}, (1, 1): {2: 1, 3: 1}, (1, 3): {3: 1}, (1, 4): {1: 1}}
MINI_POP = [5, 3, 3, 1, 0]
MINI_WEIGHTS = (0.5, 2.0, 0.25)                                         # (user, transition, popularity)
MINI_SCORES = np.array([0.5, -1.0, 0.25, 2.0, -0.0], dtype=F)          # every row starts from these; label_offset 1, V = 5
WU, WG, WP = (F(w) for w in MINI_WEIGHTS)
S = MINI_SCORES
_POP_ONLY = [F(S[0] + F(WP * L(5))), F(S[1] + F(WP * L(3))), F(S[2] + F(WP * L(3))), F(S[3] + F(WP * L(1))), S[4]]
# (hist row, user + 1, the blended row): each sum is rounded on its own, in the rule's order
MINI_ROWS = [
    # user 0 after POI 1: cg(1, 2) = 3 with cu(0, 1, 2) = 2; cg(1, 3) = 1 without a user count; POI 5 keeps its -0.0
    ([3, 1, 0, 0], 1, [_POP_ONLY[0], F(F(_POP_ONLY[1] + F(WG * L(3))) + F(WU * L(2))), F(_POP_ONLY[2] + F(WG * L(1))), _POP_ONLY[3], S[4]]),
    # an empty G_a: POI 5 was never left
    ([2, 5, 0, 0], 1, _POP_ONLY),
    # a user absent from training (7 >= U) after POI 1: the transition terms without the user's
    ([1, 0, 0, 0], 8, [_POP_ONLY[0], F(_POP_ONLY[1] + F(WG * L(3))), F(_POP_ONLY[2] + F(WG * L(1))), _POP_ONLY[3], S[4]]),
    # user 1 after POI 2: in range, but no (1, 2, .) rows
    ([1, 2, 0, 0], 2, [F(_POP_ONLY[0] + F(WG * L(1))), _POP_ONLY[1], F(_POP_ONLY[2] + F(WG * L(1))), _POP_ONLY[3], S[4]]),
    # no anchor: an all-pad row, and an id beyond P
    ([0, 0, 0, 0], 1, _POP_ONLY),
    ([1, 6, 0, 0], 1, _POP_ONLY),
]


# ---- generated tables ----------------------------------------------------------------------------------------------------------------
ROW_LENGTHS = (0, 1, 63, 64, 65, 200)                                   # CSR rows of anchors 1 .. 6
GEN_P = 2 * CHUNK + 5
GEN_U = 4                                                               # users 0 .. 3; user 3 has no rows
BOUNDARY = (CHUNK - 2, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK)       # 0-based POIs on either side of a chunk edge, for both offsets


def generated(seed=0, P=GEN_P):
    """-> dict(rowptr, col, val, ukey, uval, pop, U, P) of integer numpy arrays: counts as MarkovBaseline.fit would hold them.
    Rows 1 .. 6 have ROW_LENGTHS entries (at most P); the rows of 63 and more hold every POI of BOUNDARY; row P is the last non-empty one
    and ends at POI P.  cu: users 0 .. 2 hold a random part of every row, with smaller counts."""
    rng = np.random.RandomState(seed)
    rows = {}
    for a, n in zip(range(1, 7), ROW_LENGTHS):
        n = min(n, P)                                                   # (a small universe: the long rows hold every POI)
        forced = [q for q in BOUNDARY if q < P][:n] if n >= 63 else []
        rest = rng.choice(np.setdiff1d(np.arange(P), forced), size=n - len(forced), replace=False)
        rows[a] = np.sort(np.concatenate([np.asarray(forced, dtype=np.int64), rest]))
    rows[P] = np.array([0, P - 1])
    rowptr, col, val, ukey, uval = np.zeros(P + 1, dtype=np.int64), [], [], [], []
    for a in range(1, P + 1):
        q = rows.get(a, np.zeros(0, dtype=np.int64))
        rowptr[a] = rowptr[a - 1] + len(q)
        col.append(q)
        val.append(rng.randint(1, 400, size=len(q)))
    col, val = np.concatenate(col).astype(np.int32), np.concatenate(val).astype(np.int32)
    for u in range(GEN_U - 1):
        for a in sorted(rows):
            for e in range(rowptr[a - 1], rowptr[a]):
                if rng.rand() < 0.4:
                    ukey.append((u * P + a - 1) * P + int(col[e]))
                    uval.append(rng.randint(1, int(val[e]) + 1))
    pop = rng.randint(0, 3, size=P) * rng.randint(1, 5000, size=P)     # (a third of the POIs were never visited)
    return dict(rowptr=rowptr, col=col, val=val, ukey=np.asarray(ukey, dtype=np.int64), uval=np.asarray(uval, dtype=np.int32),
                pop=pop.astype(np.int32), U=GEN_U, P=P)


def sample_rows(G, P, n=7, seed=0, dtype=np.int32):
    """-> (hist [G, n] ids, user [G] = user + 1): the anchors walk through rows 1 .. 6 and P, then an all-pad row, an anchor id
    P + 1, a user at U, a user with no rows (U - 1)."""
    rng = np.random.RandomState(100 + seed)
    hist, user = np.zeros((G, n), dtype=dtype), np.zeros(G, dtype=dtype)
    anchors = [6, 4, 5, 3, 2, 1, P, 0, P + 1, 6, 6, 5, 4, 3, 6, 2]
    users = [0, 1, 2, 0, 1, 2, 0, 1, 2, GEN_U, GEN_U - 1, 1, 0, 2, 2, 0]
    for g in range(G):
        k = rng.randint(1, n + 1)                                       # entries before the padding
        hist[g, :k] = rng.randint(1, P + 1, size=k)
        hist[g, k - 1] = anchors[g % len(anchors)]                      # (0: the row is all pad only if everything before is too)
        if anchors[g % len(anchors)] == 0:
            hist[g] = 0
        elif k > 1 and g % 3 == 0:
            hist[g, 0] = 0                                              # a 0 inside the history is skipped, not an end
        user[g] = users[g % len(users)] + 1
    return hist, user


def scores(G, V, seed=0):
    """f32 [G, V] normal scores with +inf, -inf, -0.0 and two NaN payloads sown in"""
    rng = np.random.RandomState(200 + seed)
    s = rng.standard_normal((G, V)).astype(F)
    if s.size == 0:
        return s
    flat = s.reshape(-1).view(np.uint32)
    special = np.array([0x7F800000, 0xFF800000, 0x80000000, 0x7FC00001, 0xFFC12345, 0x80000000], dtype=np.uint32)
    at = rng.choice(G * V, size=min(G * V, max(6, G * V // 16)), replace=False)
    flat[at] = special[np.arange(len(at)) % len(special)]
    return s


# ---- sessions for the forms that count -------------------------------------------------------------------------------------------------
def walks(seed=3, P=30, users=5, sessions=60):
    """-> list of (user, [L + 1] POIs): random walks with a strong habit (every user favours a few transitions), lengths 2 .. 9;
    some sessions are A, B, A, t.  The last two POIs are never visited."""
    rng = np.random.RandomState(seed)
    P = P - 2
    nxt = rng.randint(1, P + 1, size=(users, P + 1))
    out = []
    for s in range(sessions):
        u = int(rng.randint(users))
        n = int(rng.randint(2, 10))
        p = [int(rng.randint(1, P + 1))]
        while len(p) < n:
            p.append(int(nxt[u, p[-1]]) if rng.rand() < 0.7 else int(rng.randint(1, P + 1)))
        if s % 10 == 0:
            a, b = p[0], p[0] % P + 1
            p = [a, b, a, int(rng.randint(1, P + 1))]
        out.append((u, p))
    return out


def as_checkins(pois):
    """[L + 1] POIs -> [L + 1, 3] rows (poi, time slot, category)"""
    p = np.asarray(pois, dtype=np.int64)
    return np.stack([p, 1 + np.arange(len(p)) % 47, 1 + p % 7], axis=1)
