"""Inputs of the context-prior tests (test_host_ctxprior.py, test_gpu_ctxprior.py), numpy only: packed check-in sessions with
sessions of one pair, long ones, sessions out of train and a slot-0 row; random tables with POIs without a category; rows of
samples that hit every branch of the blend's rule; and a seeded check-in log whose next category depends on the previous
category and on the previous check-in's time slot."""
import numpy as np

from mobgt_amd import ctxprior

F = np.float32


def packed(lengths, n_slots, n_cat, seed=0, train=0.7):
    """-> (seq int32 [M, 3], offsets int64 [S + 1], train uint8 [S]): sessions of the given numbers of rows, slot and category
    uniform in their ranges, the POI one of three of its category (POI p has category 1 + (p - 1) mod n_cat), the first row of
    the log in slot 0; `train`: the share of train sessions, or an array of flags."""
    rng = np.random.RandomState(500 + seed)
    lengths = np.asarray(lengths, dtype=np.int64)
    M = int(lengths.sum())
    cat = rng.randint(1, n_cat + 1, size=M)
    seq = np.stack([cat + n_cat * rng.randint(0, 3, size=M), rng.randint(0, n_slots, size=M), cat], 1).astype(np.int32)
    if M:
        seq[0, 1] = 0
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    flags = (rng.rand(len(lengths)) < train) if np.isscalar(train) else np.asarray(train)
    return seq, offsets, flags.astype(np.uint8)


def loop_hist(seq, offsets, train, n_slots, n_cat):
    """st by a plain Python loop over the sessions and their pairs: nothing shared with the package"""
    st = [[0] * n_cat for _ in range(n_slots)]
    for s in range(len(offsets) - 1):
        if not train[s]:
            continue
        for k in range(int(offsets[s]) + 1, int(offsets[s + 1])):
            st[int(seq[k - 1][1])][int(seq[k][2]) - 1] += 1
    return st


def tables(P, n_cat, n_slots, seed=0, wild=True):
    """-> ContextTables of random f32 tables; a fifth of the POIs have no category (0) and, with `wild`, POI 3 holds n_cat + 1
    and POI 5 holds -1: values the rule never uses as an index."""
    rng = np.random.RandomState(600 + seed)
    poi_cat = rng.randint(1, n_cat + 1, size=P).astype(np.int32)
    poi_cat[rng.rand(P) < 0.2] = 0
    poi_cat[-1] = n_cat                                                 # the last POI and the last category are used
    if wild and P >= 6:
        poi_cat[2], poi_cat[4] = n_cat + 1, -1
    Tc = (rng.standard_normal((n_cat, n_cat)) * 2).astype(F)
    Tt = (rng.standard_normal((n_slots, n_cat)) * 2).astype(F)
    return ctxprior.ContextTables(poi_cat, Tc, Tt, P, n_cat, n_slots)


# (anchor id, category, slot) of the anchor position, by row; P, C, S stand for the sizes: every invalid-context case of the rule
CONTEXTS = (("p", "c", "s"), ("P", "C", "S-1"), ("p", 1, 0), (0, "c", "s"), ("P+1", "c", "s"), ("p", 0, "s"), ("p", "C+1", "s"),
            ("p", "c", -1), ("p", "c", "S"), ("p", 0, -1), (-3, "c", "s"), ("far", "c", "s"), ("p", "far", "s"), ("p", "c", "far"),
            ("p", -2, "S+5"), (1, "C", 0))


def sample_rows(G, P, n_cat, n_slots, n=7, seed=0, dtype=np.int32, ctx_dtype=None):
    """-> (hist, time, cat) [G, n]: the anchor positions walk through CONTEXTS -- valid rows, no anchor, an anchor id beyond P,
    negative and beyond 31 bits, a category of 0, n_cat + 1, negative and huge, a slot of -1, n_slots and huge; every third row
    has a 0 inside its history, and the positions after the anchor hold slots and categories that must not be read as its own."""
    rng = np.random.RandomState(700 + seed)
    ctx_dtype = dtype if ctx_dtype is None else ctx_dtype
    hist, time, cat = np.zeros((G, n), dtype=dtype), np.zeros((G, n), dtype=ctx_dtype), np.zeros((G, n), dtype=ctx_dtype)
    far = lambda dt: 2 ** 40 if np.dtype(dt).itemsize == 8 else 2 ** 31 - 1
    for g in range(G):
        a, c, s = CONTEXTS[g % len(CONTEXTS)]
        k = rng.randint(1, n + 1)
        hist[g, :k] = rng.randint(1, P + 1, size=k)
        time[g] = rng.randint(0, n_slots, size=n)
        cat[g] = rng.randint(1, n_cat + 1, size=n)
        names = {"p": rng.randint(1, P + 1), "P": P, "P+1": P + 1, "c": rng.randint(1, n_cat + 1), "C": n_cat, "C+1": n_cat + 1,
                 "s": rng.randint(0, n_slots), "S-1": n_slots - 1, "S": n_slots, "S+5": n_slots + 5}
        hist[g, k - 1] = far(dtype) if a == "far" else names.get(a, a)
        cat[g, k - 1] = far(ctx_dtype) if c == "far" else names.get(c, c)
        time[g, k - 1] = far(ctx_dtype) if s == "far" else names.get(s, s)
        if a == 0:
            hist[g] = 0
        elif k > 1 and g % 3 == 0:
            hist[g, 0] = 0
    return hist, time, cat


def anchors(hist, time, cat):
    """-> [(id, category, slot) or None per row] by a plain loop: the last position whose id is not 0"""
    out = []
    for g in range(len(hist)):
        at = [i for i in range(hist.shape[1]) if hist[g, i] != 0]
        out.append((int(hist[g, at[-1]]), int(cat[g, at[-1]]), int(time[g, at[-1]])) if at else None)
    return out


def context_log(seed=0, P=400, n_cat=12, n_slots=48, sessions=720, length=8, concentration=0.15, train=0.7, users=20):
    """A seeded log whose next category is drawn ~ A[previous category] * T[previous slot], A [n_cat, n_cat] and T [n_slots, n_cat]
    rows of Dirichlet(concentration), and whose POI inside the category is drawn by a heavy-tailed popularity.  Every category owns
    at least one POI; a session starts at a random slot and moves on by 0 .. 3 slots per check-in (mod n_slots).
    -> (sessions as (user, int64 [length + 1, 3] rows (poi, slot, category)), train mask, poi_cat int [P])"""
    rng = np.random.RandomState(seed)
    A = rng.dirichlet([concentration] * n_cat, size=n_cat)
    T = rng.dirichlet([concentration] * n_cat, size=n_slots)
    poi_cat = np.concatenate([np.arange(1, n_cat + 1), rng.randint(1, n_cat + 1, size=P - n_cat)])
    pop = rng.zipf(1.6, size=P).clip(max=200).astype(np.float64)
    inside = []                                                         # per category: its POIs and their popularity shares
    for c in range(1, n_cat + 1):
        mine = np.nonzero(poi_cat == c)[0]
        inside.append((mine, pop[mine] / pop[mine].sum()))
    out = []
    for _ in range(sessions):
        p = int(rng.choice(P, p=pop / pop.sum()))
        slot = int(rng.randint(n_slots))
        rows = [(p + 1, slot, int(poi_cat[p]))]
        for _ in range(length):
            w = A[rows[-1][2] - 1] * T[rows[-1][1]] + 1e-12
            c = int(rng.choice(n_cat, p=w / w.sum()))
            p = int(rng.choice(inside[c][0], p=inside[c][1]))
            slot = (slot + int(rng.randint(4))) % n_slots
            rows.append((p + 1, slot, c + 1))
        out.append((int(rng.randint(users)), np.asarray(rows, dtype=np.int64)))
    mask = rng.rand(sessions) < train
    return out, mask, poi_cat


def held_out_prefixes(sessions, mask):
    """-> (hist, time, cat int64 [n, 1], user int64 [n], y [n]): every prefix of every held-out session, as its anchor row (the
    last history check-in) and its target POI"""
    rows, user, y = [], [], []
    for (u, s), tr in zip(sessions, mask):
        if tr:
            continue
        for k in range(1, len(s)):
            rows.append(s[k - 1])
            user.append(u + 1)
            y.append(int(s[k, 0]))
    rows = np.asarray(rows, dtype=np.int64)
    return rows[:, 0:1], rows[:, 1:2], rows[:, 2:3], np.asarray(user, dtype=np.int64), np.asarray(y, dtype=np.int64)
