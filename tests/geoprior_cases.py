"""Inputs of the distance-prior tests (test_host_geoprior.py, test_gpu_geoprior.py), numpy only: POIs of a city with exact
duplicates and a pole among them, thresholds with ties whose last is the farthest pair's own squared chord, a transition CSR
with empty rows, one full row and self-transitions, history rows that hit every branch of the anchor rule, and a seeded
distance-decay check-in log."""
import numpy as np

from mobgt_amd import geo

F = np.float32
CENTRE = (35.68, 139.76)
KM_PER_DEG = 2.0 * np.pi * geo.EARTH_RADIUS_KM / 360.0


def city(P, seed=0, box_km=20.0, special=True):
    """-> coords f64 [P, 2] degrees: uniform in a box of box_km around CENTRE; with `special` POI 2 is an exact duplicate of POI 1,
    the last POI of five or more is the north pole, and POI 4 a duplicate of it (two different longitudes at latitude 90)."""
    rng = np.random.RandomState(1000 + seed)
    half = box_km / 2.0 / KM_PER_DEG
    c = np.stack([CENTRE[0] + rng.uniform(-half, half, P), CENTRE[1] + rng.uniform(-half, half, P) / np.cos(np.radians(CENTRE[0]))], 1)
    if special and P >= 2:
        c[1] = c[0]
    if special and P >= 5:
        c[-1] = (90.0, 0.0)
        c[3] = (90.0, 0.0)
    return c


def unit(P, seed=0, **kw):
    return geo.unit_vectors_host(city(P, seed, **kw))


def chord2_max(u):
    P = u.shape[0]
    step = max(1, 4_000_000 // P)
    return max(float(geo._chord2_rows_host(u, r0, r0 + step).max()) for r0 in range(0, P, step))


def thresholds(u, nthr, seed=0):
    """-> f64 [nthr], non-decreasing: the first 0 (duplicates land in bin >= 1), the last the farthest pair's own c2 (that pair lands
    in bin nthr), between them the c2 of random pairs themselves -- so many pairs sit exactly ON a threshold -- with every
    fifth repeated (ties: empty bins)."""
    rng = np.random.RandomState(2000 + seed)
    P = u.shape[0]
    i, j = rng.randint(0, P, size=max(nthr - 2, 0)), rng.randint(0, P, size=max(nthr - 2, 0))
    d = u[i] - u[j]
    mid = np.sort(((d[:, 0] * d[:, 0]) + (d[:, 1] * d[:, 1])) + (d[:, 2] * d[:, 2]))
    k = np.arange(4, len(mid), 5)
    mid[k] = mid[k - 1]
    return np.ascontiguousarray(np.concatenate([[0.0], mid, [chord2_max(u)]]))


def csr(P, seed=0, full_row=None, big=False):
    """-> (rowptr int64 [P + 1], col int32 [nnz], val int32 [nnz]): two thirds of the rows are empty, the others hold up to 9
    distinct ascending columns, their own (a self-transition) among them; `full_row`: that row holds every POI; `big`: counts
    near 2^30, so a few of them sum past 2^31."""
    rng = np.random.RandomState(3000 + seed)
    rowptr, col = np.zeros(P + 1, dtype=np.int64), []
    for a in range(P):
        if a == full_row:
            q = np.arange(P)
        elif rng.rand() < 2 / 3:
            q = np.zeros(0, dtype=np.int64)
        else:
            q = np.unique(np.concatenate([[a], rng.randint(0, P, size=rng.randint(0, 9))]))
        col.append(q)
        rowptr[a + 1] = rowptr[a] + len(q)
    col = np.concatenate(col).astype(np.int32) if col else np.zeros(0, dtype=np.int32)
    val = rng.randint(2 ** 30 - 5, 2 ** 30 + 5, size=len(col)) if big else rng.randint(1, 400, size=len(col))
    return rowptr, col, val.astype(np.int32)


def hist_rows(G, P, n=7, seed=0, dtype=np.int32):
    """-> hist [G, n] ids: anchors walk through POI 1, P, a duplicate, the pole, then an all-pad row, ids P + 1, -3 and 2^31 - 1
    (int64: 2^40) as the last entry that is not 0, and a row whose first entry is a 0 inside the history."""
    rng = np.random.RandomState(4000 + seed)
    far = 2 ** 40 if np.dtype(dtype).itemsize == 8 else 2 ** 31 - 1
    anchors = [1, P, min(2, P), min(4, P), 0, P + 1, -3, far, max(P // 2, 1), 1, P, max(P - 1, 1), 0, P + 1, 3 % P + 1, 1]
    hist = np.zeros((G, n), dtype=dtype)
    for g in range(G):
        k = rng.randint(1, n + 1)
        hist[g, :k] = rng.randint(1, P + 1, size=k)
        hist[g, k - 1] = anchors[g % len(anchors)]
        if anchors[g % len(anchors)] == 0:
            hist[g] = 0
        elif k > 1 and g % 3 == 0:
            hist[g, 0] = 0
    return hist


def brute_bins(u, thr):
    """-> int [P, P]: bin(i, j) by a double loop and a count, nothing shared with the package but the expression of c2"""
    P = u.shape[0]
    out = np.zeros((P, P), dtype=np.int64)
    for i in range(P):
        for j in range(P):
            dx, dy, dz = u[i, 0] - u[j, 0], u[i, 1] - u[j, 1], u[i, 2] - u[j, 2]
            c2 = ((dx * dx) + (dy * dy)) + (dz * dz)
            out[i, j] = sum(1 for t in thr if t <= c2)
    return out


def decay_log(seed=7, P=400, box_km=20.0, scale_km=1.5, train=3000, test=500, length=5):
    """A seeded log whose next POI is drawn with probability ~ popularity * exp(-d / scale_km): -> (coords [P, 2], sessions as
    (user, [length + 1] POIs) lists, train mask): train / length train sessions and test / length held-out ones."""
    rng = np.random.RandomState(seed)
    c = city(P, seed, box_km, special=False)
    u = geo.unit_vectors_host(c)
    km = geo.chord2_to_km(geo._chord2_rows_host(u, 0, P))
    pop = rng.zipf(1.6, size=P).clip(max=200).astype(np.float64)
    w = pop[None, :] * np.exp(-km / scale_km)
    w /= w.sum(axis=1, keepdims=True)
    n_sessions = (train + test) // length
    sessions = []
    for s in range(n_sessions):
        p = [int(rng.choice(P, p=pop / pop.sum()))]
        for _ in range(length):
            p.append(int(rng.choice(P, p=w[p[-1]])))
        sessions.append((int(rng.randint(20)), [q + 1 for q in p]))
    mask = np.arange(n_sessions) < train // length
    return c, sessions, mask
