"""Inputs of the weight-fit tests (test_host_priorfit.py, test_gpu_priorfit.py), numpy only: seeded batches of scores, features,
targets and weight rows with a target in the first and in the last column and one out of range, rows of magnitude 80, a masked
chunk, padded rows whose padding is NaN; rows that break each finiteness condition of the rule; the gate of a comparison with
terms_host; and the held-out transitions of geoprior_cases.decay_log() with the stack's four features."""
import numpy as np

import geoprior_cases as gc
import prior_cases as pc

F = np.float32
GATE = 1e-9                                                             # of scale, see scales()
KINDS = ("nan_score", "posinf_score", "nan_feature", "neginf_feature", "all_masked", "masked_target")


def batch(G, V, K, L, seed=0, base=True, pad=0, chunk=None, ydtype=np.int64):
    """-> dict(base f32 [G, V + pad] or None, feats f32 [K, G, V + pad], y [G], offset, W f64 [L, K], V).  Columns from V on are
    NaN.  Row 0 has its target in column 0, row 1 in column V - 1, row 2 out of range (alternately below and above); every third
    row from row 1 has scores of magnitude 80; with `chunk` and a base, row 0's columns chunk .. 2 chunk - 1 are -inf (a whole
    chunk of the kernel masked).  Features differ in scale: feature k is about 0.5 (k + 1) wide."""
    rng = np.random.RandomState(10_000 + 131 * G + 17 * V + 7 * K + L + seed)
    feats = np.full((K, G, V + pad), np.nan, dtype=F)
    feats[:, :, :V] = rng.standard_normal((K, G, V)) * (0.5 * (1 + np.arange(K)))[:, None, None]
    b = None
    if base:
        b = np.full((G, V + pad), np.nan, dtype=F)
        b[:, :V] = rng.standard_normal((G, V)) * 2.0
        b[1::3, :V] = np.where(rng.rand(len(b[1::3]), V) < 0.5, -80.0, 80.0) + rng.standard_normal((len(b[1::3]), V))
        if chunk is not None and V >= 2 * chunk:
            b[0, chunk:2 * chunk] = -np.inf
    else:
        feats[0, 1::3, :V] *= 80.0                                      # (without a base the magnitude sits in feature 0)
    offset = -1
    t = rng.randint(0, V, size=G)
    t[0] = 0                                                            # (row 0 alone has the masked chunk, which never starts at 0)
    if G > 1:
        t[1] = V - 1
    if G > 2:
        t[2] = V if seed % 2 else -1
    W = rng.uniform(-1.0, 1.0, size=(L, K))
    W[0] = 0.0 if L > 1 else W[0]
    return dict(base=b, feats=feats, y=(t - offset).astype(ydtype), offset=offset, W=np.ascontiguousarray(W), V=V)


def broken(kind, G=4, V=70, K=2, L=2, seed=0):
    """batch(G, V, K, L) with a base, whose row 1 breaks one finiteness condition of the rule -> (the dict, the row)."""
    d = batch(G, V, K, L, seed=seed)
    d["y"][2] = 5 - d["offset"]                                         # (every target in range: only row 1 is left out)
    d["y"][1] = 9 - d["offset"]
    d["W"][:] = np.random.RandomState(seed).uniform(0.25, 1.0, size=d["W"].shape)
    b, f = d["base"], d["feats"]
    if kind == "nan_score":
        b[1, V - 1] = np.nan
    elif kind == "posinf_score":
        b[1, 3] = np.inf
    elif kind == "nan_feature":
        f[K - 1, 1, 0] = np.nan
    elif kind == "neginf_feature":
        f[0, 1, 17] = -np.inf                                           # (z = -inf there, legal as a score: the feature is what breaks)
    elif kind == "all_masked":
        b[1, :V] = -np.inf
    elif kind == "masked_target":
        b[1, 9] = -np.inf
    else:
        raise ValueError(kind)
    return d, 1


def scales(d, terms):
    """The scale of every entry of terms [L, G, NT] for the gate: 1 + |nll| for nll, 1 + max |F_k| for g_k, 1 + max |F_k| max |F_j|
    for H_kj (the maxima over the batch's finite feature values), 1 for n."""
    K, V = d["feats"].shape[0], d["V"]
    f = d["feats"][:, :, :V].astype(np.float64)
    top = np.array([np.abs(x[np.isfinite(x)]).max(initial=0.0) for x in f])
    iu = np.triu_indices(K)
    s = np.ones_like(terms)
    s[..., 1] = 1.0 + np.abs(terms[..., 1])
    s[..., 2:2 + K] = 1.0 + top
    s[..., 2 + K:] = 1.0 + top[iu[0]] * top[iu[1]]
    return s


def decay_world():
    """geoprior_cases.decay_log() through the package's host path: the baseline and the distance prior fitted on the 3 000 train
    transitions, the stack of both on the CPU, and the 500 held-out transitions as rows -- hist [500, 1] (the anchor), user [500],
    y [500] POI ids -- with the stack's features f32 [4, 500, P]."""
    import torch
    from mobgt_amd import baseline, data, geo, prior
    coords, sessions, train = gc.decay_log()
    ds = data.SessionDataset([(u, pc.as_checkins(p)) for u, p in sessions])
    P = len(coords)
    mb = baseline.MarkovBaseline.fit(ds, train, P=P, device="cpu")
    pb = geo.pair_bins(coords, edges=np.arange(0.0, 30.0, 0.5), device="cpu")
    stack = prior.Stack(mb.prior(), mb.distance_prior(pb))
    held = [(u, p) for (u, p), tr in zip(sessions, train) if not tr]
    hist = torch.tensor([[a] for _, p in held for a in p[:-1]], dtype=torch.int64)
    user = torch.tensor([u + 1 for u, p in held for _ in p[:-1]], dtype=torch.int64)
    y = np.array([b for _, p in held for b in p[1:]], dtype=np.int64)
    feats = stack.features((hist, user), 1, torch.zeros(4, len(y), P))
    return dict(stack=stack, hist=hist, user=user, y=y, feats=feats.numpy(), P=P)
