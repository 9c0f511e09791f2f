"""Evaluation metrics of `graphormer/model_fqandtoyo.py`: `get_acc` (:48-90) and
`MRR_metric` (:122-131), evaluated on the device with one `topk` / one rank computation for the whole
batch instead of per-row Python loops.  Quirks kept: row order of the result (`[top10, top5, top1, top20]`),
targets are class ids already shifted by the caller (`y - 1`, :1487), and `get_acc` stops at the FIRST row
whose target is 0 (:88-89) -- rows after it are ignored, exactly as in the reference.
"""
import numpy as np
import torch


def get_acc(target, scores):
    """-> (acc [4,1], ndcg [4,1]) numpy arrays: rows = top-10, top-5, top-1, top-20 hit counts / DCG sums."""
    target = torch.as_tensor(target).reshape(-1).to(scores.device)
    n = target.numel()
    zero = (target == 0).nonzero()
    stop = int(zero[0]) if zero.numel() else n                       # `else: break` at the first target == 0
    acc, ndcg = np.zeros((4, 1)), np.zeros((4, 1))
    if stop == 0:
        return acc, ndcg
    if scores.is_cuda:                                                 # one rank kernel instead of a top-k + search
        from . import ops
        rank = ops.target_rank(scores[:stop], target[:stop])[:, 0].long()
        found = (rank >= 0) & (rank < 20)
    else:
        _, idx = scores[:stop].topk(20, dim=1)
        hit = idx == target[:stop].unsqueeze(1)                        # at most one True per row
        rank = hit.float().argmax(dim=1)                               # position of the hit (0 when no hit)
        found = hit.any(dim=1)
    gain = 1.0 / torch.log2(rank.clamp(min=0).double() + 2.0)
    for row, k in ((3, 20), (0, 10), (1, 5), (2, 1)):
        m = found & (rank < k)
        acc[row] = float(m.sum())
        ndcg[row] = float(gain[m].sum())
    return acc, ndcg


def MRR_metric(target, scores):
    """Sum over rows of 1 / rank of the target under a descending sort (ties: numpy argsort order of the
    reference is approximated by counting strictly greater scores plus earlier-index... see note)."""
    target = torch.as_tensor(target).reshape(-1).to(scores.device)
    if scores.is_cuda:
        from . import ops
        r_idx = ops.target_rank(scores, target)[:, 1]
        return float((1.0 / (r_idx.double() + 1.0)).sum())
    s = scores.double()
    t = s.gather(1, target.long().unsqueeze(1))
    # reference: rec_list = argsort(row)[::-1]; r_idx = position of the target.  For distinct scores this is the
    # number of strictly larger scores; with ties, reversed ascending argsort puts LATER indices first.
    greater = (s > t).sum(dim=1)
    cols = torch.arange(s.shape[1], device=s.device).unsqueeze(0)
    ties_before = ((s == t) & (cols > target.long().unsqueeze(1))).sum(dim=1)
    r_idx = greater + ties_before
    return float((1.0 / (r_idx.double() + 1.0)).sum())


def evaluate_outputs(outputs):
    """`test_epoch_end` bookkeeping (model_fqandtoyo.py:1546-1597) over a list of {"y_pred": [poi, cat], "y_true"}:
    returns dict(acc@1/5/10/20, ndcg@1/5/10/20, mrr), each averaged over the number of test samples."""
    tot = np.zeros(8)
    mrr, n = 0.0, 0
    for o in outputs:
        y_pred, y_true = o["y_pred"][0], o["y_true"]
        a, d = get_acc(y_true, y_pred)
        tot += np.array([a[2, 0], a[1, 0], a[0, 0], d[2, 0], d[1, 0], d[0, 0], a[3, 0], d[3, 0]])
        mrr += MRR_metric(y_true, y_pred)
        n += len(y_true)
    tot /= max(n, 1)
    return {"acc@1": tot[0], "acc@5": tot[1], "acc@10": tot[2], "ndcg@1": tot[3], "ndcg@5": tot[4], "ndcg@10": tot[5],
            "acc@20": tot[6], "ndcg@20": tot[7], "mrr": mrr / max(n, 1)}


# ---- device accumulation (ops.rank_metrics / ops.skinny_linear_rank_metrics, train.EvalLoop) --------------------------------------
# One f64 [10] tensor on the device: {n, hit@1, hit@5, hit@10, hit@20, dcg@1, dcg@5, dcg@10, dcg@20, sum 1 / rank}.  A batch adds
# exactly what evaluate_outputs adds for it (counts bit for bit; the DCG / MRR sums in another order: ~1e-16 relative), so a whole
# split is one host read at the end.
ACC_FIELDS = ("n", "hit@1", "hit@5", "hit@10", "hit@20", "dcg@1", "dcg@5", "dcg@10", "dcg@20", "rr")


def new_accumulator(device):
    return torch.zeros(len(ACC_FIELDS), dtype=torch.float64, device=device)


def finalize(acc):
    """The dict of evaluate_outputs (each sum divided by the number of samples) plus "n", from an accumulator (device or host)."""
    a = np.asarray(torch.as_tensor(acc).detach().double().cpu().numpy(), dtype=np.float64).reshape(-1)
    assert a.size == len(ACC_FIELDS)
    n = a[0]
    d = max(n, 1.0)
    out = {k: float(a[i] / d) for k, i in (("acc@1", 1), ("acc@5", 2), ("acc@10", 3), ("ndcg@1", 5), ("ndcg@5", 6), ("ndcg@10", 7),
                                              ("acc@20", 4), ("ndcg@20", 8), ("mrr", 9))}
    out["n"] = int(n)
    return out


# ---- restricted and split evaluation (ops.rank_metrics_masked, train.EvalLoop(exclude_visited=, candidates=, split_revisits=)) ---
# Slots of 11 f64: ACC_FIELDS, then the rows whose target can be listed at all.  One slot, or three with the split: every row /
# rows whose target is not among the trajectory's POIs (new) / rows whose target is (revisit).
RACC_FIELDS = ACC_FIELDS + ("reachable",)
SPLIT_SLOTS = ("all", "new", "revisit")


def new_restricted_accumulator(device, split=False):
    return torch.zeros(3 if split else 1, len(RACC_FIELDS), dtype=torch.float64, device=device)


def _finalize_slot(a):
    out = finalize(a[:len(ACC_FIELDS)])
    out["reachable"] = int(a[len(ACC_FIELDS)])
    return out


def finalize_restricted(acc):
    """finalize's dict of slot 0 plus "reachable"; with the split also "new" and "revisit", dicts of the same keys over their
    rows.  Averages are over each slot's n (every row, reachable or not: the reference's denominator)."""
    a = np.asarray(torch.as_tensor(acc).detach().double().cpu().numpy(), dtype=np.float64).reshape(-1, len(RACC_FIELDS))
    assert a.shape[0] in (1, 3), "acc: new_restricted_accumulator's [1, 11] or [3, 11]"
    out = _finalize_slot(a[0])
    if a.shape[0] == 3:
        out["new"], out["revisit"] = _finalize_slot(a[1]), _finalize_slot(a[2])
    return out


def restricted_sums(scores, target, target_offset=0, allow=None, hist=None, hist_offset=0, exclude_hist=False, split=False):
    """The contract of mobgt_rank_metrics_masked in torch, on the scores' device: one batch's f64 [1 or 3, 11] slot sums.

    Per row g, t = target[g] + target_offset.  Column c is a candidate when its bit of `allow` (ops.pack_allow words; None: every
    column) is set and, with exclude_hist, no entry p != 0 of hist[g] has p - hist_offset == c (0 is padding, ids outside [0, V)
    are ignored).  The row is reachable when t is in [0, V) and a candidate; its ACC / NDCG position is the number of candidates
    scoring above s[t] plus the equal-scored candidates at lower columns, its MRR position the same with higher columns.  An
    unreachable row adds to n only.  Hits and DCG stop at the batch's first row with t == 0 (get_acc).  split: slot 1 takes the
    rows whose t is not among their hist ids, slot 2 the others (hist read whether or not exclude_hist is set)."""
    from . import ops
    G, V = scores.shape
    dev = scores.device
    t = target.reshape(-1)[:G].to(device=dev, dtype=torch.int64) + int(target_offset)
    ok = (t >= 0) & (t < V)
    tc = t.clamp(0, V - 1)
    rows = torch.arange(G, device=dev)
    use_hist = hist is not None and hist.numel() > 0
    cand = ops._candidates(G, V, allow, hist if exclude_hist and use_hist else None, hist_offset, dev)
    reach = ok & cand[rows, tc]
    if use_hist:
        h = hist.to(device=dev, dtype=torch.int64)
        in_hist = ok & ((h != 0) & (h - int(hist_offset) == t[:, None])).any(1)
    else:
        in_hist = torch.zeros(G, dtype=torch.bool, device=dev)
    s = scores
    ts = s[rows, tc][:, None]
    cols = torch.arange(V, device=dev)[None, :]
    greater = ((s > ts) & cand).sum(1)
    lo = greater + ((s == ts) & cand & (cols < tc[:, None])).sum(1)
    hi = greater + ((s == ts) & cand & (cols > tc[:, None])).sum(1)
    zero = (t == 0).nonzero()
    live = rows < (int(zero[0]) if zero.numel() else G)
    gain = 1.0 / torch.log2(lo.double() + 2.0)
    rr = 1.0 / (hi.double() + 1.0)
    out = torch.zeros(3 if split else 1, len(RACC_FIELDS), dtype=torch.float64, device=dev)
    sels = (torch.ones(G, dtype=torch.bool, device=dev), ~in_hist, in_hist)[:3 if split else 1]
    for i, sel in enumerate(sels):
        r = sel & reach
        out[i, 0] = sel.sum()
        for q, k in enumerate((1, 5, 10, 20)):
            h = r & live & (lo < k)
            out[i, 1 + q] = h.sum()
            out[i, 5 + q] = gain[h].sum()
        out[i, 9] = rr[r].sum()
        out[i, 10] = r.sum()
    return out
