"""Host half of the device evaluation (train.EvalLoop, metrics.finalize): no GPU needed.

  * the eval batch order is the reference's eval DataLoader -- no shuffle, consecutive runs of batch_size, drop_last=False --
    and, per rank, the non-shuffling DistributedSampler;
  * metrics.finalize turns a filled accumulator into evaluate_outputs' dict (+ n), and agrees with evaluate_outputs' CPU path.
"""
import numpy as np
import torch

from mobgt_amd import metrics
from mobgt_amd.train import EvalLoop


def _order(n, batch_size, rank, world):
    loop = EvalLoop.__new__(EvalLoop)                # (the batch order needs no device state)
    loop.dataset, loop.batch_size, loop.rank, loop.world = [None] * n, batch_size, rank, world
    return loop.batches()


def test_eval_batch_order_is_the_non_shuffling_sampler():
    from torch.utils.data import DataLoader
    from torch.utils.data.distributed import DistributedSampler
    n, B = 37, 16
    assert _order(n, B, 0, 1) == [list(b) for b in DataLoader(range(n), batch_size=B, shuffle=False, drop_last=False)]
    assert _order(n, B, 0, 1)[-1] == list(range(32, 37))
    for r in range(2):
        want = list(DistributedSampler(range(n), num_replicas=2, rank=r, shuffle=False))
        assert [i for b in _order(n, B, r, 2) for i in b] == want
        assert [len(b) for b in _order(n, B, r, 2)] == [16, 3]
    assert _order(n, B, 1, 2)[-1][-1] == 0           # the wrap-around duplicate of the padded sampler


def test_finalize_of_a_hand_filled_accumulator():
    acc = torch.tensor([8.0, 2, 3, 5, 6, 2.0, 2.5, 3.1, 3.3, 4.0], dtype=torch.float64)
    r = metrics.finalize(acc)
    assert set(r) == {"acc@1", "acc@5", "acc@10", "acc@20", "ndcg@1", "ndcg@5", "ndcg@10", "ndcg@20", "mrr", "n"}
    assert r["n"] == 8
    assert (r["acc@1"], r["acc@5"], r["acc@10"], r["acc@20"]) == (0.25, 0.375, 0.625, 0.75)
    assert (r["ndcg@1"], r["ndcg@5"], r["ndcg@10"], r["ndcg@20"], r["mrr"]) == (0.25, 2.5 / 8, 3.1 / 8, 3.3 / 8, 0.5)
    assert metrics.finalize(metrics.new_accumulator("cpu"))["acc@1"] == 0.0


def test_finalize_agrees_with_evaluate_outputs_bookkeeping():
    """The accumulator's fields, filled on the host from evaluate_outputs' CPU path (top-k + argsort ranks), give its dict."""
    rng = np.random.RandomState(3)
    outs, acc = [], np.zeros(10)
    for G in (16, 16, 5):
        s = torch.from_numpy(rng.standard_normal((G, 50)).astype(np.float32))
        t = torch.from_numpy(rng.randint(1, 50, G))
        t[2] = 0 if G == 5 else t[2]
        outs.append({"y_pred": [s, None], "y_true": t})
        a, d = metrics.get_acc(t, s)
        acc += [G, a[2, 0], a[1, 0], a[0, 0], a[3, 0], d[2, 0], d[1, 0], d[0, 0], d[3, 0], metrics.MRR_metric(t, s)]
    want = metrics.evaluate_outputs(outs)
    got = metrics.finalize(torch.from_numpy(acc))
    assert got["n"] == 37
    for k, v in want.items():
        np.testing.assert_allclose(got[k], v, rtol=1e-15, err_msg=k)
