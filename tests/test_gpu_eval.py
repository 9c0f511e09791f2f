"""The device evaluation path: `ops.rank_metrics` / `ops.skinny_linear_rank_metrics` (csrc/skinny.hip, evaluation section),
`Graphormer.metric_step` and `train.EvalLoop` -- the reference's validation / test protocol (model_fqandtoyo.py:48-131,
:1484-1597) on the device data path.

  * the stored-scores kernel gives the reference's own numbers (golden G7), get_acc's stop at the first target 0 included;
  * the fused classifier + ranking launches give the same accumulator bits as skinny_linear + rank_metrics, with ties engineered
    on both sides of the target (bit-identical logits, both tie rules), and the counts of evaluate_outputs;
  * a captured graph of the launches replayed n times adds exactly n x one call;
  * EvalLoop (graphs and eager) equals evaluate_outputs over test_step outputs of the same batches at the same padding;
  * an evaluation between training epochs sees the current weights and leaves the training run alone;
  * toyotagraph ranks log_softmax(logits) against the unshifted y;
  * the eval batch order of two ranks pools to the one-rank result over both shards.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mobgt_amd import metrics, ops, workloads                              # noqa: E402
from mobgt_amd.data import bucket_nodes                                     # noqa: E402
from mobgt_amd.train import EpochLoop, EvalLoop                             # noqa: E402

DEV = "cuda"
COUNTS = ("n", "acc@1", "acc@5", "acc@10", "acc@20")
SUMS = ("ndcg@1", "ndcg@5", "ndcg@10", "ndcg@20", "mrr")


def _same(got, want):
    for k in COUNTS[1:]:
        assert got[k] == want[k], (k, got[k], want[k])
    for k in SUMS:
        np.testing.assert_allclose(got[k], want[k], rtol=1e-12, atol=0, err_msg=k)


def _acc_of(fn):
    acc = metrics.new_accumulator(DEV)
    fn(acc)
    return acc


def test_rank_metrics_kernel_matches_reference_g7(golden_dir):
    z = np.load(os.path.join(golden_dir, "g7_lr_loss.npz"))
    scores, target = torch.from_numpy(z["acc/scores"]).to(DEV), torch.from_numpy(z["acc/target"]).to(DEV)
    G = scores.shape[0]
    r = metrics.finalize(_acc_of(lambda a: ops.rank_metrics(scores, target, a)))
    assert r["n"] == G
    a, d = z["acc/acc"][:, 0], z["acc/ndcg"][:, 0]                 # rows: top-10, top-5, top-1, top-20
    for k, row in (("1", 2), ("5", 1), ("10", 0), ("20", 3)):
        assert r["acc@" + k] * G == a[row], k
        np.testing.assert_allclose(r["ndcg@" + k] * G, d[row], rtol=1e-12)
    np.testing.assert_allclose(r["mrr"] * G, float(z["acc/mrr"]), rtol=1e-12)
    # a target 0 in row 5: hits and DCG stop there (rows 0-4 count), n and MRR still count every row
    t2 = target.clone()
    t2[5] = 0
    r2 = metrics.finalize(_acc_of(lambda a: ops.rank_metrics(scores, t2, a)))
    r5 = metrics.finalize(_acc_of(lambda a: ops.rank_metrics(scores[:5], target[:5], a)))
    for k in ("acc@1", "acc@5", "acc@10", "acc@20", "ndcg@1", "ndcg@5", "ndcg@10", "ndcg@20"):
        np.testing.assert_allclose(r2[k] * G, r5[k] * 5, rtol=1e-12, err_msg=k)
    np.testing.assert_allclose(r2["mrr"] * G, metrics.MRR_metric(t2, scores), rtol=1e-12)
    # target_offset: 1-based targets with offset -1 are the same call
    r3 = metrics.finalize(_acc_of(lambda a: ops.rank_metrics(scores, target + 1, a, target_offset=-1)))
    assert r3 == r


def _tied_classifier(G, K, V, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(G, K, generator=g)
    w = torch.randn(V, K, generator=g) * 0.05
    b = torch.randn(V, generator=g) * 0.05
    t = torch.randint(1, V - 1, (G,), generator=g)
    t[0] = V - 1                                               # (last column: the last, partial tile)
    if G > 3:
        t[G // 2] = 0                                           # get_acc's stop rule mid-batch
    for gi in range(G):
        tv = int(t[gi])
        for c in (tv - 7, tv - 1, tv + 1, tv + 5, tv + 16):      # exact ties below and above the target, across tile boundaries
            if 0 <= c < V and c not in t.tolist():
                w[c], b[c] = w[tv], b[tv]
    return x.to(DEV), w.to(DEV), b.to(DEV), t.to(DEV)


@pytest.mark.parametrize("G", [1, 5, 16])
@pytest.mark.parametrize("K", [320, 384, 448])
@pytest.mark.parametrize("V", [1024, 7857, 100001])
def test_fused_classifier_ranking_equals_unfused_exactly(G, K, V):
    x, w, b, t = _tied_classifier(G, K, V, seed=G * 1000 + K + V)
    fused = _acc_of(lambda a: ops.skinny_linear_rank_metrics(x, w, b, t, a, target_offset=0))
    logits = ops.skinny_linear(x, w, b)
    unfused = _acc_of(lambda a: ops.rank_metrics(logits, t, a, target_offset=0))
    assert torch.equal(fused, unfused), (fused.tolist(), unfused.tolist())
    # ... and evaluate_outputs' numbers for the same logits (target_rank + the host bookkeeping)
    want = metrics.evaluate_outputs([{"y_pred": [logits, None], "y_true": t}])
    _same(metrics.finalize(fused), want)
    # the engineered ties did take part: some target has equal scores on both sides
    rk = ops.target_rank(logits, t)
    assert bool((rk[:, 0] != rk[:, 1]).any())


def test_captured_graph_of_the_kernel_pair_replays_additively():
    G, K, V = 16, 448, 7857
    x, w, b, t = _tied_classifier(G, K, V, seed=5)
    work = torch.empty(ops.rank_metrics_work_bytes(G, V), dtype=torch.uint8, device=DEV)
    one = _acc_of(lambda a: ops.skinny_linear_rank_metrics(x, w, b, t, a, work=work))
    acc = metrics.new_accumulator(DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ops.skinny_linear_rank_metrics(x, w, b, t, acc, work=work)
    torch.cuda.current_stream().wait_stream(s)
    assert float(acc.abs().sum()) == 0.0                      # (capture does not run)
    n = 7
    for _ in range(n):
        g.replay()
    torch.cuda.synchronize()
    exact = one * n
    assert torch.equal(acc[:5], exact[:5])                    # counts: exact
    np.testing.assert_allclose(acc.cpu().numpy(), exact.cpu().numpy(), rtol=1e-14)


# ------------------------------------------------------------------------------------------------ EvalLoop
def _eval_dataset(uni, n=300, seed=61):
    from mobgt_amd import synth
    rng = np.random.RandomState(seed)
    lens = list(np.clip(rng.lognormal(2.0, 0.9, n).astype(int), 2, 120))
    trajs = synth.make_batch_of_trajectories(seed=seed, G=n, P=uni.P, n_user=uni.n_user, cat_of_poi=uni.cat_of_poi, n_nodes=lens)
    trajs[16 + 7]["target"] = np.array([1], dtype=np.int64)    # y == 1 mid-batch: get_acc's stop (shifted target 0)
    return trajs


def _eager_eval(model, coll, data, batches):
    """test_step + evaluate_outputs over the loop's batches, collated at the loop's bucket padding."""
    outs = []
    model.eval()
    with torch.no_grad():
        for ids in batches:
            trajs = [data[i] for i in ids if len(data[i]["node_name"]) <= coll.max_node]
            if not trajs:
                continue
            b = coll(trajs, n_pad=bucket_nodes(max(len(t["node_name"]) for t in trajs)))
            out = model.test_step(b)
            outs.append({"y_pred": [out["y_pred"][0].detach().clone(), None], "y_true": out["y_true"].clone()})
    r = metrics.evaluate_outputs(outs)
    r["n"] = sum(len(o["y_true"]) for o in outs)
    return r


@pytest.fixture(scope="module", params=["bf16", "f32"])
def fsq_eval(request):
    uni, model, coll = workloads.build("fsq", DEV, seed=1, P=1500, dtype=request.param, gemm_dtype=request.param,
                                       model_overrides=dict(n_layers=2))
    return uni, model, coll, _eval_dataset(uni)


def test_eval_loop_equals_eager_test_step_exactly(fsq_eval):
    uni, model, coll, data = fsq_eval
    loop = EvalLoop(model, coll, data, batch_size=16, use_graph=True)
    batches = loop.batches()
    assert [i for b in batches for i in b] == list(range(len(data))) and len(batches[-1]) == len(data) % 16
    want = _eager_eval(model, coll, data, batches)
    got = loop.run()
    assert got["n"] == want["n"] == len(data)
    _same(got, want)
    assert len({k[:2] for k in loop.graphs}) >= 3                # several buckets, and the final partial batch's G
    assert any(k[0] == len(data) % 16 for k in loop.graphs)
    assert loop.run() == got                                    # replayed graphs: the same numbers again
    eager = EvalLoop(model, coll, data, batch_size=16, use_graph=False).run()
    assert eager == got
    assert not model.training                                   # (the mode it was in before run())


def _trainer_state(ts):
    if ts is None:
        return []
    torch.cuda.synchronize()
    parts = [ts.flat_params.tensor, ts.exp_avg, ts.exp_avg_sq, ts.seed_dev, ts.lr_dev]
    if ts.shadow_flat is not None:
        parts.append(ts.shadow_flat)
    return [t.detach().clone() for t in parts]


def test_eval_between_epochs_sees_fresh_weights_and_leaves_training_alone():
    """Two identically built models train two epochs each; one is evaluated before, between and after.  Exactly: every piece of
    trainer state an evaluation could touch is bit-identical across each evaluation (_trainer_state), and run() itself raises on
    parked work left behind (ops.step_state_leftovers).  The two runs' losses can only agree to the run-to-run spread of training
    (tests/test_gpu_loop.py: f32 atomics in the backward pass in front of bf16 rounding points, rtol 2e-3).  The evaluation after
    epoch 1 equals an eager evaluation of the weights at that point."""
    runs = []
    for with_eval in (True, False):
        uni, model, coll = workloads.build("fsq", DEV, seed=1, model_overrides=dict(n_layers=2, peak_lr=2e-4, warmup_updates=2,
                                                                                  tot_updates=100))
        train = [t for trajs in workloads.make_pool("fsq", 6, 16, uni, seed0=7000) for t in trajs]
        test = _eval_dataset(uni, n=80, seed=62)
        loop = EpochLoop(model, coll, train, batch_size=16, seed=3, use_graph=True)
        ev = EvalLoop(model, coll, test, batch_size=16) if with_eval else None
        seq, evals = [], []

        def evaluate():
            # deterministic half: everything the trainer's next replay reads that an evaluation could touch -- fp32 weights,
            # both Adam moments, the bf16 shadows the optimizer keeps, the step / dropout counter -- is bit for bit unchanged
            before = _trainer_state(loop.ts)
            evals.append(ev.run())
            after = _trainer_state(loop.ts)
            assert len(before) == len(after) and all(torch.equal(x, y) for x, y in zip(before, after))
            assert model.training

        for epoch in (0, 1):
            if ev is not None:
                evaluate()
            loop.run_epoch(epoch, on_step=lambda k, l: seq.append(float(l.item())))
        if ev is not None:
            evaluate()
            evals.append(_eager_eval(model, coll, test, ev.batches()))
            model.train()
        runs.append((seq, evals))
    (a, evals), (b, _) = runs
    assert len(a) == len(b) == 12
    np.testing.assert_allclose(a, b, rtol=2e-3)
    before, mid, after, eager = evals
    _same(after, eager)
    assert (before["mrr"], before["acc@20"]) != (after["mrr"], after["acc@20"])
    assert (mid["mrr"], mid["acc@20"]) != (after["mrr"], after["acc@20"])


def test_toyotagraph_ranks_log_softmax_against_unshifted_y():
    """The toyotagraph branch (its constructor as in golden G11: 996 user rows, the log_softmax POI head)."""
    uni, model, coll = workloads.build("fsq", DEV, seed=2, P=1500, dtype="f32", gemm_dtype="f32",
                                       model_overrides=dict(n_layers=2, dataset_name="toyotagraph"))
    data = _eval_dataset(uni, n=40, seed=63)
    for t in data:
        t["user"] = t["user"] % model.user_embed_model.user_embedding.num_embeddings
    loop = EvalLoop(model, coll, data, batch_size=16)
    got = loop.run()
    # reference bookkeeping (model_fqandtoyo.py:1484-1495: toyotagraph keeps y) from the eager forward's log-probabilities
    outs = []
    model.eval()
    with torch.no_grad():
        for ids in loop.batches():
            trajs = [data[i] for i in ids]
            bt = coll(trajs, n_pad=bucket_nodes(max(len(t["node_name"]) for t in trajs)))
            logp = model(bt)[0]
            outs.append({"y_pred": [logp.detach().clone(), None], "y_true": bt.y.long().view(-1).clone()})
    want = metrics.evaluate_outputs(outs)
    _same(got, want)
    assert got["n"] == len(data)


def test_two_rank_shards_pool_to_the_one_rank_result():
    """The eval sampler of rank r of 2 (no shuffle, wrap-around padding): the two ranks' accumulators added (what run()'s
    all-reduce does) equal ONE rank over the concatenation of both shards, batch for batch."""
    uni, model, coll = workloads.build("fsq", DEV, seed=1, P=1500, model_overrides=dict(n_layers=2))
    data = _eval_dataset(uni, n=63, seed=64)                     # 32 samples per rank (one wrap-around duplicate): 2 batches each
    accs = []
    for r in range(2):
        loop = EvalLoop(model, coll, data, batch_size=16, rank=r, world=2)
        assert [i for b in loop.batches() for i in b] == list(range(63))[r::2] + ([0] if r == 1 else [])
        loop.run()
        accs.append(loop.acc.clone())
    cat = [data[i] for r in range(2) for b in EvalLoop(model, coll, data, batch_size=16, rank=r, world=2).batches() for i in b]
    one = EvalLoop(model, coll, cat, batch_size=16)
    one.run()
    pooled = accs[0] + accs[1]
    assert torch.equal(pooled[:5], one.acc[:5])
    np.testing.assert_allclose(pooled.cpu().numpy(), one.acc.cpu().numpy(), rtol=1e-13)


def test_stock_variant_has_no_metric_step():
    uni, model, coll = workloads.build("fsq", DEV, seed=1, P=1500, variant="stock", model_overrides=dict(n_layers=1))
    with pytest.raises(NotImplementedError):
        model.eval().metric_step(None, metrics.new_accumulator(DEV))


def test_two_rank_gloo_evaluation_returns_the_pooled_result(tmp_path):
    """Two processes over gloo sharing cuda:0 (MOBGT_TEST_SHARED_GPU=1): EvalLoop takes rank / world from the process group,
    run() all-reduces the accumulator, and both ranks return the dict of ONE rank evaluating both shards back to back."""
    import json
    import socket
    import subprocess
    import sys
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY="0", MOBGT_TEST_SHARED_GPU="1")
        procs.append(subprocess.Popen([sys.executable, os.path.join(os.path.dirname(__file__), "_eval_ddp_worker.py"), str(tmp_path)],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(o.decode(errors="replace"))
    assert all(p.returncode == 0 for p in procs), "\n".join(o[-3000:] for o in outs)
    res = [json.load(open(os.path.join(tmp_path, f"rank{r}.json"))) for r in range(2)]
    assert res[0]["pooled"] == res[1]["pooled"]
    assert res[0]["pooled"]["n"] == 64                         # 63 samples + the sampler's wrap-around duplicate
    _same(res[0]["pooled"], res[0]["one_rank"])
    assert res[0]["pooled"]["n"] == res[0]["one_rank"]["n"]
