"""Top-k next-POI recommendations on the device: `ops.topk_rows` (csrc/topk.hip), `Graphormer.recommend_step` and
`train.PredictLoop`.

  * the kernel pair equals torch.sort(scores, dim=1, descending=True, stable=True)[:, :k] bit for bit -- ties, +-0.0, +-inf, NaN,
    a padded row stride -- and refuses a k it cannot take;
  * replayed in a captured graph it equals the eager call;
  * a target is in the top k exactly when the metrics count it a hit at k (ops.target_rank, EvalLoop's ACC@k);
  * on real Gowalla data (golden G8) the f32 model recommends the reference logits' own ranking wherever that ranking is not
    within the parity tolerance of a tie;
  * label spaces: toyotagraph returns unshifted POI ids ranked by log_softmax, the other datasets column + 1;
  * PredictLoop: graphs equal eager, a second run captures nothing, new weights are seen, dropped trajectories read -1 / -inf.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mobgt_amd import _lib, ops, workloads                                  # noqa: E402
from mobgt_amd.data import bucket_nodes                                     # noqa: E402
from mobgt_amd.train import EvalLoop, PredictLoop                           # noqa: E402
from test_gpu_eval import _eval_dataset                                     # noqa: E402
from test_gpu_real import DeviceCollator, g8, real_model, real_trajs        # noqa: E402,F401  (g8, real_model: fixtures)

DEV = "cuda"
SPECIAL = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0, 3.0], np.float32)


def _want(scores, k, off=0):
    """the contract, on the host: the stable descending sort's first k (values as stored bits)"""
    v, i = torch.sort(scores.cpu(), dim=1, descending=True, stable=True)
    return i[:, :k] + off, v[:, :k].contiguous().view(torch.int32)


def _check(scores, k, off=0):
    ids, vals = ops.topk_rows(scores, k, col_offset=off)
    wi, wv = _want(scores, k, off)
    assert torch.equal(ids.cpu(), wi)
    assert torch.equal(vals.cpu().view(torch.int32), wv)


def _inputs(G, V, seed):
    rng = np.random.default_rng(seed)
    yield "random", rng.standard_normal((G, V)).astype(np.float32)
    yield "quantised", rng.integers(-3, 4, (G, V)).astype(np.float32) * 0.5               # a handful of values: heavy ties
    yield "equal", np.full((G, V), -1.25, np.float32)
    x = rng.choice(SPECIAL, (G, V))
    yield "special", x
    x = rng.standard_normal((G, V)).astype(np.float32)
    x[:, rng.integers(0, V, 1 + V // 50)] = np.float32(np.nan)
    x[:, rng.integers(0, V, 1 + V // 50)] = np.float32(-0.0)
    x[:, rng.integers(0, V, 1 + V // 50)] = np.float32(0.0)
    x[:, rng.integers(0, V, 1 + V // 50)] = np.float32(np.inf)
    yield "sprinkled", x


@pytest.mark.parametrize("V,k", [(V if V else k, k) for V in (0, 63, 64, 65, 3680, 7857, 100001) for k in (1, 5, 10, 20, 64)
                                 if (V if V else k) >= k])                        # (V = 0: V = k; k > V is refused, below)
def test_topk_kernel_is_the_stable_sort_bit_for_bit(V, k):
    for G in (1, 3, 16, 17):
        for kind, x in _inputs(G, V, seed=G * 7919 + V + k):
            s = torch.from_numpy(x).to(DEV)
            try:
                _check(s, k, off=1)
            except AssertionError as e:
                raise AssertionError(f"G={G} V={V} k={k} {kind}") from e
        # a padded row stride; the padding holds scores that would win if they were read
        pad = torch.full((G, V + 37), float("inf"), device=DEV)
        pad[:, :V] = torch.from_numpy(next(_inputs(G, V, seed=V + k))[1]).to(DEV)
        view = pad[:, :V]
        assert view.stride(0) == V + 37
        _check(view, k)


def test_topk_kernel_refuses_bad_arguments():
    s = torch.randn(3, 100, device=DEV)
    work = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    ids = torch.empty(3, 65, dtype=torch.int64, device=DEV)
    vals = torch.empty(3, 65, device=DEV)
    L = _lib.lib()
    for G, V, k, ld in ((3, 100, 0, 100), (3, 100, 65, 100), (3, 10, 11, 100), (3, 100, 5, 99), (0, 100, 5, 100)):
        rc = L.mobgt_topk_rows(ops._p(s), ld, G, V, k, 0, ops._p(ids), ops._p(vals), ops._p(work), ops._stream())
        assert rc == -1, (G, V, k, ld, rc)
    with pytest.raises(_lib.MobgtError):
        ops.topk_rows(s, 65)
    for k in (0, 101):
        with pytest.raises(ValueError):
            ops.topk_rows(s, k)


def test_topk_pair_replayed_in_a_captured_graph_equals_eager():
    G, V, k = 16, 7857, 20
    src = torch.empty(G, V, device=DEV)
    out = (torch.empty(G, k, dtype=torch.int64, device=DEV), torch.empty(G, k, device=DEV))
    work = torch.empty(ops.topk_work_bytes(G, V, k), dtype=torch.uint8, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ops.topk_rows(src, k, col_offset=1, work=work, out=out)
    torch.cuda.current_stream().wait_stream(s)
    for seed, (kind, x) in enumerate(_inputs(G, V, seed=3)):
        src.copy_(torch.from_numpy(x))
        g.replay()
        ei, ev = ops.topk_rows(src, k, col_offset=1)
        torch.cuda.synchronize()
        assert torch.equal(out[0], ei), kind
        assert torch.equal(out[1].view(torch.int32), ev.view(torch.int32)), kind


def test_top_k_membership_is_the_metrics_hit():
    """target in ids[:, :k]  <=>  target_rank's ACC position < k, with ties on both sides of the target."""
    rng = np.random.default_rng(11)
    for V in (3680, 7857, 100001):
        G = 16
        x = rng.integers(-40, 40, (G, V)).astype(np.float32) * 0.25
        t = rng.integers(1, V, G)
        for g in range(G):
            x[g, t[g]] = np.sort(x[g])[-1 - g]          # targets spread over the top ranks, tied with their neighbours
        s, tt = torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV)
        both = ops.target_rank(s, tt)
        rank = both[:, 0]
        assert bool((both[:, 0] != both[:, 1]).any())           # (equal scores on both sides of some target)
        for k in (1, 5, 10, 20):
            ids, _ = ops.topk_rows(s, k)
            hit = (ids == tt[:, None]).any(1)
            assert torch.equal(hit, rank < k), (V, k)


# ------------------------------------------------------------------------------------------------ the model
def test_recommendations_on_real_gowalla_follow_the_reference_logits_g8(g8, real_model):
    """At every position where the reference's own sorted logits are further from both neighbours than the f32 parity tolerance
    (2e-4 absolute + 2e-4 relative per logit, tests/test_gpu_real.py), the model recommends the reference's POI (column + 1)."""
    z, _, table = g8
    coll = DeviceCollator(DEV, bin_table=table, multi_hop_max_dist=20, rel_pos_max=1024)
    k = 20
    checked = total = 0
    for tag in ("a", "b"):
        b = coll(real_trajs(z, tag))
        G = b.x.shape[0]
        ids = torch.empty(G, k, dtype=torch.int64, device=DEV)
        vals = torch.empty(G, k, device=DEV)
        real_model.recommend_step(b, ids, vals)
        ref = torch.from_numpy(z[f"{tag}/logits"]).float()
        rv, ri = torch.sort(ref, dim=1, descending=True, stable=True)
        rv, ri = rv[:, :k + 1].numpy(), ri[:, :k].numpy() + 1
        got = ids.cpu().numpy()
        tol = 2 * (2e-4 + 2e-4 * np.abs(rv))
        for g in range(G):
            for p in range(k):
                total += 1
                lo = rv[g, p] - rv[g, p + 1] > max(tol[g, p], tol[g, p + 1])
                hi = p == 0 or rv[g, p - 1] - rv[g, p] > max(tol[g, p - 1], tol[g, p])
                if lo and hi:
                    checked += 1
                    assert got[g, p] == ri[g, p], (tag, g, p, got[g], ri[g])
        np.testing.assert_allclose(vals.cpu().numpy(), rv[:, :k], rtol=2e-4, atol=2e-4)
    assert checked >= total // 2, (checked, total)




@pytest.mark.parametrize("dataset", ["toyotagraph", "gowalla_nevda"])
def test_label_space_and_scores_of_recommend_step(dataset):
    uni, model, coll = workloads.build("fsq", DEV, seed=2, P=1500, dtype="f32", gemm_dtype="f32",
                                       model_overrides=dict(n_layers=2, dataset_name=dataset))
    model.eval()
    data = _eval_dataset(uni, n=40, seed=71)[:12]
    for t in data:
        t["user"] = t["user"] % model.user_embed_model.user_embedding.num_embeddings     # (toyotagraph's smaller user table)
    b = coll(data, n_pad=bucket_nodes(max(len(t["node_name"]) for t in data)))
    G, k = b.x.shape[0], 10
    ids = torch.empty(G, k, dtype=torch.int64, device=DEV)
    vals = torch.empty(G, k, device=DEV)
    model.recommend_step(b, ids, vals)
    with torch.no_grad():
        scores = model(b)[0]                             # toyotagraph: log_softmax(logits); otherwise the logits
    if dataset == "toyotagraph":
        assert torch.allclose(scores.exp().sum(1), torch.ones(G, device=DEV), atol=1e-4)
    wi, wv = _want(scores, k, off=0 if dataset == "toyotagraph" else 1)
    assert torch.equal(ids.cpu(), wi)
    assert torch.equal(vals.cpu().view(torch.int32), wv)
    with pytest.raises(RuntimeError):
        model.train().recommend_step(b, ids, vals)


def test_stock_variant_has_no_recommend_step():
    uni, model, coll = workloads.build("fsq", DEV, seed=1, P=1500, variant="stock", model_overrides=dict(n_layers=1))
    ids = torch.empty(1, 5, dtype=torch.int64, device=DEV)
    with pytest.raises(NotImplementedError):
        model.eval().recommend_step(None, ids, torch.empty(1, 5, device=DEV))


# ------------------------------------------------------------------------------------------------ PredictLoop
@pytest.fixture(scope="module")
def fsq_predict():
    uni, model, coll = workloads.build("fsq", DEV, seed=1, P=1500, model_overrides=dict(n_layers=2))
    return uni, model, coll, _eval_dataset(uni)


def test_predict_loop_hits_are_eval_loop_acc(fsq_predict):
    """Hits of PredictLoop's lists, counted with get_acc's stop at the first shifted target 0 in a batch, equal EvalLoop's
    ACC@k x n on the same split, for k = 1, 5, 10, 20."""
    uni, model, coll, data = fsq_predict
    ev = EvalLoop(model, coll, data, batch_size=16)
    r = ev.run()
    loop = PredictLoop(model, coll, data, k=20, batch_size=16)
    idx, ids, vals = loop.run()
    assert idx.tolist() == [i for b in loop.batches() for i in b]
    ids = ids.cpu().numpy()
    y = np.array([int(t["target"][0]) for t in data])
    hits = {k: 0 for k in (1, 5, 10, 20)}
    row = 0
    for b in loop.batches():
        stopped = False
        for i in b:
            stopped = stopped or y[i] == 1
            if not stopped:
                for k in hits:
                    hits[k] += int(y[i] in ids[row, :k])
            row += 1
    assert any(y[i] == 1 for i in range(len(data)))          # (the stop rule takes part)
    for k, h in hits.items():
        assert h == round(r[f"acc@{k}"] * r["n"]), (k, h, r[f"acc@{k}"] * r["n"])
    assert hits[20] > hits[1]


def test_predict_loop_graphs_equal_eager_and_see_new_weights(fsq_predict):
    uni, model, coll, data = fsq_predict
    loop = PredictLoop(model, coll, data, k=10, batch_size=16, use_graph=True)
    a = loop.run()
    n_graphs = loop.captures
    assert n_graphs >= 3 and len(loop.graphs) == n_graphs
    b = loop.run()
    assert loop.captures == n_graphs                           # replayed, nothing captured again
    eager = PredictLoop(model, coll, data, k=10, batch_size=16, use_graph=False).run()
    for x, y, z in zip(a, b, eager):
        assert torch.equal(x, y) and torch.equal(x, z)
    assert bool((a[1] >= 1).all()) and bool((a[1] <= model.out_proj.out_features).all())
    # new weights between runs: a column lifted far above the rest is every sample's first recommendation
    c = 123
    bias = model.out_proj.bias
    keep = bias.detach().clone()
    try:
        with torch.no_grad():
            bias[c] += 1.0e4
        _, ids, _ = loop.run()
        assert bool((ids[:, 0] == c + 1).all())
        assert loop.captures == n_graphs
    finally:
        with torch.no_grad():
            bias.copy_(keep)
    assert all(torch.equal(x, y) for x, y in zip(loop.run(), a))


def test_predict_loop_marks_dropped_trajectories(fsq_predict):
    uni, model, coll, data = fsq_predict
    data = data[:48]
    lens = np.array([len(t["node_name"]) for t in data])
    cut = int(np.sort(lens)[-3])                               # the longest few trajectories are over max_node
    saved = coll.max_node
    coll.max_node = cut - 1
    try:
        idx, ids, vals = PredictLoop(model, coll, data, k=5, batch_size=16).run()
    finally:
        coll.max_node = saved
    drop = torch.from_numpy(lens[idx.cpu().numpy()] >= cut).to(DEV)
    assert 1 <= int(drop.sum()) < len(data)
    assert bool((ids[drop] == -1).all()) and bool(torch.isneginf(vals[drop]).all())
    assert bool((ids[~drop] >= 1).all()) and bool(torch.isfinite(vals[~drop]).all())
