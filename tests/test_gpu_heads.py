"""The fq model's explicit heads (`Graphormer.encode`, `poi_logits`, `poi_scores`) and `restriction.Restriction`:

  * every step kind makes the library calls it made when `forward` ended in a head with five hidden modes, in that order
    (the expected lists are literals recorded from that code);
  * no step leaves an autograd graph or a mode on the module: a train-mode forward no longer stands in the way of a TrainStep;
  * one label offset: restricted metric_step hits are membership in recommend_step's lists for toyotagraph (0) and gowalla (1),
    through the keywords and through a prebuilt Restriction, with identical accumulators.

Models: one encoder layer, f32, P = 1500 POIs (a classifier wide enough for the skinny kernels: V >= 1024, K = 320) or P = 600
(not wide enough); G = 6 graphs of 2 .. 12 nodes.
"""
import functools
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mobgt_amd import _lib, metrics, ops, synth, workloads                  # noqa: E402
from mobgt_amd.data import bucket_nodes                                      # noqa: E402

DEV = "cuda"
NODES = (2, 12, 5, 7, 3, 9)
KEPT = ("_enc_out", "_bias_pack", "_cuts")                                   # what train.TrainStep reads off the module
GONE = ("_loss_in_head", "_poi_logits_only", "_metrics_in_head", "_recommend_in_head", "_head_loss", "_toyota_logits")


def _build(dataset, P, bad_target=False):
    """(universe, model, batch, coords [P + 1, 2] degrees); bad_target: row 2's y is past the classifier's last class"""
    uni, model, coll = workloads.build("fsq", DEV, seed=2, P=P, dtype="f32", gemm_dtype="f32",
                                       model_overrides=dict(n_layers=1, dataset_name=dataset))
    data = synth.make_batch_of_trajectories(seed=71, G=len(NODES), P=uni.P, n_user=uni.n_user, cat_of_poi=uni.cat_of_poi,
                                            n_nodes=list(NODES))
    for t in data:
        t["user"] = t["user"] % model.user_embed_model.user_embedding.num_embeddings     # (toyotagraph's smaller user table)
    for i in (1, 4):                                                         # revisits: the target is a POI of the trajectory
        data[i]["target"] = np.array([int(data[i]["node_name"][0])], dtype=np.int64)
    if bad_target:
        data[2]["target"] = np.array([model.out_proj.out_features + 3], dtype=np.int64)
    b = coll(data, n_pad=bucket_nodes(max(NODES)))
    c = np.zeros((uni.P + 1, 2))
    c[1:] = uni.poi_table[:, 2:4]
    return uni, model, b, torch.from_numpy(c)


_model = functools.lru_cache(maxsize=None)(_build)                           # (shared: its batch is read only)


def _restriction_args(dataset, P, r_km=3.0):
    """exclude_visited + allow + split_revisits + near, as metric_step's keywords"""
    uni, model, b, c = _model(dataset, P)
    G, V = b.x.shape[0], model.out_proj.out_features
    off = 0 if dataset == "toyotagraph" else 1
    rng = np.random.default_rng(1)
    cand = torch.from_numpy(rng.choice(np.arange(1, uni.P + 1), uni.P // 2, replace=False))
    cand = torch.cat([cand, b.y.reshape(-1)[:4].cpu()])                      # (some targets among the candidates)
    near = (ops.pack_positions(c, V, off).to(DEV), ops.chord2_of_km(r_km), "any",
            torch.zeros(G, (V + 31) // 32, dtype=torch.int32, device=DEV))
    return dict(exclude_visited=True, allow=ops.pack_allow(cand, V, offset=off).to(DEV), split_revisits=True, near=near)


def _train(dataset, P):
    _, model, b, _ = _model(dataset, P)
    model.train()
    for p in model.parameters():
        p.grad = None
    model.training_step(b).backward()


def _forward_train(dataset, P):
    _, model, b, _ = _model(dataset, P)
    model.train()
    model(b)


def _metric(dataset, P, restricted):
    _, model, b, _ = _model(dataset, P)
    model.eval()
    if restricted:
        model.metric_step(b, metrics.new_restricted_accumulator(DEV, True), **_restriction_args(dataset, P))
    else:
        model.metric_step(b, metrics.new_accumulator(DEV))


def _recommend(dataset, P, near):
    _, model, b, _ = _model(dataset, P)
    model.eval()
    G = b.x.shape[0]
    ids, vals = torch.empty(G, 20, dtype=torch.int64, device=DEV), torch.empty(G, 20, device=DEV)
    model.recommend_step(b, ids, vals, **(dict(near=_restriction_args(dataset, P)["near"]) if near else {}))


SCENARIOS = {                                                                # name -> (step, dataset, P, its argument)
    "training_step, wide classifier": (_train, "foursquaregraph", 1500),
    "training_step, narrow classifier": (_train, "foursquaregraph", 600),
    "training_step, toyotagraph": (_train, "toyotagraph", 1500),
    "forward in train mode": (_forward_train, "foursquaregraph", 1500),
    "forward in train mode, toyotagraph": (_forward_train, "toyotagraph", 1500),
    "metric_step": (_metric, "foursquaregraph", 1500, False),
    "metric_step, restricted": (_metric, "foursquaregraph", 1500, True),
    "recommend_step": (_recommend, "foursquaregraph", 1500, False),
    "recommend_step, near": (_recommend, "foursquaregraph", 1500, True),
}


def run_scenario(name):
    step, *args = SCENARIOS[name]
    step(*args)
    return _model(*args[:2])[1]


def record_calls(name):
    """The names asked of the kernel library while the scenario runs, in order (it has run once before: lazy initialisations
    are over)"""
    run_scenario(name)
    torch.cuda.synchronize()
    real, seen = _lib.lib, []

    class _Spy:
        def __getattr__(self, entry):
            seen.append(entry)
            return getattr(real(), entry)

    _lib.lib = lambda: _Spy()
    try:
        run_scenario(name)
    finally:
        _lib.lib = real
    torch.cuda.synchronize()
    return seen


# The library calls of each scenario at the commit before `encode` and the explicit heads (forward with its five head modes),
# recorded there with record_calls on an MI355X: the encoder up to the heads' input, a head, and for a training step the backward.
ENCODE = ["mobgt_small_gcn_fwd_pack", "mobgt_build_bias", "mobgt_bias_act_fwd_t", "mobgt_small_gemm_f32",
          "mobgt_bias_act_fwd_t", "mobgt_small_gemm_f32", "mobgt_embed_gather_multi", "mobgt_small_gemm_f32_act",
          "mobgt_small_gemm_f32_act", "mobgt_assemble_tokens_fwd", "mobgt_attn_bias_fwd", "mobgt_dropout_add_ln_fwd",
          "mobgt_gelu_fwd", "mobgt_dropout_add_ln_fwd", "mobgt_head_chain_fwd"]
BACKWARD = ["mobgt_head_chain_bwd", "mobgt_colsum", "mobgt_dropout_add_ln_bwd", "mobgt_gelu_bwd_colsum",
            "mobgt_dropout_add_ln_bwd", "mobgt_attn_bias_bwd", "mobgt_colsum", "mobgt_assemble_tokens_bwd", "mobgt_colsum",
            "mobgt_colsum", "mobgt_embed_gather_multi", "mobgt_small_gcn_bwd_bias", "mobgt_colsum", "mobgt_bias_act_bwd",
            "mobgt_small_gemm_f32", "mobgt_bias_act_bwd", "mobgt_build_bias_bwd", "mobgt_hop_table_bwd"]
EXPECTED = {
    "training_step, wide classifier": ENCODE + ["mobgt_skinny_linear_gtl", "mobgt_skinny_linear_bwd_both"] + BACKWARD,
    "training_step, narrow classifier": ENCODE + ["mobgt_gradient_tail_loss"] + BACKWARD,
    "training_step, toyotagraph": ENCODE + ["mobgt_skinny_linear_fwd_mfma", "mobgt_gradient_tail_loss", "mobgt_cross_entropy",
                                            "mobgt_skinny_linear_bwd_both"] + BACKWARD,
    "forward in train mode": ENCODE + ["mobgt_skinny_linear_fwd_mfma"],
    "forward in train mode, toyotagraph": ENCODE + ["mobgt_skinny_linear_fwd_mfma"],
    "metric_step": ENCODE + ["mobgt_skinny_linear_fwd_mfma", "mobgt_rank_metrics_work_bytes", "mobgt_rank_metrics"],
    "metric_step, restricted": ENCODE + ["mobgt_skinny_linear_fwd_mfma", "mobgt_near_words", "mobgt_rank_metrics_masked_work_bytes",
                                         "mobgt_rank_metrics_masked_rows"],
    "recommend_step": ENCODE + ["mobgt_skinny_linear_fwd_mfma", "mobgt_topk_work_bytes", "mobgt_topk_rows"],
    "recommend_step, near": ENCODE + ["mobgt_skinny_linear_fwd_mfma", "mobgt_near_words", "mobgt_topk_work_bytes",
                                      "mobgt_topk_rows_masked_rows"],
}


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_entry_points_in_order(name):
    assert record_calls(name) == EXPECTED[name]


def _holds_graph(v):
    if isinstance(v, torch.Tensor):
        return v.grad_fn is not None
    if isinstance(v, (tuple, list)):
        return any(_holds_graph(x) for x in v)
    if isinstance(v, dict):
        return any(_holds_graph(x) for x in v.values())
    return False


def _check_nothing_left(model, tag):
    left = [k for k, v in model.__dict__.items() if k not in KEPT and _holds_graph(v)]
    assert not left, (tag, left)
    assert not [k for k in GONE if hasattr(model, k)], tag


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_a_step_leaves_nothing_on_the_module(name):
    _check_nothing_left(run_scenario(name), name)


def test_train_mode_forward_then_a_trainer():
    """model(batch) in train mode used to leave the toyotagraph logits, with their graph, on the module; only training_step took
    them off again.  Now a TrainStep can be prepared right behind it."""
    from mobgt_amd.train import TrainStep
    _, model, b, _ = _build("toyotagraph", 1500)                             # (a model of its own: the trainer re-homes its weights)
    model.train()
    out = model(b)
    assert out[0].grad_fn is not None and out[1].grad_fn is not None
    del out
    gc.collect()
    _check_nothing_left(model, "forward")
    ts = TrainStep(model, [b], use_graph=True, seed=1)
    ts.prepare()
    loss = ts.step(0)
    assert bool(torch.isfinite(loss))
    _check_nothing_left(model, "step")


def test_encode_raising_inside_metric_step_leaves_the_model_as_it_was():
    """validate_batch refuses an out-of-range index on the host, before any launch"""
    _, model, b, _ = _model("foursquaregraph", 1500)
    bad = _build("foursquaregraph", 1500, bad_target=True)[2]
    model.eval()
    acc = metrics.new_accumulator(DEV)
    model.metric_step(b, acc)
    before, counted = dict(model.__dict__), acc.clone()
    G = b.x.shape[0]
    ids, vals = torch.empty(G, 20, dtype=torch.int64, device=DEV), torch.empty(G, 20, device=DEV)
    for step in (lambda: model.metric_step(bad, acc),
                 lambda: model.metric_step(bad, metrics.new_restricted_accumulator(DEV, True), exclude_visited=True,
                                           split_revisits=True),
                 lambda: model.recommend_step(bad, ids, vals, exclude_visited=True)):
        with pytest.raises(IndexError, match="batch.y"):
            step()
        assert not model.training and torch.is_grad_enabled()
        after = model.__dict__
        assert set(after) == set(before) and all(after[k] is before[k] for k in before)
        _check_nothing_left(model, "raised")
    assert torch.equal(acc, counted)
    model.train()
    with pytest.raises(RuntimeError, match="training mode"):
        model.metric_step(b, acc)
    assert model.training and torch.equal(acc, counted)
    _check_nothing_left(model, "training mode")


def _topk_hits(ids, y, target_offset):
    """hit@1/5/10/20 counts of ids [G, 20] (label space) against y, with get_acc's stop at the first shifted target 0"""
    hits = np.zeros(4)
    for g in range(ids.shape[0]):
        if int(y[g]) + target_offset == 0:
            break
        row = ids[g].tolist()
        for q, k in enumerate((1, 5, 10, 20)):
            hits[q] += int(y[g]) in row[:k]
    return hits


@pytest.mark.parametrize("dataset", ["toyotagraph", "gowalla_nevda"])
def test_one_label_offset_through_keywords_and_a_prebuilt_restriction(dataset):
    """test_gpu_eval_masked.py::test_restricted_metric_step_label_space, also through a prebuilt Restriction: hits are membership
    in recommend_step's lists in both label spaces, and the two ways give the same accumulator and the same lists bit for bit"""
    from mobgt_amd.restriction import Restriction
    uni, model, b, c = _model(dataset, 1500)
    model.eval()
    off = 0 if dataset == "toyotagraph" else 1
    assert model.label_offset == off
    G, V = b.x.shape[0], model.out_proj.out_features
    y = b.y.reshape(-1).cpu()
    full = {k: v for k, v in _restriction_args(dataset, 1500).items() if k != "split_revisits"}
    with torch.no_grad():
        scores = model(b)[0].float()
    reached = 0
    for kw in (dict(exclude_visited=True), dict(allow=full["allow"]), dict(exclude_visited=True, allow=full["allow"]), full):
        r = Restriction(model.label_offset, split_revisits=True, **kw)
        assert r.active and r.label_offset == off
        got = []
        for metric_kw, recommend_kw in ((dict(kw, split_revisits=True), kw), (dict(restriction=r), dict(restriction=r))):
            acc = metrics.new_restricted_accumulator(DEV, True)
            ids, vals = torch.empty(G, 20, dtype=torch.int64, device=DEV), torch.empty(G, 20, device=DEV)
            model.metric_step(b, acc, **metric_kw)
            model.recommend_step(b, ids, vals, **recommend_kw)
            got.append((acc.cpu(), ids.cpu(), vals.cpu().view(torch.int32)))
        a, ids, _ = got[0]
        assert all(torch.equal(u, v) for u, v in zip(*got)), (dataset, sorted(kw))
        assert np.array_equal(a[0, 1:5].numpy(), _topk_hits(ids, y, -off)), (dataset, sorted(kw))
        hist = Restriction.hist(b)
        want = metrics.restricted_sums(scores, b.y.reshape(-1), -off, r.allow_for(hist), hist, off, r.exclude_visited, True).cpu()
        assert torch.equal(a[:, [0, 1, 2, 3, 4, 10]], want[:, [0, 1, 2, 3, 4, 10]]), (dataset, sorted(kw))
        assert int(a[0, 0]) == G and int(a[2, 0]) >= 2                       # the revisits are split off
        if r.exclude_visited:
            assert int(a[2, 10]) == 0                                        # a visited target is never reachable
        reached += int(a[0, 10])
    assert reached > 0
    assert not Restriction(off).active
