"""Restricted and split evaluation on the device: `ops.rank_metrics_masked` (csrc/skinny.hip, mobgt_rank_metrics_masked),
`Graphormer.metric_step(exclude_visited=, allow=, split_revisits=)` and `train.EvalLoop(exclude_visited=, candidates=,
split_revisits=)`.

  * the kernel pair equals metrics.restricted_sums (itself checked against a plain restatement in tests/test_host_eval_masked.py):
    counts exact, DCG / MRR sums to 1e-12, over G 1 / 5 / 16 and V up to past the RM_MAXB * RM_CHUNK column cap, int32 and
    int64 hist with a padded row stride, ties on both sides of the target; unrestricted it is mobgt_rank_metrics bit for bit;
    replayed in a captured graph it adds as the eager call does; it refuses bad arguments;
  * model: a hit at k is exactly "y is in recommend_step's restricted top k", on real Gowalla data and in both label spaces;
  * loop: graphs equal an eager metric_step loop, hits equal PredictLoop's lists, a visited target is never reachable, and a
    default loop built after a restricted one gives its former result.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mobgt_amd import _lib, metrics, ops, workloads                         # noqa: E402
from mobgt_amd._lib import I32, I64                                          # noqa: E402
from mobgt_amd.data import bucket_nodes                                      # noqa: E402
from mobgt_amd.train import EvalLoop, PredictLoop                            # noqa: E402
from test_gpu_eval import _eval_dataset                                      # noqa: E402
from test_gpu_real import DeviceCollator, g8, real_model, real_trajs         # noqa: E402,F401  (g8, real_model: fixtures)

DEV = "cuda"
COUNTS = [0, 1, 2, 3, 4, 10]                                                 # n, hits, reachable: exact


def _case(rng, G, V, hist_dtype, n_hist=24, ld_extra=5):
    """scores (ties, some copied to both sides of the target), targets in label space offset 1 (revisits, new, out of range, a
    target-0 row), hist [G, n_hist] with padding, duplicates and ids outside [1, V] as a column slice of a wider tensor"""
    if V < 100:
        s = rng.integers(-3, 4, (G, V)).astype(np.float32) * 0.5
    else:
        s = rng.standard_normal((G, V)).astype(np.float32)
    y = rng.integers(1, V + 1, G)
    wide = rng.integers(-2, V + 4, (G, n_hist + ld_extra))
    wide[:, ::4] = 0
    wide[:, 3] = wide[:, 5]
    h = wide[:, :n_hist]
    y[::2] = np.where(h[::2, 1] >= 1, np.minimum(h[::2, 1], V), 1)       # revisits
    if G > 2:
        y[1] = V + 3                                                         # out of range
        y[G // 2] = 1                                                        # column 0: the batch's hits stop here
    for g in range(G):
        c = int(y[g]) - 1
        if 0 <= c < V and V > 2:
            for d in (-1, 1):                                                # ties on both sides of the target
                if 0 <= c + d < V and rng.random() < 0.7:
                    s[g, c + d] = s[g, c]
    wide_t = torch.from_numpy(wide).to(hist_dtype).to(DEV)
    return torch.from_numpy(s).to(DEV), torch.from_numpy(y).to(DEV), wide_t[:, :n_hist]


def _check(got, want, tag):
    got, want = got.cpu(), want.cpu()
    assert torch.equal(got[:, COUNTS], want[:, COUNTS]), (tag, got[:, COUNTS], want[:, COUNTS])
    assert torch.allclose(got, want, rtol=1e-12, atol=0), (tag, got, want)


@pytest.mark.parametrize("V", [1, 63, 2049, 7857, 100001, 300001])
def test_masked_rank_metrics_kernel_is_the_contract(V):
    rng = np.random.default_rng(V)
    for G in (1, 5, 16):
        for hist_dtype in (torch.int32, torch.int64):
            s, y, h = _case(rng, G, V, hist_dtype)
            assert h.stride(0) > h.shape[1]                                  # (ld_hist > n_hist_cols)
            allow = ops.pack_allow(torch.from_numpy(rng.random(V) < 0.6).to(DEV), V)
            for al, excl, split in ((None, False, False), (None, True, True), (allow, True, True), (allow, False, True),
                                    (allow, False, False), (None, False, True)):
                acc = metrics.new_restricted_accumulator(DEV, split)
                ops.rank_metrics_masked(s, y, acc, target_offset=-1, allow=al, hist=h, exclude_hist=excl, split=split)
                want = metrics.restricted_sums(s, y, -1, al, h, 1, excl, split)
                _check(acc, want, (G, V, hist_dtype, al is not None, excl, split))
                if split:
                    assert acc[1, 0] + acc[2, 0] == G


def test_unrestricted_masked_is_rank_metrics_bit_for_bit():
    rng = np.random.default_rng(2)
    for V in (63, 7857, 300001):
        for G in (1, 16):
            s = torch.from_numpy(rng.integers(-20, 20, (G, V)).astype(np.float32) * 0.25).to(DEV)
            y = torch.from_numpy(rng.integers(0, V, G)).to(DEV)
            if G > 4:
                y[3] = 0
            a = metrics.new_accumulator(DEV)
            ops.rank_metrics(s, y, a)
            b = metrics.new_restricted_accumulator(DEV)
            ops.rank_metrics_masked(s, y, b)
            assert torch.equal(b[0, :10], a), (V, G)
            assert int(b[0, 10]) == G


def test_masked_pair_replayed_in_a_captured_graph_adds_as_eager():
    rng = np.random.default_rng(7)
    G, V = 16, 7857
    s, y, h = _case(rng, G, V, torch.int64)
    allow = ops.pack_allow(torch.from_numpy(rng.random(V) < 0.5).to(DEV), V)
    work = torch.empty(ops.rank_metrics_masked_work_bytes(G, V), dtype=torch.uint8, device=DEV)
    eager = metrics.new_restricted_accumulator(DEV, True)
    for _ in range(3):
        ops.rank_metrics_masked(s, y, eager, -1, allow, h, exclude_hist=True, split=True, work=work)
    acc = metrics.new_restricted_accumulator(DEV, True)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        ops.rank_metrics_masked(s, y, acc, -1, allow, h, exclude_hist=True, split=True, work=work)
    torch.cuda.current_stream().wait_stream(st)
    acc.zero_()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(acc, eager)
    _check(eager / 3, metrics.restricted_sums(s, y, -1, allow, h, 1, True, True), "capture")


def test_masked_rank_metrics_refuses_bad_arguments():
    lib = _lib.lib()
    G, V = 4, 100
    s = torch.zeros(G, V, device=DEV)
    y = torch.ones(G, dtype=torch.int64, device=DEV)
    h = torch.ones(G, 8, dtype=torch.int64, device=DEV)
    acc = metrics.new_restricted_accumulator(DEV, True)
    work = torch.empty(ops.rank_metrics_masked_work_bytes(G, V), dtype=torch.uint8, device=DEV)
    p = ops._p

    def call(G=G, V=V, hist=h, dt=I64, ld=8, n=8, flags=3, sc=s, w=work):
        return lib.mobgt_rank_metrics_masked(p(sc), p(y), -1, G, V, None, p(hist), dt, ld, n, 1, flags, p(acc), p(w), ops._stream())

    assert call() == 0
    assert call(G=0) == _lib_err("EBADDIM") and call(G=70000) == _lib_err("EBADDIM")
    assert call(V=0) == _lib_err("EBADDIM") and call(V=1 << 31) == _lib_err("EBADDIM")
    assert call(flags=4) == _lib_err("EBADDIM") and call(flags=-1) == _lib_err("EBADDIM")
    assert call(ld=7) == _lib_err("EBADDIM") and call(n=-1) == _lib_err("EBADDIM")
    assert call(dt=7) == _lib_err("EDTYPE") and call(dt=I32, ld=16, n=16) == 0
    assert call(sc=None) == _lib_err("EBADDIM") and call(w=None) == _lib_err("EBADDIM")
    assert ops.rank_metrics_masked_work_bytes(0, V) == 0
    torch.cuda.synchronize()
    with pytest.raises(AssertionError):
        ops.rank_metrics_masked(s, y, metrics.new_restricted_accumulator(DEV), hist=h, split=True)     # acc of one slot
    with pytest.raises(AssertionError):
        ops.rank_metrics_masked(s, y, metrics.new_restricted_accumulator(DEV), allow=torch.zeros(2, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        ops.rank_metrics_masked(s, y, metrics.new_restricted_accumulator(DEV), exclude_hist=True)


def _lib_err(name):
    return {"EBADDIM": -1, "EALIGN": -2, "EDTYPE": -3}[name]


# ------------------------------------------------------------------------------------------------ the model
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


def test_restricted_metric_step_hits_are_recommend_step_lists_on_real_gowalla_g8(g8, real_model):
    z, _, table = g8
    coll = DeviceCollator(DEV, bin_table=table, multi_hop_max_dist=20, rel_pos_max=1024)
    V = real_model.out_proj.out_features
    rng = np.random.default_rng(4)
    cand = torch.from_numpy(rng.choice(np.arange(1, V + 1), V // 2, replace=False)).to(DEV)
    allow = ops.pack_allow(cand, V, offset=1)
    reached = 0
    for tag in ("a", "b"):
        b = coll(real_trajs(z, tag))
        G = b.x.shape[0]
        ids = torch.empty(G, 20, dtype=torch.int64, device=DEV)
        vals = torch.empty(G, 20, device=DEV)
        for excl, al in ((True, None), (True, allow), (False, allow)):
            acc = metrics.new_restricted_accumulator(DEV, True)
            real_model.metric_step(b, acc, exclude_visited=excl, allow=al, split_revisits=True)
            real_model.recommend_step(b, ids, vals, exclude_visited=excl, allow=al)
            a = acc.cpu()
            assert np.array_equal(a[0, 1:5].numpy(), _topk_hits(ids.cpu(), b.y.reshape(-1).cpu(), -1)), (tag, excl, al is not None)
            assert int(a[0, 0]) == G
            if excl:
                assert int(a[2, 10]) == 0
            reached += int(a[0, 10])
    assert reached > 0


@pytest.mark.parametrize("dataset", ["toyotagraph", "gowalla_nevda"])
def test_restricted_metric_step_label_space(dataset):
    uni, model, coll = workloads.build("fsq", DEV, seed=2, P=1500, dtype="f32", gemm_dtype="f32",
                                       model_overrides=dict(n_layers=2, dataset_name=dataset))
    model.eval()
    data = _eval_dataset(uni, n=40, seed=71)[:16]
    for t in data:
        t["user"] = t["user"] % model.user_embed_model.user_embedding.num_embeddings     # (toyotagraph's smaller user table)
    for i in (2, 5, 9):                                                      # revisits: the target is a POI of the trajectory
        data[i]["target"] = np.array([int(data[i]["node_name"][0])], dtype=np.int64)
    b = coll(data, n_pad=bucket_nodes(max(len(t["node_name"]) for t in data)))
    G, V = b.x.shape[0], model.out_proj.out_features
    off = 0 if dataset == "toyotagraph" else 1
    rng = np.random.default_rng(1)
    cand = torch.from_numpy(rng.choice(np.arange(off, V + off), V // 3, replace=False))
    cand = torch.cat([cand, b.y.reshape(-1)[:8].cpu()])                      # (some targets among the candidates)
    allow = ops.pack_allow(cand, V, offset=off).to(DEV)
    with torch.no_grad():
        scores = model(b)[0].float()
    ids = torch.empty(G, 20, dtype=torch.int64, device=DEV)
    vals = torch.empty(G, 20, device=DEV)
    x = b.x.reshape(G, -1)
    for excl, al in ((True, None), (False, allow), (True, allow)):
        acc = metrics.new_restricted_accumulator(DEV, True)
        model.metric_step(b, acc, exclude_visited=excl, allow=al, split_revisits=True)
        model.recommend_step(b, ids, vals, exclude_visited=excl, allow=al)
        a = acc.cpu()
        assert np.array_equal(a[0, 1:5].numpy(), _topk_hits(ids.cpu(), b.y.reshape(-1).cpu(), -off)), (dataset, excl)
        want = metrics.restricted_sums(scores, b.y.reshape(-1), -off, al, x, off, excl, True).cpu()
        assert torch.equal(a[:, COUNTS], want[:, COUNTS]), (dataset, excl)
        assert int(a[2, 0]) >= 3                                             # the revisits are split off
        if excl:
            assert int(a[2, 10]) == 0


# ------------------------------------------------------------------------------------------------ EvalLoop
@pytest.fixture(scope="module")
def fsq_eval():
    uni, model, coll = workloads.build("fsq", DEV, seed=1, P=1500, model_overrides=dict(n_layers=2))
    data = _eval_dataset(uni)
    for i in range(0, len(data), 5):                                         # every fifth target a revisit
        data[i]["target"] = np.array([int(data[i]["node_name"][-1])], dtype=np.int64)
    return uni, model, coll, data


def test_restricted_eval_loop(fsq_eval):
    uni, model, coll, data = fsq_eval
    plain_loop = EvalLoop(model, coll, data, batch_size=16)
    plain = plain_loop.run()
    loop = EvalLoop(model, coll, data, batch_size=16, exclude_visited=True, split_revisits=True)
    res = loop.run()
    assert loop.captures >= 3 and loop.run() == res and loop.captures == len(loop.graphs)
    # an eager metric_step loop over the same batches
    acc = metrics.new_restricted_accumulator(DEV, True)
    model.eval()
    for idx in loop.batches():
        trajs = [data[i] for i in idx if len(data[i]["node_name"]) <= coll.max_node]
        b = coll(trajs, n_pad=bucket_nodes(max(len(t["node_name"]) for t in trajs)))
        model.metric_step(b, acc, exclude_visited=True, split_revisits=True)
    want = metrics.finalize_restricted(acc)
    for part in (None, "new", "revisit"):
        r, w = (res, want) if part is None else (res[part], want[part])
        for k, v in w.items():
            if isinstance(v, dict):
                continue
            assert r[k] == pytest.approx(v, rel=1e-12, abs=0), (part, k)
    assert res["n"] == plain["n"] == res["new"]["n"] + res["revisit"]["n"] and res["revisit"]["n"] > 0
    assert res["revisit"]["reachable"] == 0 and res["reachable"] == res["new"]["reachable"] == res["new"]["n"]
    assert res["revisit"]["acc@20"] == 0.0 and res["revisit"]["mrr"] == 0.0
    # hits are PredictLoop's next-new-POI lists, with get_acc's per-batch stop at the first target 0
    idx, ids, _ = PredictLoop(model, coll, data, k=20, batch_size=16, exclude_visited=True).run()
    ids = ids.cpu()
    row = {int(i): r for r, i in enumerate(idx.cpu().tolist())}
    hits = np.zeros(4)
    for bidx in loop.batches():
        kept = [i for i in bidx if len(data[i]["node_name"]) <= coll.max_node]
        y = torch.tensor([int(data[i]["target"][0]) for i in kept])
        hits += _topk_hits(torch.stack([ids[row[i]] for i in kept]), y, -1)
    n = res["n"]
    for q, k in enumerate((1, 5, 10, 20)):
        assert round(res[f"acc@{k}"] * n) == hits[q], k
    # a default loop built after the restricted one: its former result, exactly
    assert EvalLoop(model, coll, data, batch_size=16).run() == plain
    assert set(plain) == set(metrics.finalize(metrics.new_accumulator("cpu")))


def test_restricted_evaluate_with_candidates(fsq_eval):
    uni, model, coll, data = fsq_eval
    V = model.out_proj.out_features
    data = data[:96]
    every = model.evaluate(data, coll, candidates=torch.arange(1, V + 1))
    plain = model.evaluate(data, coll)
    for k, v in plain.items():
        assert every[k] == pytest.approx(v, rel=1e-12, abs=0), k
    assert every["reachable"] == every["n"]
    cand = torch.tensor([int(data[i]["target"][0]) for i in range(0, 96, 2)])
    some = model.evaluate(data, coll, candidates=cand, split_revisits=True, use_graph=False)
    graphed = model.evaluate(data, coll, candidates=cand, split_revisits=True)
    assert some == graphed
    assert some["n"] == plain["n"] and 0 < some["reachable"] < some["n"]
    assert some["new"]["n"] + some["revisit"]["n"] == some["n"]
