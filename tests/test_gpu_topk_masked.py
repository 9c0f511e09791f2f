"""Restricted top-k recommendations on the device: `ops.topk_rows(..., allow=, exclude=)` (csrc/topk.hip,
mobgt_topk_rows_masked), `Graphormer.recommend_step(exclude_visited=, allow=)` and `train.PredictLoop(exclude_visited=,
candidates=)`.

  * the kernel pair equals the torch form of the contract (itself checked against a plain restatement in
    tests/test_host_topk_masked.py) bit for bit: allow densities 0 .. 1, exclusion lists with duplicates, padding and ids past V
    as int32 and int64, a padded row stride, ties and special values; with every column allowed it is mobgt_topk_rows' output;
    replayed in a captured graph it equals the eager call; it refuses what mobgt_topk_rows refuses;
  * on real Gowalla data (golden G8) exclude_visited lists no POI of the trajectory and is the unrestricted top 64 with the
    visited POIs removed; the exclusion works in recommend_step's label space for toyotagraph and the other datasets;
  * PredictLoop: graphs equal eager, a second run captures nothing, short candidate sets and dropped trajectories read -1 / -inf,
    the defaults still give the unrestricted lists.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mobgt_amd import _lib, ops, workloads                                  # noqa: E402
from mobgt_amd._lib import I64                                         # noqa: E402
from mobgt_amd.data import bucket_nodes                                     # noqa: E402
from mobgt_amd.train import PredictLoop                                     # noqa: E402
from test_gpu_eval import _eval_dataset                                     # noqa: E402
from test_gpu_real import DeviceCollator, g8, real_model, real_trajs        # noqa: E402,F401  (g8, real_model: fixtures)

DEV = "cuda"
SPECIAL = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0, 3.0], np.float32)


def _scores(rng, G, V, kind):
    if kind == "random":
        return rng.standard_normal((G, V)).astype(np.float32)
    if kind == "ties":
        return rng.integers(-3, 4, (G, V)).astype(np.float32) * 0.5
    return rng.choice(SPECIAL, (G, V))


def _exclude(rng, G, V, dt):
    """[G, n] ids in label space (offset 1): duplicates, padding 0, ids past V and below the offset"""
    n = int(min(V, 900)) + 8
    e = rng.integers(-2, V + 40, (G, n))
    e[:, ::5] = 0
    e[:, 1::7] = e[:, ::7][:, :e[:, 1::7].shape[1]]
    return torch.from_numpy(e).to(dt)


def _check(s, k, off, allow, exclude, tag):
    ids, vals = ops.topk_rows(s, k, col_offset=off, allow=allow, exclude=exclude)
    wi, wv = ops.topk_rows(s.cpu(), k, col_offset=off, allow=None if allow is None else allow.cpu(),
                           exclude=None if exclude is None else exclude.cpu())
    assert torch.equal(ids.cpu(), wi), tag
    assert torch.equal(vals.cpu().view(torch.int32), wv.contiguous().view(torch.int32)), tag


@pytest.mark.parametrize("V", [1, 63, 1024, 1025, 3680, 100001])
def test_masked_topk_kernel_is_the_contract_bit_for_bit(V):
    rng = np.random.default_rng(V)
    kinds = ("random", "ties", "special")
    for G in (1, 16):
        for k in (1, 10, 20, 64):
            if k > V:
                continue
            for j, density in enumerate((0.0, 0.001, 0.5, 0.99, 1.0, None)):
                kind = kinds[(j + k) % 3]
                s = torch.from_numpy(_scores(rng, G, V, kind)).to(DEV)
                allow = None if density is None else ops.pack_allow(torch.from_numpy(rng.random(V) < density), V).to(DEV)
                for dt in (torch.int32, torch.int64, None):
                    if allow is None and dt is None:
                        continue
                    exclude = None if dt is None else _exclude(rng, G, V, dt).to(DEV)
                    _check(s, k, 1, allow, exclude, (G, V, k, density, dt, kind))
        # a padded row stride whose padding would win if it were read; an exclusion list with a row stride of its own
        k = min(20, V)
        pad = torch.full((G, V + 37), float("inf"), device=DEV)
        pad[:, :V] = torch.from_numpy(_scores(rng, G, V, "special")).to(DEV)
        view = pad[:, :V]
        e = _exclude(rng, G, V, torch.int64)[:, :40]
        ex = torch.zeros(G, e.shape[1] + 24, dtype=torch.int64, device=DEV)
        ex[:, :e.shape[1]] = e.to(DEV)
        ex_view = ex[:, :e.shape[1]]
        assert view.stride(0) == V + 37 and ex_view.stride(0) == e.shape[1] + 24
        allow = ops.pack_allow(torch.from_numpy(rng.random(V) < 0.5), V).to(DEV)
        _check(view, k, 0, allow, ex_view, (G, V, "strided"))
        # the excluded POI in every row is the row's best score
        x = torch.from_numpy(_scores(rng, G, V, "random")).to(DEV)
        best = x.argmax(1)
        ids, _ = ops.topk_rows(x, k, col_offset=1, exclude=(best + 1)[:, None])
        assert not bool((ids == (best + 1)[:, None]).any())


def test_masked_topk_with_every_column_allowed_is_topk_rows():
    rng = np.random.default_rng(7)
    L = _lib.lib()
    for G, V, k in ((1, 63, 10), (16, 3680, 20), (16, 100001, 64), (3, 1025, 1)):
        for kind in ("random", "ties", "special"):
            s = torch.from_numpy(_scores(rng, G, V, kind)).to(DEV)
            allow = ops.pack_allow(torch.ones(V, dtype=torch.bool), V).to(DEV)
            a = ops.topk_rows(s, k, col_offset=1, allow=allow)
            b = ops.topk_rows(s, k, col_offset=1)
            # and the entry point with both restrictions NULL
            ids = torch.empty(G, k, dtype=torch.int64, device=DEV)
            vals = torch.empty(G, k, device=DEV)
            work = torch.empty(ops.topk_work_bytes(G, V, k), dtype=torch.uint8, device=DEV)
            ops.check(L.mobgt_topk_rows_masked(ops._p(s), V, G, V, k, 1, None, None, I64, 0, 0, 0, ops._p(ids), ops._p(vals),
                                               ops._p(work), ops._stream()), "mobgt_topk_rows_masked")
            for i, v in (a, (ids, vals)):
                assert torch.equal(i, b[0]), (G, V, k, kind)
                assert torch.equal(v.view(torch.int32), b[1].view(torch.int32)), (G, V, k, kind)


def test_masked_topk_pair_replayed_in_a_captured_graph_equals_eager():
    G, V, k = 16, 7857, 20
    rng = np.random.default_rng(3)
    src = torch.empty(G, V, device=DEV)
    allow = torch.empty((V + 31) // 32, dtype=torch.int32, device=DEV)
    excl = torch.empty(G, 120, dtype=torch.int32, device=DEV)
    out = (torch.empty(G, k, dtype=torch.int64, device=DEV), torch.empty(G, k, device=DEV))
    work = torch.empty(ops.topk_work_bytes(G, V, k), dtype=torch.uint8, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ops.topk_rows(src, k, col_offset=1, work=work, out=out, allow=allow, exclude=excl)
    torch.cuda.current_stream().wait_stream(s)
    for kind, density in (("random", 0.5), ("ties", 0.99), ("special", 0.001), ("random", 0.0), ("ties", 1.0)):
        src.copy_(torch.from_numpy(_scores(rng, G, V, kind)))
        allow.copy_(ops.pack_allow(torch.from_numpy(rng.random(V) < density), V))
        excl.copy_(_exclude(rng, G, V, torch.int32)[:, :120])
        g.replay()
        ei, ev = ops.topk_rows(src, k, col_offset=1, allow=allow, exclude=excl)
        torch.cuda.synchronize()
        assert torch.equal(out[0], ei), kind
        assert torch.equal(out[1].view(torch.int32), ev.view(torch.int32)), kind


def test_masked_topk_kernel_refuses_bad_arguments():
    s = torch.randn(3, 100, device=DEV)
    work = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    ids = torch.empty(3, 65, dtype=torch.int64, device=DEV)
    vals = torch.empty(3, 65, device=DEV)
    allow = torch.full((4,), -1, dtype=torch.int32, device=DEV)
    excl = torch.ones(3, 8, dtype=torch.int64, device=DEV)
    L = _lib.lib()

    def call(G, V, k, ld, a=allow, e=excl, dt=I64, ld_e=8, n_e=8):
        return L.mobgt_topk_rows_masked(ops._p(s), ld, G, V, k, 0, ops._p(a), ops._p(e), dt, ld_e, n_e, 1, ops._p(ids),
                                        ops._p(vals), ops._p(work), ops._stream())
    for G, V, k, ld in ((3, 100, 0, 100), (3, 100, 65, 100), (3, 10, 11, 100), (3, 100, 5, 99), (0, 100, 5, 100),
                        (65536, 100, 5, 100)):
        assert call(G, V, k, ld) == -1, (G, V, k, ld)
        assert call(G, V, k, ld, a=None, e=None) == -1, (G, V, k, ld)
    assert call(3, 100, 5, 100, ld_e=7) == -1                  # row stride below the list's width
    assert call(3, 100, 5, 100, n_e=-1) == -1
    assert call(3, 100, 5, 100, dt=2) == -3                    # int16 ids: not a dtype the kernel takes
    torch.cuda.synchronize()
    with pytest.raises(_lib.MobgtError):
        ops.topk_rows(s, 65, allow=allow)
    for k in (0, 101):
        with pytest.raises(ValueError):
            ops.topk_rows(s, k, exclude=excl)


# ------------------------------------------------------------------------------------------------ the model
def test_exclude_visited_on_real_gowalla_g8(g8, real_model):
    """Next-new-POI lists: no POI of the trajectory, and the unrestricted top 64 of the same batch with the visited POIs removed
    (every row that keeps at least k of them)."""
    z, _, table = g8
    coll = DeviceCollator(DEV, bin_table=table, multi_hop_max_dist=20, rel_pos_max=1024)
    k, K = 20, ops.TOPK_MAX
    rows = 0
    for tag in ("a", "b"):
        trajs = real_trajs(z, tag)
        b = coll(trajs)
        G = b.x.shape[0]
        ids = torch.empty(G, k, dtype=torch.int64, device=DEV)
        vals = torch.empty(G, k, device=DEV)
        real_model.recommend_step(b, ids, vals, exclude_visited=True)
        full_i = torch.empty(G, K, dtype=torch.int64, device=DEV)
        full_v = torch.empty(G, K, device=DEV)
        real_model.recommend_step(b, full_i, full_v)
        ids, vals, full_i, full_v = ids.cpu(), vals.cpu(), full_i.cpu(), full_v.cpu()
        x = b.x.reshape(G, -1).cpu()
        for g in range(G):
            visited = set(int(p) for p in trajs[g]["node_name"])
            assert visited == set(x[g].tolist()) - {0}
            assert not visited & set(ids[g].tolist()), (tag, g)
            keep = [j for j in range(K) if int(full_i[g, j]) not in visited]
            if len(keep) >= k:
                rows += 1
                assert ids[g].tolist() == [int(full_i[g, j]) for j in keep[:k]], (tag, g)
                assert torch.equal(vals[g].view(torch.int32), full_v[g, keep[:k]].view(torch.int32)), (tag, g)
    assert rows >= 8, rows


@pytest.mark.parametrize("dataset", ["toyotagraph", "gowalla_nevda"])
def test_restricted_recommend_step_label_space(dataset):
    uni, model, coll = workloads.build("fsq", DEV, seed=2, P=1500, dtype="f32", gemm_dtype="f32",
                                       model_overrides=dict(n_layers=2, dataset_name=dataset))
    model.eval()
    data = _eval_dataset(uni, n=40, seed=71)[:12]
    for t in data:
        t["user"] = t["user"] % model.user_embed_model.user_embedding.num_embeddings     # (toyotagraph's smaller user table)
    b = coll(data, n_pad=bucket_nodes(max(len(t["node_name"]) for t in data)))
    G, k, V = b.x.shape[0], 10, model.out_proj.out_features
    off = 0 if dataset == "toyotagraph" else 1
    with torch.no_grad():
        scores = model(b)[0]
    ids = torch.empty(G, k, dtype=torch.int64, device=DEV)
    vals = torch.empty(G, k, device=DEV)
    rng = np.random.default_rng(1)
    cand = torch.from_numpy(rng.choice(np.arange(off, V + off), V // 3, replace=False))
    allow = ops.pack_allow(cand, V, offset=off).to(DEV)
    for excl, al in ((True, None), (False, allow), (True, allow)):
        model.recommend_step(b, ids, vals, exclude_visited=excl, allow=al)
        wi, wv = ops.topk_rows(scores.cpu(), k, col_offset=off, allow=None if al is None else al.cpu(),
                               exclude=b.x.reshape(G, -1).cpu() if excl else None)
        assert torch.equal(ids.cpu(), wi), (excl, al is not None)
        assert torch.equal(vals.cpu().view(torch.int32), wv.view(torch.int32))
        for g, t in enumerate(data):
            got = set(ids[g].tolist())
            if excl:
                assert not got & set(int(p) for p in t["node_name"])
            if al is not None:
                assert got <= set(cand.tolist())
    # the visited ids are in the label space of the list: excluding them removes exactly the ids the unrestricted list shares
    model.recommend_step(b, ids, vals)
    plain = ids.cpu().clone()
    model.recommend_step(b, ids, vals, exclude_visited=True)
    for g, t in enumerate(data):
        visited = set(int(p) for p in t["node_name"])
        kept = [i for i in plain[g].tolist() if i not in visited]
        assert ids[g].tolist()[:len(kept)] == kept, g


def test_stock_variant_keeps_raising():
    uni, model, coll = workloads.build("fsq", DEV, seed=1, P=1500, variant="stock", model_overrides=dict(n_layers=1))
    ids = torch.empty(1, 5, dtype=torch.int64, device=DEV)
    with pytest.raises(NotImplementedError):
        model.eval().recommend_step(None, ids, torch.empty(1, 5, device=DEV), exclude_visited=True)


# ------------------------------------------------------------------------------------------------ PredictLoop
@pytest.fixture(scope="module")
def fsq_predict():
    uni, model, coll = workloads.build("fsq", DEV, seed=1, P=1500, model_overrides=dict(n_layers=2))
    return uni, model, coll, _eval_dataset(uni)


def test_restricted_predict_loop(fsq_predict):
    uni, model, coll, data = fsq_predict
    V = model.out_proj.out_features
    rng = np.random.default_rng(9)
    cand = torch.from_numpy(rng.choice(np.arange(1, V + 1), V // 2, replace=False))
    loop = PredictLoop(model, coll, data, k=10, batch_size=16, exclude_visited=True, candidates=cand)
    a = loop.run()
    n_graphs = loop.captures
    assert n_graphs >= 3 and len(loop.graphs) == n_graphs
    b = loop.run()
    assert loop.captures == n_graphs                           # replayed, nothing captured again
    eager = PredictLoop(model, coll, data, k=10, batch_size=16, use_graph=False, exclude_visited=True, candidates=cand).run()
    for x, y, z in zip(a, b, eager):
        assert torch.equal(x, y) and torch.equal(x, z)
    # the unrestricted top 64 with the visited and non-candidate POIs removed, wherever 10 of them remain
    full = PredictLoop(model, coll, data, k=ops.TOPK_MAX, batch_size=16).run()
    allowed = set(cand.tolist())
    idx, ids, fids = a[0].cpu().tolist(), a[1].cpu(), full[1].cpu()
    assert idx == full[0].cpu().tolist()
    checked = 0
    for r, i in enumerate(idx):
        visited = set(int(p) for p in data[i]["node_name"])
        got = ids[r].tolist()
        assert set(got) <= allowed and not set(got) & visited
        keep = [p for p in fids[r].tolist() if p in allowed and p not in visited]
        if len(keep) >= 10:
            checked += 1
            assert got == keep[:10], r
    assert checked >= len(idx) // 2, (checked, len(idx))


def test_predict_loop_short_candidate_sets_and_dropped_rows(fsq_predict):
    uni, model, coll, data = fsq_predict
    data = data[:48]
    lens = np.array([len(t["node_name"]) for t in data])
    cut = int(np.sort(lens)[-3])                               # the longest few trajectories are over max_node
    # three candidates, one of them visited by the first trajectory
    cand = torch.tensor([int(data[0]["node_name"][0]), 7, 300])
    saved = coll.max_node
    coll.max_node = cut - 1
    try:
        idx, ids, vals = PredictLoop(model, coll, data, k=5, batch_size=16, exclude_visited=True, candidates=cand).run()
    finally:
        coll.max_node = saved
    idx = idx.cpu().tolist()
    ids, vals = ids.cpu(), vals.cpu()
    n_drop = 0
    for r, i in enumerate(idx):
        if lens[i] >= cut:
            n_drop += 1
            assert ids[r].tolist() == [-1] * 5 and bool(torch.isneginf(vals[r]).all())
            continue
        m = len(set(cand.tolist()) - set(int(p) for p in data[i]["node_name"]))
        assert sorted(ids[r, :m].tolist()) == sorted(set(cand.tolist()) - set(int(p) for p in data[i]["node_name"])), r
        assert bool(torch.isfinite(vals[r, :m]).all())
        assert ids[r, m:].tolist() == [-1] * (5 - m) and bool(torch.isneginf(vals[r, m:]).all()), r
    assert 1 <= n_drop < len(idx)
    assert ids[idx.index(0), 2].item() == -1                   # (the visited candidate is left out)


def test_predict_loop_defaults_are_the_unrestricted_lists(fsq_predict):
    uni, model, coll, data = fsq_predict
    V = model.out_proj.out_features
    data = data[:64]
    plain = PredictLoop(model, coll, data, k=20, batch_size=16).run()
    assert PredictLoop(model, coll, data, k=20, batch_size=16).allow is None
    every = PredictLoop(model, coll, data, k=20, batch_size=16, candidates=torch.arange(1, V + 1)).run()
    for x, y in zip(plain, every):
        assert torch.equal(x, y)
    new = PredictLoop(model, coll, data, k=20, batch_size=16, exclude_visited=True).run()
    for r, i in enumerate(new[0].tolist()):
        assert not set(int(p) for p in data[i]["node_name"]) & set(new[1][r].tolist()), r
