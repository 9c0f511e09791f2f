"""The Markov prior on the device (csrc_prior/prior.hip through mobgt_amd.prior) against prior.blend_host, compared as uint32 views:
widths on either side of the kernel's chunk and of a wave, rows of 0 .. 200 entries that straddle two workgroups, both label
offsets, V = P, P + 1 and < P, int32 and int64 ids with padded leading dimensions, rows without an anchor or without a user, in
place and out of place, scores with inf, NaN payloads and -0.0.  Then the entry point itself -- return codes with nothing
launched, the sticky status word -- and the loops: EvalLoop / PredictLoop(prior=) captured and eager against test_step ->
blend_host -> metrics.restricted_sums, set_weights without a new capture, the weight sweep against single-weight loops, tune,
and the old path without a prior."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import anchor_cases as ac
import checkins_cases as cc
import prior_cases as pc
from mobgt_amd import _prior, data, metrics, prior, workloads
from mobgt_amd.data import bucket_nodes
from mobgt_amd.train import EvalLoop, PredictLoop

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHUNK = _prior.CHUNK
POISON = 77.0
WEIGHTS = (0.75, 1.5, 0.3)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def tables(P=pc.GEN_P, users=True):
    """-> prior.PriorTables of the generated counts (numpy), the logs gathered from one log_table as MarkovPrior does"""
    t = pc.generated(P=P)
    log = prior.log_table(max(int(t["val"].max()), int(t["uval"].max()), int(t["pop"].max())))
    ukey, uval = (t["ukey"], t["uval"]) if users else (t["ukey"][:0], t["uval"][:0])
    return prior.PriorTables(t["rowptr"], t["col"], log[t["val"]], ukey, log[uval], log[t["pop"]], t["U"], P)


ARGS = ("scores", "ld_scores", "out", "ld_out", "G", "V", "label_offset", "hist", "hist_dtype", "ld_hist", "n_hist_cols", "user",
        "user_dtype", "ld_user", "user_offset", "rowptr", "col", "lg", "nnz", "ukey", "lu", "nnzU", "U", "lp", "P", "weights", "status")
POINTERS = ("scores", "out", "hist", "user", "rowptr", "col", "lg", "ukey", "lu", "lp", "weights", "status")


def _direct(t, G, V, label_offset=1, wide=False, in_place=False, weights=WEIGHTS, seed=0, status=None):
    """Device buffers and sizes of a direct call: {argument: tensor or int}, and the host inputs under "host".  wide: int64 ids.
    Out of place `out` is poisoned and three columns wider than V; hist is three columns wider than its n."""
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(DEV)
    dtype = np.int64 if wide else np.int32
    hist, user = pc.sample_rows(G, t.P, seed=seed, dtype=dtype)
    scores = pc.scores(G, V, seed=seed)
    n = hist.shape[1]
    d = dict(G=G, V=V, label_offset=label_offset, hist_dtype=_prior.I64 if wide else _prior.I32, user_dtype=_prior.I64 if wide else _prior.I32,
             n_hist_cols=n, ld_hist=n + 3, ld_user=1, user_offset=1, nnz=len(t.col), nnzU=len(t.ukey), U=t.U, P=t.P)
    d["hist"] = up(np.concatenate([hist, np.full((G, 3), 5, dtype=dtype)], axis=1))     # (the columns beyond n hold an id: not read)
    d["user"] = up(user)
    for key in ("rowptr", "col", "lg", "ukey", "lu", "lp"):
        d[key] = up(getattr(t, key))
    d["weights"] = up(np.asarray(weights, dtype=np.float32))
    d["status"] = torch.zeros(1, dtype=torch.int32, device=DEV) if status is None else status
    d["scores"] = up(scores)
    d["ld_scores"] = V
    if in_place:
        d["out"], d["ld_out"] = d["scores"], V
    else:
        d["out"], d["ld_out"] = torch.full((G, V + 3), POISON, dtype=torch.float32, device=DEV), V + 3
    d["host"] = (scores, hist, user)
    return d


def _call(d, **over):
    args = []
    for a in ARGS:
        v = over.get(a, d[a])
        args.append(ctypes.c_void_p(v.data_ptr()) if isinstance(v, torch.Tensor) else v)
    rc = _prior.LIBRARY.lib().mobgt_prior_blend_rows(*args, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


def _assert_blended(d, t, weights=WEIGHTS, status=0):
    scores, hist, user = d["host"]
    V = d["V"]
    host_status = [0]
    want = prior.blend_host(scores, hist, user, t, weights, d["label_offset"], status=host_status)
    got = d["out"].cpu().numpy()
    assert np.array_equal(bits(got[:, :V]), bits(want))                 # every element inside is the rule's, NaN payloads included
    assert np.all(got[:, V:] == POISON)                                 # and nothing beyond V was touched
    assert int(d["status"][0]) == host_status[0] == status
    return want


# ------------------------------------------------------------------------------------------------ the kernel against blend_host
@pytest.mark.parametrize("form", ("in-place-i32", "out-i64"))
@pytest.mark.parametrize("label_offset", (0, 1))
@pytest.mark.parametrize("G", (1, 3, 16))
@pytest.mark.parametrize("V", (1, 31, 32, 33, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 5, 2 * CHUNK + 6))
def test_kernel_equals_the_host_rule(V, G, label_offset, form):
    """P = 2 * CHUNK + 5: the widths are V < P, V = P and V = P + 1.  16 rows walk through every anchor of prior_cases.sample_rows:
    CSR rows of 0, 1, 63, 64, 65 and 200 entries with entries at the chunk edges, the last row, an all-pad row, an anchor id
    P + 1, a user at U and a user without rows."""
    t = tables()
    d = _direct(t, G, V, label_offset, wide=form == "out-i64", in_place=form == "in-place-i32", seed=V + G)
    assert _call(d) == 0
    want = _assert_blended(d, t)
    if G == 16 and V >= CHUNK + 1:
        scores = d["host"][0]
        q = t.col[t.rowptr[5]:t.rowptr[6]] + 1 - label_offset          # the columns of row 6, the anchor of sample 0
        assert {CHUNK - 1, CHUNK} <= set(q.tolist()) and d["host"][1][0].max() > 0     # it straddles two workgroups
        changed = (bits(want) != bits(scores)) | ~np.isfinite(scores)  # (inf and NaN keep their bits under a finite term)
        assert changed[0, CHUNK - 1] and changed[0, CHUNK] and changed[:, :CHUNK].any() and changed[:, CHUNK:].any()
        assert (bits(want) == 0xFFC12345).any() and (bits(want) == 0x80000000).any()      # a NaN payload and some -0.0 survived


def test_no_user_table_and_a_small_universe():
    t = tables(users=False)
    assert len(t.ukey) == 0
    d = _direct(t, 16, CHUNK + 1)
    assert _call(d, ukey=ctypes.c_void_p(0), lu=ctypes.c_void_p(0)) == 0    # nnzU = 0: the table may be null
    _assert_blended(d, t)
    small = tables(P=40)                                                # every row is shorter than a wave's probes
    for lo, V in ((1, 40), (0, 41), (1, 7)):
        d = _direct(small, 16, V, lo, seed=V)
        assert _call(d) == 0
        _assert_blended(d, small)
    d = _direct(small, 0, 40)                                           # no row: nothing is launched
    assert _call(d) == 0


def test_all_three_weights_zero():
    """The output equals the input as floats; -0.0 may become +0.0 where a term applies, and nothing else changes."""
    t = tables()
    d = _direct(t, 16, 2 * CHUNK + 5, weights=(0.0, 0.0, 0.0), seed=3)
    assert _call(d) == 0
    want = _assert_blended(d, t, weights=(0.0, 0.0, 0.0))
    scores = d["host"][0]
    assert ((want == scores) | (np.isnan(want) & np.isnan(scores))).all()
    flipped = bits(want) != bits(scores)
    assert flipped.any() and ((bits(scores)[flipped] == 0x80000000) & (bits(want)[flipped] == 0)).all()


def test_the_weights_are_read_on_the_device_in_their_order():
    t = tables()
    for w in ((2.0, 0.0, 0.0), (0.0, -3.0, 0.0), (0.0, 0.0, 0.5)):
        d = _direct(t, 16, CHUNK + 1, weights=w, seed=9)
        assert _call(d) == 0
        _assert_blended(d, t, weights=w)


@pytest.mark.parametrize("wide", (False, True), ids=("i32", "i64"))
@pytest.mark.parametrize("n", ac.WIDTHS)
def test_the_anchor_search_across_waves_and_strides(n, wide):
    """The history rows of anchor_cases, n ids wide, by direct call: the only id in the first and in the last position, and two
    ids whose positions lie in different waves and strides, the later one deciding -- the rows of two anchors differ, so a wrong
    winner shows in the output."""
    t = tables(P=40)
    d = _direct(t, ac.G, ac.V, ac.LABEL_OFFSET, wide=wide, seed=n)
    scores, _, user = d["host"]
    hist = ac.rows(n, 3, 17, np.int64 if wide else np.int32)
    assert _call(d, hist=torch.from_numpy(hist).to(DEV), n_hist_cols=n, ld_hist=n) == 0
    d["host"] = (scores, hist, user)
    want = _assert_blended(d, t)
    if n > 1:
        assert (bits(want[3]) != bits(prior.blend_host(scores, ac.loser(hist), user, t, WEIGHTS, ac.LABEL_OFFSET)[3])).any()


# ------------------------------------------------------------------------------------------------ the entry point itself
def test_return_codes_with_nothing_launched():
    t = tables()
    G, V = 3, 33
    d = _direct(t, G, V)
    before = d["out"].clone()
    bad = [("G", -1), ("G", 65536), ("V", -1), ("V", 2 ** 31), ("nnz", -1), ("nnz", 2 ** 31), ("nnzU", -1), ("nnzU", 2 ** 31),
           ("n_hist_cols", -1), ("n_hist_cols", 2 ** 31), ("P", 0), ("P", 2 ** 31), ("U", -1), ("U", 2 ** 63 // (t.P * t.P) + 1),
           ("ld_scores", V - 1), ("ld_out", V - 1), ("ld_hist", d["n_hist_cols"] - 1), ("ld_user", 0), ("label_offset", -1),
           ("label_offset", 2), ("user_offset", -1), ("user_offset", 2)]
    for key, value in bad:
        assert _call(d, **{key: value}) == _prior.EBADDIM, (key, value)
    assert _call(d, out=d["scores"]) == _prior.EBADDIM                  # in place with another leading dimension
    for key in ("hist_dtype", "user_dtype"):
        for value in (-1, 2):
            assert _call(d, **{key: value}) == _prior.EDTYPE, (key, value)
    wide = _direct(t, G, V, wide=True)
    for key in POINTERS:
        assert _call(d, **{key: ctypes.c_void_p(0)}) == _prior.EALIGN, key
        assert _call(d, **{key: ctypes.c_void_p(d[key].data_ptr() + 2)}) == _prior.EALIGN, key
        if key in ("hist", "user", "rowptr", "ukey"):                   # 8-byte elements at a 4-byte address
            assert _call(wide, **{key: ctypes.c_void_p(wide[key].data_ptr() + 4)}) == _prior.EALIGN, key
    assert torch.equal(d["out"], before) and torch.equal(wide["out"], before) and int(d["status"][0]) == 0      # nothing was launched
    with pytest.raises(_prior.MobgtPriorError, match="MOBGT_PRIOR_EBADDIM") as e:
        _prior.launch("mobgt_prior_blend_rows", *(-1 if a == "G" else None if a in POINTERS else 1 for a in ARGS), None)
    assert e.value.code == _prior.EBADDIM
    assert _call(d) == 0                                                # and the same buffers are good
    _assert_blended(d, t)


def test_the_status_word():
    """Tables that fit did not make: the row, or the entry, is dropped, the rest is blended as the host rule blends it, and
    SBADINDEX stays in the word through a second, clean call.  None of these inputs is read out of bounds."""
    t = tables()
    nnz = len(t.col)

    def with_(array, i, value):
        out = array.copy()
        out[i] = value
        return out
    r6 = int(t.rowptr[6])                                               # closes row 6 (200 entries), opens row 7 (empty)
    broken = [t._replace(rowptr=with_(t.rowptr, 6, t.rowptr[5] - 1)),   # row 6 descends
              t._replace(rowptr=with_(t.rowptr, t.P, nnz + 7)),         # the last row runs beyond nnz
              t._replace(rowptr=with_(t.rowptr, 0, -1)),                # row 1 starts before the table
              t._replace(col=with_(t.col, r6 - 1, t.P)),                # row 6's last entry: POI P + 1
              t._replace(col=with_(t.col, r6 - 1, 2 ** 31 - 1)),
              t._replace(col=with_(t.col, int(t.rowptr[5]), -1))]       # its first entry
    for V, lo in ((2 * CHUNK + 6, 1), (CHUNK + 1, 0)):
        for bt in broken:
            d = _direct(bt, 16, V, lo, seed=1)
            assert _call(d) == 0
            _assert_blended(d, bt, status=_prior.SBADINDEX)
            clean = _direct(t, 16, V, lo, seed=1, status=d["status"])  # the same word
            assert _call(clean) == 0
            scores, hist, user = clean["host"]
            assert np.array_equal(bits(clean["out"].cpu().numpy()[:, :V]), bits(prior.blend_host(scores, hist, user, t, WEIGHTS, lo)))
            assert int(clean["status"][0]) == _prior.SBADINDEX         # not cleared
    d = _direct(t, 16, 2 * CHUNK + 6)
    assert _call(d) == 0 and int(d["status"][0]) == 0                   # and it stays 0 on valid tables


def test_the_public_call_and_a_captured_graph():
    """MarkovPrior.blend on device tensors: in place by default, `out` and a `weights` view otherwise; a captured blend reads the
    weights set after the capture."""
    t = tables()
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(DEV)
    pr = prior.MarkovPrior(t.P, t.U, up(t.rowptr), up(t.col), up(t.lg), up(t.ukey), up(t.lu), up(t.lp), WEIGHTS)
    G, V = 16, CHUNK + 1
    hist, user = pc.sample_rows(G, t.P)
    scores = pc.scores(G, V)
    want = prior.blend_host(scores, hist, user, t, WEIGHTS, 1)
    s = up(scores)
    assert pr.blend(s, (up(hist), up(user).reshape(G, 1)), 1) is s and np.array_equal(bits(s.cpu().numpy()), bits(want))
    W = up(np.array([[9, 9, 9], [0.5, 0.25, 2.0]], dtype=np.float32))
    out = torch.full((G, V), POISON, device=DEV)
    pr.blend(up(scores), (up(hist).long(), up(user).long()), 1, out=out, weights=W[1])
    assert np.array_equal(bits(out.cpu().numpy()), bits(prior.blend_host(scores, hist, user, t, (0.5, 0.25, 2.0), 1)))
    src, dst = up(scores), torch.zeros(G, V, device=DEV)
    h, u = up(hist), up(user)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        pr.blend(src, (h, u), 1, out=dst)
    torch.cuda.current_stream().wait_stream(stream)
    pr.set_weights(user=-1.0, popularity=0.0)
    graph.replay()
    torch.cuda.synchronize()
    assert pr.get_weights() == dict(user=-1.0, transition=1.5, popularity=0.0)
    assert np.array_equal(bits(dst.cpu().numpy()), bits(prior.blend_host(scores, hist, user, t, (-1.0, 1.5, 0.0), 1)))
    pr.check()
    assert pr.status.tolist() == [0]


# ------------------------------------------------------------------------------------------------ the loops
COUNTS = ("n", "acc@1", "acc@5", "acc@10", "acc@20")
SUMS = ("ndcg@1", "ndcg@5", "ndcg@10", "ndcg@20", "mrr")
LOOP_WEIGHTS = dict(user=1.0, transition=50.0, popularity=0.5)


def _same(got, want):
    for k in COUNTS:
        assert got[k] == want[k], (k, got[k], want[k])
    for k in SUMS:
        np.testing.assert_allclose(got[k], want[k], rtol=1e-12, atol=0, err_msg=k)
    for part in ("new", "revisit"):
        assert (part in got) == (part in want)
        if part in want:
            _same(got[part], want[part])
    assert got.get("reachable") == want.get("reachable")


@pytest.fixture(scope="module")
def world():
    """G14's log: 40 POIs; the tables fitted on its train sessions, the samples every prefix of the others; a small untrained
    fq Graphormer; and the reference of every batch -- test_step's scores, the batch's hist, user and y -- on the host."""
    from mobgt_amd.model_fqandtoyo import Graphormer
    res = data.sessionize(device=DEV, **cc.g14_log("sorted"))
    built = data.build_universe(res.dataset, train=res.train, coords_deg=res.coords_deg, radius_km=3.0, device=DEV)
    torch.manual_seed(13)
    args = dict(workloads.COMMON, n_layers=2, hidden_dim=128, dataset_name="foursquaregraph", ffn_dim=256)
    model = Graphormer(universe=built.universe, num_bins=built.bins.num_bins + 2, **args).to(DEV).eval()
    coll = data.SessionCollator(DEV, bin_table=built.bins.table)
    mb = data.MarkovBaseline.fit(res.dataset, res.train, P=built.universe.P, device=DEV)
    samples = data.PrefixDataset(res.dataset, sessions=~res.train, device=DEV)
    batches = []
    with torch.no_grad():
        for ids in EvalLoop(model, coll, samples, batch_size=4).batches():
            recs = [samples[i] for i in ids]
            b = coll(recs, n_pad=bucket_nodes(max(r.n for r in recs)))
            scores = model.test_step(b)["y_pred"][0]
            batches.append(tuple(v.cpu().numpy() for v in (scores, b.x.reshape(len(recs), -1), b.user.reshape(-1), b.y.reshape(-1))))
    assert built.universe.P == 40 and model.label_offset == 1 and len(samples) >= 8
    return dict(model=model, coll=coll, mb=mb, samples=samples, batches=batches)


def _reference(world, weights, **kw):
    """test_step scores -> blend_host -> metrics.restricted_sums, batch by batch -> the loop's dict, and the blended rows"""
    t = world["mb"].prior().tables()
    restricted = bool(kw)
    total, blended = None, []
    for scores, hist, user, y in world["batches"]:
        s = prior.blend_host(scores, hist, user, t, weights, 1) if weights is not None else scores
        blended.append(s)
        sums = metrics.restricted_sums(torch.from_numpy(s), torch.from_numpy(y), target_offset=-1, hist=torch.from_numpy(hist).long(),
                                       hist_offset=1, exclude_hist=kw.get("exclude_visited", False), split=kw.get("split_revisits", False))
        total = sums if total is None else total + sums
    return (metrics.finalize_restricted(total) if restricted else metrics.finalize(total[0, :10])), blended


def test_the_prior_moves_a_top_1(world):
    """transition = 50 outweighs an untrained model's logits: checked on the host rule, so the loop tests below are not vacuous"""
    w = tuple(LOOP_WEIGHTS[k] for k in prior.WEIGHTS)
    _, blended = _reference(world, w)
    moved = sum(int((s.argmax(1) != b[0].argmax(1)).sum()) for s, b in zip(blended, world["batches"]))
    assert moved >= 1
    assert _reference(world, w)[0]["mrr"] != _reference(world, None)[0]["mrr"]


@pytest.mark.parametrize("kw", ({}, dict(exclude_visited=True, split_revisits=True)), ids=("plain", "new-pois-split"))
def test_eval_loop_with_a_prior(world, kw):
    w = tuple(LOOP_WEIGHTS[k] for k in prior.WEIGHTS)
    pr = world["mb"].prior(**LOOP_WEIGHTS)
    loop = EvalLoop(world["model"], world["coll"], world["samples"], batch_size=4, prior=pr, **kw)
    got = loop.run()
    eager = EvalLoop(world["model"], world["coll"], world["samples"], batch_size=4, use_graph=False, prior=pr, **kw).run()
    assert loop.captures > 0 and got == eager
    want, _ = _reference(world, w, **kw)
    _same(got, want)
    assert got["n"] == len(world["samples"]) and pr.status.tolist() == [0]
    assert world["model"].evaluate(world["samples"], world["coll"], batch_size=4, prior=pr, **kw) == got


def test_predict_loop_lists_are_the_hits_of_the_blended_scores(world):
    w = tuple(LOOP_WEIGHTS[k] for k in prior.WEIGHTS)
    pr = world["mb"].prior(**LOOP_WEIGHTS)
    ev = EvalLoop(world["model"], world["coll"], world["samples"], batch_size=4, prior=pr).run()
    loop = PredictLoop(world["model"], world["coll"], world["samples"], k=20, batch_size=4, prior=pr)
    idx, ids, vals = loop.run()
    assert idx.tolist() == [i for b in loop.batches() for i in b]
    ids = ids.cpu().numpy()
    _, blended = _reference(world, w)
    hits, row = {k: 0 for k in (1, 5, 20)}, 0
    for s, (_, _, _, y) in zip(blended, world["batches"]):
        stopped = False
        for g in range(len(y)):
            order = np.lexsort((np.arange(s.shape[1]), -s[g].astype(np.float64)))
            rank = int(np.nonzero(order == y[g] - 1)[0][0])
            stopped = stopped or y[g] == 1
            for k in hits:
                assert (y[g] in ids[row, :k]) == (rank < k), (row, k)   # in the list exactly when the blended row ranks it there
                hits[k] += int(rank < k and not stopped)                # (EvalLoop's counts stop at a batch's first target 1: get_acc)
            row += 1
    assert row == len(ids) and all(hits[k] == round(ev[f"acc@{k}"] * ev["n"]) for k in hits) and hits[20] > 0
    plain = PredictLoop(world["model"], world["coll"], world["samples"], k=20, batch_size=4).run()[1].cpu().numpy()
    assert (plain[:, 0] != ids[:, 0]).any()
    eager = PredictLoop(world["model"], world["coll"], world["samples"], k=20, batch_size=4, use_graph=False, prior=pr).run()
    assert np.array_equal(eager[1].cpu().numpy(), ids) and torch.equal(eager[2].view(torch.int32), vals.view(torch.int32))


def test_new_weights_need_no_new_capture(world):
    pr = world["mb"].prior(**LOOP_WEIGHTS)
    loop = EvalLoop(world["model"], world["coll"], world["samples"], batch_size=4, prior=pr)
    first = loop.run()
    captures = loop.captures
    pr.set_weights(user=0.0, transition=0.25, popularity=2.0)
    second = loop.run()
    assert loop.captures == captures > 0 and second != first
    fresh = EvalLoop(world["model"], world["coll"], world["samples"], batch_size=4, prior=world["mb"].prior(0.0, 0.25, 2.0)).run()
    assert second == fresh
    _same(second, _reference(world, (0.0, 0.25, 2.0))[0])


def test_a_sweep_is_its_single_weight_loops(world):
    W = [[1.0, 50.0, 0.5], [0.0, 0.25, 2.0], [0.0, 0.0, 0.0]]
    pr = world["mb"].prior(7.0, 7.0, 7.0)
    for kw in ({}, dict(exclude_visited=True, split_revisits=True)):
        got = EvalLoop(world["model"], world["coll"], world["samples"], batch_size=4, prior=pr, prior_weights=W, **kw).run()
        assert isinstance(got, list) and len(got) == 3
        for row, one in zip(W, got):
            single = EvalLoop(world["model"], world["coll"], world["samples"], batch_size=4, prior=world["mb"].prior(*row), **kw).run()
            assert one == single                                        # the same ranking launches on the same bits
    assert pr.get_weights() == dict(user=7.0, transition=7.0, popularity=7.0)            # the prior's own weights are not touched
    with pytest.raises(ValueError, match="prior_weights without prior="):
        EvalLoop(world["model"], world["coll"], world["samples"], batch_size=4, prior_weights=W)
    with pytest.raises(ValueError, match=r"the prior is on cpu, the loop on cuda"):
        fitted_on = world["mb"]._fitted_on
        EvalLoop(world["model"], world["coll"], world["samples"], batch_size=4, prior=data.MarkovBaseline.fit(*fitted_on, P=40, device="cpu").prior())


def test_tune_sets_the_best_weights(world):
    grid = [[0.0, 0.0, 0.0], [1.0, 50.0, 0.5], [0.0, 0.25, 2.0], [1.0, 50.0, 0.5]]
    pr = world["mb"].prior()
    results = pr.tune(world["model"], world["coll"], world["samples"], grid, batch_size=4)
    assert len(results) == 4 and results[1] == results[3]
    best = max(range(4), key=lambda i: (results[i]["mrr"], -i))
    assert pr.get_weights() == dict(zip(prior.WEIGHTS, grid[best])) and pr.weights.tolist() == grid[best]
    assert len({r["mrr"] for r in results}) == 3
    by_acc = pr.tune(world["model"], world["coll"], world["samples"], grid, key="acc@5", batch_size=4)
    assert by_acc == results and pr.weights.tolist() == grid[max(range(4), key=lambda i: (results[i]["acc@5"], -i))]


def test_without_a_prior_the_old_path_runs(world, monkeypatch):
    calls = []
    blend, launch = prior.MarkovPrior.blend, _prior.launch
    monkeypatch.setattr(prior.MarkovPrior, "blend", lambda self, *a, **k: calls.append("blend") or blend(self, *a, **k))
    monkeypatch.setattr(_prior, "launch", lambda *a: calls.append("launch") or launch(*a))
    plain = EvalLoop(world["model"], world["coll"], world["samples"], batch_size=4).run()
    PredictLoop(world["model"], world["coll"], world["samples"], k=5, batch_size=4).run()
    acc = metrics.new_accumulator(DEV)
    recs = [world["samples"][i] for i in range(4)]
    world["model"].metric_step(world["coll"](recs), acc)
    assert calls == []
    _same(plain, _reference(world, None)[0])
    EvalLoop(world["model"], world["coll"], world["samples"], batch_size=4, prior=world["mb"].prior(), use_graph=False).run(max_batches=1)
    assert calls[:2] == ["blend", "launch"] and calls.count("blend") == calls.count("launch")
