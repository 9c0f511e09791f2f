"""The weight fit on the device (csrc_priorfit/fit.hip through mobgt_amd.priorfit and train.PriorFitLoop) against the host rule
priorfit.terms_host: the launch on either side of its chunk, with one row and sixteen, one feature and eight, one weight row and
sixteen, with and without a base, padded rows whose padding is NaN, int32 and int64 targets in the first column, the last and
out of range, a masked chunk, scores of magnitude 80, a row of every non-finite kind; the same bits twice; every return code
with nothing launched; a captured graph replayed after W is overwritten; PriorFitLoop captured against eager and against the
host rule; and fit_weights on a stack against fit_host.

The gate is derived, not measured: everything is f64, each term is a sum of at most V <= 2^17 products of probabilities with
bounded features, and exp is good to an ulp or two, so the worst case is about V * 2^-53 = 1.5e-11 of scale; the gate is 1e-9 of
scale (priorfit_cases.scales: 1 + |nll|, 1 + max |F_k|, 1 + max |F_k| max |F_j|)."""
import ctypes

import numpy as np
import pytest
import torch

import geoprior_cases as gc
import prior_cases as pc
import priorfit_cases as fc
from mobgt_amd import _priorfit, data, geo, prior, priorfit, workloads
from mobgt_amd.data import bucket_nodes
from mobgt_amd.train import EvalLoop, PriorFitLoop

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHUNK, MAX_K, MAX_L = _priorfit.CHUNK, _priorfit.MAX_K, _priorfit.MAX_L
SENTINEL = -7.25


def up(v):
    return None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(DEV)


def launch(d, **kw):
    """priorfit.terms on the uploaded batch -> (terms numpy [L, G, NT], status bits); the rows keep their padding"""
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = priorfit.terms(up(d["base"]), up(d["feats"]), up(d["y"]), d["offset"], up(d["W"]), V=d["V"], status=status, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), int(status[0])


def host(d):
    V = d["V"]
    return priorfit.terms_host(None if d["base"] is None else d["base"][:, :V], d["feats"][:, :, :V], d["y"], d["offset"], d["W"])


def assert_gate(d, got, want, what=""):
    assert got.shape == want.shape and np.isfinite(got).all(), what
    assert np.array_equal(got[..., 0], want[..., 0]), what              # n: exactly
    err = np.abs(got - want) / fc.scales(d, want)
    assert err.max() <= fc.GATE, (what, float(err.max()), np.unravel_index(err.argmax(), err.shape))
    assert not got[want[..., 0] == 0].any(), what                       # a row that does not count: zeros, exactly


# ------------------------------------------------------------------------------------------------ the launch
@pytest.mark.parametrize("with_base", (True, False), ids=("base", "nobase"))
@pytest.mark.parametrize("V", (1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3))
def test_the_launch_on_either_side_of_a_chunk(V, with_base):
    worst, case = 0.0, 0
    for G in (1, 3, 16):
        for K in (1, 4, MAX_K):
            for L in (1, MAX_L):
                case += 1
                d = fc.batch(G, V, K, L, seed=case, base=with_base, pad=(0, 3, 5)[case % 3], chunk=CHUNK,
                             ydtype=np.int32 if case % 2 else np.int64)
                want, flagged = host(d)
                got, status = launch(d)
                assert status == flagged == 0, (G, K, L)
                assert_gate(d, got, want, (G, K, L))
                assert want[:, 0, 0].all() and (G < 3 or not want[:, 2, 0].any())       # the cases are what they say
                worst = max(worst, float((np.abs(got - want) / fc.scales(d, want)).max()))
    print(f"V = {V}: worst error {worst:.3e} of scale")


def test_a_masked_chunk_and_scores_of_magnitude_80_are_in_the_cases():
    d = fc.batch(16, 2 * CHUNK + 3, 4, 2, seed=1, chunk=CHUNK)
    assert np.isneginf(d["base"][0, CHUNK:2 * CHUNK]).all() and np.isfinite(d["base"][0, :CHUNK]).all()
    assert np.abs(d["base"][1, :d["V"]]).min() > 70 and (d["base"][1, :d["V"]] > 0).any() and (d["base"][1, :d["V"]] < 0).any()
    assert (d["y"][:3] + d["offset"]).tolist() == [0, d["V"] - 1, d["V"]]
    want, _ = host(d)
    got, status = launch(d)
    assert status == 0
    assert_gate(d, got, want)
    assert want[:, 1, 1].max() > 50                                     # an nll of that magnitude, to a relative 1e-9


@pytest.mark.parametrize("kind", fc.KINDS)
def test_a_row_of_every_non_finite_kind(kind):
    for G, V, K, L in ((4, 70, 2, 2), (5, CHUNK + 9, 3, 4)):
        d, row = fc.broken(kind, G, V, K, L)
        want, flagged = host(d)
        got, status = launch(d)
        assert flagged == status == _priorfit.SNONFINITE
        assert not got[:, row].any() and got[:, [0, 2, 3], 0].all()
        assert_gate(d, got, want, kind)
    # out of range alone raises no flag; the status word is sticky and only ORed into
    d = fc.batch(4, 70, 2, 2)
    status = torch.full((1,), 4, dtype=torch.int32, device=DEV)
    out = priorfit.terms(up(d["base"]), up(d["feats"]), up(d["y"]), d["offset"], up(d["W"]), V=70, status=status)
    assert status.tolist() == [4] and not out[:, 2].any()
    d, _ = fc.broken(kind)
    priorfit.terms(up(d["base"]), up(d["feats"]), up(d["y"]), d["offset"], up(d["W"]), V=70, status=status)
    assert status.tolist() == [5]


def test_the_same_bits_twice_whatever_the_workspace_held():
    d = fc.batch(16, 2 * CHUNK + 3, MAX_K, MAX_L, seed=2, chunk=CHUNK, pad=1)
    need = priorfit.work_bytes(MAX_K, 16, d["V"], MAX_L)
    assert need == 16 * MAX_L * 3 * (_priorfit.MAX_NT + 1) * 8
    work = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)     # (NaNs)
    a, _ = launch(d, work=work)
    work.zero_()
    b, _ = launch(d, work=work)
    c, _ = launch(d)
    assert np.array_equal(a.view(np.int64), b.view(np.int64)) and np.array_equal(a.view(np.int64), c.view(np.int64))
    # a weight row's terms do not depend on its place among the rows
    d1 = dict(d, W=np.ascontiguousarray(d["W"][5:6]))
    assert np.array_equal(launch(d1)[0].view(np.int64), a[5:6].view(np.int64))


# ------------------------------------------------------------------------------------------------ the return codes
ARGS = ("base", "ld_base", "feats", "ld_feats", "plane_feats", "K", "G", "V", "y", "y_dtype", "ld_y", "target_offset", "W", "L", "work",
        "terms", "status")


def _good(G=3, V=40, K=2, L=2):
    d = fc.batch(G, V, K, L, pad=2)
    t = dict(base=up(d["base"]), feats=up(d["feats"]), y=up(d["y"]), W=up(d["W"]),
             work=torch.empty(priorfit.work_bytes(K, G, V, L) + 8, dtype=torch.uint8, device=DEV),
             terms=torch.full((L, G, priorfit.nt_of(K)), SENTINEL, dtype=torch.float64, device=DEV),
             status=torch.zeros(1, dtype=torch.int32, device=DEV))
    a = dict(ld_base=V + 2, ld_feats=V + 2, plane_feats=G * (V + 2), K=K, G=G, V=V, y_dtype=_priorfit.I64, ld_y=1, target_offset=d["offset"], L=L)
    a.update({k: v.data_ptr() for k, v in t.items()})
    return d, t, a


def _call(a):
    args = [ctypes.c_void_p(a[k]) if k in ("base", "feats", "y", "W", "work", "terms", "status") else a[k] for k in ARGS]
    rc = _priorfit.LIBRARY.lib().mobgt_priorfit_terms(*args, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


def test_every_return_code_with_nothing_launched():
    d, t, a = _good()
    bad_dim = [dict(K=0), dict(K=MAX_K + 1), dict(L=0), dict(L=MAX_L + 1), dict(G=-1), dict(G=_priorfit.MAX_G + 1), dict(V=-1), dict(V=2 ** 31),
               dict(ld_feats=39), dict(plane_feats=39), dict(ld_base=39), dict(ld_y=0)]
    bad_ptr = [dict(feats=0), dict(feats=a["feats"] + 2), dict(base=a["base"] + 1), dict(y=0), dict(y=a["y"] + 4), dict(W=0), dict(W=a["W"] + 4),
               dict(work=0), dict(work=a["work"] + 4), dict(terms=0), dict(terms=a["terms"] + 4), dict(status=0), dict(status=a["status"] + 2)]
    for change, code in [(c, _priorfit.EBADDIM) for c in bad_dim] + [(c, _priorfit.EALIGN) for c in bad_ptr] + [(dict(y_dtype=2), _priorfit.EDTYPE)]:
        assert _call(dict(a, **change)) == code, change
    assert _call(dict(a, ld_base=0, base=0)) == 0                       # an absent base has no stride to check
    t["terms"].fill_(SENTINEL)
    assert _call(dict(a, G=0)) == 0 and _call(dict(a, V=0)) == 0 and _call(dict(a, G=0, feats=0, y=0, terms=0)) == 0
    assert bool((t["terms"] == SENTINEL).all()) and t["status"].tolist() == [0]         # nothing was launched by any of them
    with pytest.raises(_priorfit.MobgtPriorfitError, match="MOBGT_PRIORFIT_EDTYPE") as e:
        _priorfit.launch("mobgt_priorfit_terms", *(dict(a, y_dtype=7)[k] for k in ARGS), None)
    assert e.value.code == _priorfit.EDTYPE
    assert _call(a) == 0                                                # and the same buffers are good
    want, _ = host(d)
    assert_gate(d, t["terms"].cpu().numpy(), want)
    lib = _priorfit.LIBRARY.lib()
    assert [lib.mobgt_priorfit_nt(K) for K in (0, 1, 4, 8, 9)] == [-1, 4, 16, 46, -1]
    assert lib.mobgt_priorfit_work_bytes(4, 16, 100001, 4) == 16 * 4 * 98 * 17 * 8 and lib.mobgt_priorfit_work_bytes(4, 0, 5, 1) == 0
    assert lib.mobgt_priorfit_work_bytes(9, 1, 1, 1) == -1 and lib.mobgt_priorfit_work_bytes(1, 1, 2 ** 31, 1) == -1
    with pytest.raises(ValueError, match="outside 1 .. 8 features"):
        priorfit.work_bytes(0, 1, 1, 1)
    # the wrapper refuses what it can see
    f, y, W = up(d["feats"]), up(d["y"]), up(d["W"])
    for args, match in (((None, f.double(), y, -1, W), "feats must be f32"), ((None, f, y.float(), -1, W), "int32 or int64 targets"),
                        ((None, f, y, -1, W.float()), r"contiguous f64 \[L, 2\]"), ((None, f, y[:2], -1, W), "3 int32 or int64 targets"),
                        ((f[0, :, :10], f, y, -1, W), r"base must be f32 \[3, >= 42\]"), ((None, f.cpu(), y, -1, W), "GPU only")):
        with pytest.raises(ValueError, match=match):
            priorfit.terms(*args)


def test_a_captured_launch_replayed_after_w_is_overwritten():
    d = fc.batch(16, CHUNK + 1, 5, 4, seed=4, pad=3)
    base, feats, y, W = up(d["base"]), up(d["feats"]), up(d["y"]), up(d["W"])
    work = torch.empty(priorfit.work_bytes(5, 16, d["V"], 4), dtype=torch.uint8, device=DEV)
    out = torch.zeros(4, 16, priorfit.nt_of(5), dtype=torch.float64, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    priorfit.terms(base, feats, y, d["offset"], W, V=d["V"], work=work, out=out, status=status)       # (loads the code object)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        priorfit.terms(base, feats, y, d["offset"], W, V=d["V"], work=work, out=out, status=status)
    torch.cuda.current_stream().wait_stream(stream)
    eager = out.clone()
    for seed in (1, 2):
        new = np.random.RandomState(seed).uniform(-2.0, 2.0, size=d["W"].shape)
        W.copy_(up(new))
        out.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        assert_gate(d, out.cpu().numpy(), host(dict(d, W=new))[0], seed)
    W.copy_(up(d["W"]))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int64), eager.view(torch.int64)) and status.tolist() == [0]


# ------------------------------------------------------------------------------------------------ the loop and the fit
@pytest.fixture(scope="module")
def world():
    """test_gpu_geoprior's world: a seeded distance-decay log of 200 POIs, the baseline and the distance prior fitted on its train
    sessions, the samples every prefix of the 12 others, a small untrained fq Graphormer -- and of every batch the scores
    model.poi_scores(model.encode(batch)), the stack's features and y, downloaded."""
    from mobgt_amd.model_fqandtoyo import Graphormer
    coords, sessions, train = gc.decay_log(seed=11, P=200, box_km=12.0, train=360, test=108, length=9)
    sessions = [(s % 20, list(range(1 + 10 * s, 11 + 10 * s))) for s in range(20)] + sessions      # every POI is visited, so has a category
    train = np.r_[np.ones(20, dtype=bool), train]
    ds = data.SessionDataset([(u, pc.as_checkins(p)) for u, p in sessions])
    built = data.build_universe(ds, train=train, coords_deg=coords, radius_km=3.0, device=DEV)
    torch.manual_seed(13)
    args = dict(workloads.COMMON, n_layers=2, hidden_dim=128, dataset_name="foursquaregraph", ffn_dim=256)
    model = Graphormer(universe=built.universe, num_bins=built.bins.num_bins + 2, **args).to(DEV).eval()
    coll = data.SessionCollator(DEV, bin_table=built.bins.table)
    mb = data.MarkovBaseline.fit(ds, train, P=200, device=DEV)
    pb = geo.pair_bins(coords, bins=built.bins, device=DEV)
    samples = data.PrefixDataset(ds, sessions=~train, device=DEV)
    stack = prior.Stack(mb.prior(), mb.distance_prior(pb))
    V = model.out_proj.out_features
    batches = []
    with torch.no_grad():
        for ids in EvalLoop(model, coll, samples, batch_size=8).batches():
            recs = [samples[i] for i in ids]
            b = coll(recs, n_pad=bucket_nodes(max(r.n for r in recs)))
            scores = model.poi_scores(model.encode(b))
            feats = stack.features(b, 1, torch.zeros(4, len(recs), V, device=DEV))
            batches.append(tuple(v.cpu().numpy() for v in (scores, feats, b.y.reshape(-1))))
    assert built.universe.P == 200 and model.label_offset == 1 and len(samples) >= 60 and V == 200
    assert len({bucket_nodes(samples[i].n) for i in range(len(samples))}) >= 2
    return dict(model=model, coll=coll, mb=mb, pb=pb, samples=samples, batches=batches, stack=stack)


def _host_sums(world, W, scale_model):
    """-> (the terms of the rows W summed over every batch [L, NT], the sum of their scales)"""
    total = bound = 0.0
    for scores, feats, y in world["batches"]:
        d = dict(base=None if scale_model else scores, feats=np.concatenate([scores[None], feats]) if scale_model else feats, y=y,
                 offset=-1, W=W, V=scores.shape[1])
        terms, status = host(d)
        assert status == 0 and terms[..., 0].all()
        total, bound = total + terms.sum(axis=1), bound + fc.scales(d, terms).sum(axis=1)
    return total, bound


@pytest.mark.parametrize("scale_model", (True, False), ids=("scaled", "base"))
def test_the_loop_captured_eager_and_on_the_host(world, scale_model):
    K = 4 + scale_model
    W = np.random.RandomState(K).uniform(-1.0, 1.5, size=(4, K))
    kw = dict(batch_size=8, scale_model=scale_model)
    loop = PriorFitLoop(world["model"], world["coll"], world["samples"], world["stack"], weights=W, **kw)
    assert loop.start.tolist() == [1.0] * K and loop.K == K
    got = loop.run()
    captures = loop.captures
    eager = PriorFitLoop(world["model"], world["coll"], world["samples"], world["stack"], weights=W, use_graph=False, **kw)
    assert captures >= 2 and eager.run().tobytes() == got.tobytes() and eager.captures == 0
    want, bound = _host_sums(world, W, scale_model)
    assert got.shape == want.shape == (4, priorfit.nt_of(K)) and got[:, 0].tolist() == [float(len(world["samples"]))] * 4
    err = np.abs(got - want) / bound
    print(f"worst error of the summed terms: {err.max():.3e} of the summed scales")
    assert err.max() <= fc.GATE
    # new rows, fewer rows: the same graphs, and a row's sums do not depend on its place
    loop.set_rows(W[2:3])
    one = loop.run()
    assert loop.captures == captures and one.shape == (1, priorfit.nt_of(K)) and one[0].tobytes() == got[2].tobytes()
    loop.set_rows(W[::-1])
    assert loop.run().tobytes() == got[::-1].tobytes() and loop.captures == captures
    assert all(p.status.tolist() == [0] for p in world["stack"].priors) and loop.status.tolist() == [0]


def test_what_the_loop_refuses(world):
    model, coll, samples, stack = (world[k] for k in ("model", "coll", "samples", "stack"))
    with pytest.raises(ValueError, match="world = 2: a fit on several ranks is not offered"):
        PriorFitLoop(model, coll, samples, stack, batch_size=8, rank=0, world=2)
    for kw in (dict(exclude_visited=True), dict(candidates=torch.arange(1, 9)), dict(within_km=2.0)):
        with pytest.raises(ValueError, match="a fit under a restriction .* is not offered"):
            PriorFitLoop(model, coll, samples, stack, batch_size=8, **kw)

    class Wide:
        n_weights, WEIGHTS = 8, tuple("abcdefgh")
    with pytest.raises(ValueError, match=r"8 prior weights and the model's scale are 9 features, one launch takes up to 8 \(MOBGT_PRIORFIT_MAX_K\)"):
        PriorFitLoop(model, coll, samples, Wide(), batch_size=8)
    with pytest.raises(ValueError, match="rows = 17 outside 1 .. 16"):
        PriorFitLoop(model, coll, samples, stack, batch_size=8, rows=17)
    loop = PriorFitLoop(model, coll, samples, stack, batch_size=8)
    for bad in (np.ones((5, 5)), np.ones((1, 4)), np.full((1, 5), np.nan)):
        with pytest.raises(ValueError, match=r"1 .. 4 finite rows of \(scale, user, transition, popularity, distance\) weights"):
            loop.set_rows(bad)
    # scores that are not finite: the rows are left out, the pass is refused
    bias = model.out_proj.bias
    kept = bias.detach().clone()
    try:
        with torch.no_grad():
            bias[3] = float("nan")
        with pytest.raises(ValueError, match=r"PriorFitLoop: scores or features that are not finite \(status 1\)"):
            loop.run()
    finally:
        with torch.no_grad():
            bias.copy_(kept)
    assert loop.run()[0, 0] == len(samples)


def test_fit_weights_on_the_stack(world):
    """The optimum of a strictly convex J is unique: with both gradients <= tol = 1e-7 and the smallest eigenvalue of hess J of
    order 0.1, the device fit and fit_host on the downloaded scores and features differ by at most about 1e-6; the gate is 1e-5."""
    model, coll, samples = (world[k] for k in ("model", "coll", "samples"))
    start = dict(user=1.0, transition=1.0, popularity=1.0, distance=1.0)
    scores = np.concatenate([b[0] for b in world["batches"]])
    feats = np.concatenate([b[1] for b in world["batches"]], axis=1)
    y = np.concatenate([b[2] for b in world["batches"]])
    for scale_model in (True, False):
        st = prior.Stack(world["mb"].prior(), world["mb"].distance_prior(world["pb"]))
        ev = EvalLoop(model, coll, samples, batch_size=8, prior=st)
        before = ev.run()
        captures = ev.captures
        res = st.fit_weights(model, coll, samples, scale_model=scale_model, batch_size=8)
        twin = prior.Stack(world["mb"].prior(), world["mb"].distance_prior(world["pb"]))
        want = priorfit.fit_host(scores, feats, y, target_offset=-1, prior=twin, scale_model=scale_model)
        print(f"scale_model={scale_model}: passes {res.passes} (host {want.passes}), grad {res.grad:.2e}, scale {res.scale:.4f}, "
              f"weights {res.weights}, nll {res.nll_start:.4f} -> {res.nll:.4f}")
        assert res.converged and want.converged and res.passes <= 12 and res.grad <= 1e-7 and res.n == want.n == len(samples)
        assert res.nll < res.nll_start and len(res.history) == res.passes
        assert abs(res.scale - want.scale) <= 1e-5 and max(abs(res.weights[k] - want.weights[k]) for k in st.WEIGHTS) <= 1e-5
        assert res.applied == want.applied == (res.scale > 0)
        if res.applied:
            assert st.get_weights() == {k: float(np.float32(res.weights[k] / res.scale)) for k in st.WEIGHTS}
            after = ev.run()                                            # the evaluation's graphs read the new weights, no new capture
            assert ev.captures == captures and after != before
            fresh = prior.Stack(world["mb"].prior(), world["mb"].distance_prior(world["pb"])).set_weights(**st.get_weights())
            assert after == EvalLoop(model, coll, samples, batch_size=8, prior=fresh).run()
        else:
            assert st.get_weights() == start
        assert scale_model or res.applied                               # without the scale the fit is always written
