"""The radius restriction on the device: `ops.near_words` (csrc/near.hip, mobgt_near_words), per-row allow words in
`ops.topk_rows` / `ops.rank_metrics_masked` (mobgt_topk_rows_masked_rows, mobgt_rank_metrics_masked_rows),
`Graphormer.recommend_step / metric_step(near=)` and `train.PredictLoop / EvalLoop(within_km=)`.

  * mobgt_near_words equals the torch statement of its contract (ops.near_words on CPU tensors, itself checked against the
    float64 haversine distance in tests/test_host_near.py) bit for bit: widths around the word, wave and workgroup sizes, id
    lists across the kernel's anchor chunk, both id dtypes, padded strides, rows without anchors, columns without POIs, r = 0
    and r past half the circumference, the shared allow words ANDed in;
  * the _rows kernels equal the torch contract with random words per row, their siblings with ld_allow = 0 and with the same
    words in every row, and refuse a row stride below ceil(V / 32);
  * near_words + per-row top-k replay in a captured graph; the model steps on both label spaces; the loops on S-FSQ.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mobgt_amd import _lib, metrics, ops, synth, workloads                  # noqa: E402
from mobgt_amd._lib import I32, I64                                          # noqa: E402
from mobgt_amd.data import bucket_nodes                                      # noqa: E402
from mobgt_amd.train import EvalLoop, PredictLoop                            # noqa: E402
from test_gpu_eval import _eval_dataset                                      # noqa: E402
from test_gpu_eval_masked import _topk_hits                                  # noqa: E402
from test_gpu_topk_masked import _exclude, _scores, fsq_predict              # noqa: E402,F401  (fsq_predict: fixture)

DEV = "cuda"
NEAR_CHUNK = 256                 # csrc/near.hip: anchors staged in LDS per round; 257 and 513 ids cross one and two boundaries
R_KM = 2.0


def _city(rng, V):
    """pos [V, 4] (label offset 1: column c = POI c + 1) of a city about 20 km across: every 9th column without a POI (+inf),
    every 7th POI on the spot of its left neighbour"""
    c = np.zeros((V + 1, 2))
    c[1:, 0] = 35.68 + 0.08 * rng.standard_normal(V)
    c[1:, 1] = 139.76 + 0.10 * rng.standard_normal(V)
    c[2::7] = c[1:-1:7][:c[2::7].shape[0]]
    pos = ops.pack_positions(torch.from_numpy(c), V, 1)
    pos[4::9, :3] = float("inf")
    return pos


def _ids(rng, G, n, V, dt):
    """[G, n] ids (column + 1) as a column slice of a wider tensor: padding inside, ids below and past the columns; with 16 rows,
    row 0 all padding, row 1 a single id that maps outside [0, V), row 2 padding-trailed after its last id"""
    wide = rng.integers(1, V + 1, (G, n + 3))
    wide[:, 1::4] = 0
    wide[:, 2::11] = V + 1 + rng.integers(0, 50)
    wide[:, 6::13] = -3
    if G > 2:
        wide[0] = 0
        wide[1] = 0
        wide[1, 0] = V + 9
        wide[2, max(1, n // 2):] = 0
    return torch.from_numpy(wide).to(dt)[:, :n]


def _near_check(pos, h, c2, mode, tag, allow=None, slack=0):
    """the kernel on a device copy of h that keeps a padded row stride, into words with `slack` extra words per row"""
    want = ops.near_words(pos, h, 1, c2, mode, allow=allow)
    G, W = want.shape
    base = torch.zeros(h.shape[0], h.shape[1] + 3, dtype=h.dtype, device=DEV)
    hd = base[:, :h.shape[1]]
    hd.copy_(h)
    assert hd.stride(0) > hd.shape[1]                          # ld_hist > n
    out = torch.full((G, W + slack), 0x5a5a5a5a, dtype=torch.int32, device=DEV)
    got = ops.near_words(pos.to(DEV), hd, 1, c2, mode, allow=None if allow is None else allow.to(DEV), out=out)
    assert got is out
    assert torch.equal(out[:, :W].cpu(), want), tag
    assert bool((out[:, W:] == 0x5a5a5a5a).all()), tag          # the slack words are not written
    return want


@pytest.mark.parametrize("V", [1, 31, 32, 33, 63, 64, 65, 1024, 1025, 2049, 100001])
def test_near_words_kernel_is_the_torch_statement_bit_for_bit(V):
    rng = np.random.default_rng(V)
    pos = _city(rng, V)
    c2 = ops.chord2_of_km(R_KM)
    W = (V + 31) // 32
    allow = ops.pack_allow(torch.from_numpy(rng.random(V) < 0.5), V)
    seen = 0
    for G in (1, 16):
        for n in (1, 2, 64, 257, 513):
            dt = torch.int32 if (n + G) % 2 else torch.int64
            h = _ids(rng, G, n, V, dt)
            if V == 100001 and G == 16 and n > 64:
                # (the CPU statement costs G x anchors x V: here the lists keep only the ids on both sides of every chunk
                #  boundary and a few others, so the kernel still walks every chunk of every row)
                keep = torch.zeros(n, dtype=torch.bool)
                keep[[j for j in (0, 1, 100, NEAR_CHUNK - 1, NEAR_CHUNK, NEAR_CHUNK + 1, 2 * NEAR_CHUNK - 1, 2 * NEAR_CHUNK) if j < n]] = True
                h = h.clone()
                h[:, ~keep] = 0
                assert int((h[3:] != 0).sum()) > 0
            want = _near_check(pos, h, c2, "any", (G, n, "any"), slack=3)
            seen += int((want != 0).sum())
            _near_check(pos, h, c2, "last", (G, n, "last"), slack=3)
        h = _ids(rng, G, 64, V, torch.int64)
        _near_check(pos, h.to(torch.int32), c2, "last", (G, "i32"))
        _near_check(pos, h, c2, "any", (G, "allow_and"), allow=allow)
        _near_check(pos, h, c2, "last", (G, "allow_and"), allow=allow)
        # r = 0: the anchor itself and the POIs on its spot; r past half the circumference: every column with a POI
        zero = _near_check(pos, h, 0.0, "any", (G, "r0"))
        every = _near_check(pos, h, ops.chord2_of_km(1e9), "last", (G, "all"))
        has = ops.pack_allow(torch.isfinite(pos[:, 0]), V)
        for g in range(G):
            cols = h[g].long() - 1
            cols = cols[(h[g] != 0) & (cols >= 0) & (cols < V)]
            anchored = bool(torch.isfinite(pos[cols, 0]).any()) if cols.numel() else False
            last_ok = cols.numel() > 0 and bool(torch.isfinite(pos[cols[-1], 0]))
            assert torch.equal(every[g], has if last_ok else torch.zeros_like(has)), (G, g)
            assert bool((zero[g] != 0).any()) == anchored, (G, g)
        if V % 32:
            assert bool(((every[:, W - 1].long() & 0xffffffff) >> (V % 32) == 0).all())     # bits at columns >= V are 0
    assert seen > 0 or V < 32
    # no ids at all: every word is written, as zeros
    out = torch.full((2, W), -1, dtype=torch.int32, device=DEV)
    for mode in ("last", "any"):
        ops.near_words(pos.to(DEV), torch.zeros(2, 0, dtype=torch.int64, device=DEV), 1, c2, mode, out=out.fill_(-1))
        assert bool((out == 0).all()), mode


def test_near_words_refuses_bad_arguments():
    V, G, n = 100, 3, 8
    pos = _city(np.random.default_rng(0), V).to(DEV)
    h = torch.ones(G, n, dtype=torch.int64, device=DEV)
    words = torch.zeros(G, 4, dtype=torch.int32, device=DEV)
    L = _lib.lib()

    def call(V=V, G=G, dt=I64, ld=n, n=n, mode=0, ld_w=4, p=pos, hist=h, w=words):
        return L.mobgt_near_words(ops._p(p), V, ops._p(hist), dt, ld, n, 1, mode, 1.0, None, ops._p(w), ld_w, G, ops._stream())
    assert call() == 0 and call(mode=1) == 0 and call(dt=I32, ld=16, n=16) == 0
    for bad in (dict(V=0), dict(G=0), dict(G=65536), dict(ld=n - 1), dict(n=-1), dict(mode=2), dict(mode=-1), dict(ld_w=3),
                dict(p=None), dict(hist=None), dict(w=None)):
        assert call(**bad) == -1, bad
    assert call(dt=2) == -3
    assert call(hist=None, n=0, ld=0) == 0                     # an empty id list needs no pointer
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ per-row allow words
def _row_words(rng, G, V):
    """[G, W + 2] words, a different density per row (row 0 none, row 1 every column) -> the [G, W] view with a padded stride"""
    dens = np.concatenate([[0.0, 1.0], rng.random(max(G - 2, 0))])[:G] if G > 1 else np.array([0.5])
    m = torch.from_numpy(rng.random((G, V)) < dens[:, None])
    W = (V + 31) // 32
    wide = torch.full((G, W + 2), -1, dtype=torch.int32)
    wide[:, :W] = torch.stack([ops.pack_allow(m[g], V) for g in range(G)])
    return wide


@pytest.mark.parametrize("V", [1, 63, 1025, 3680, 100001])
def test_topk_rows_kernel_with_words_per_row_is_the_contract_bit_for_bit(V):
    rng = np.random.default_rng(V)
    W = (V + 31) // 32
    for G in (1, 16):
        wide = _row_words(rng, G, V)
        wd = wide.to(DEV)[:, :W]
        assert wd.stride(0) == W + 2
        for k, kind in ((1, "ties"), (20, "random"), (64, "special")):
            if k > V:
                continue
            s = torch.from_numpy(_scores(rng, G, V, kind))
            for excl in (None, _exclude(rng, G, V, torch.int32), _exclude(rng, G, V, torch.int64)):
                ids, vals = ops.topk_rows(s.to(DEV), k, col_offset=1, allow=wd, exclude=None if excl is None else excl.to(DEV))
                wi, wv = ops.topk_rows(s, k, col_offset=1, allow=wide[:, :W], exclude=excl)
                assert torch.equal(ids.cpu(), wi), (G, V, k, kind)
                assert torch.equal(vals.cpu().view(torch.int32), wv.contiguous().view(torch.int32)), (G, V, k, kind)
            if G > 1:
                assert ids[0].tolist() == [-1] * k             # the row without candidates


def _rank_statement(s, y, words, hist, exclude_hist, gain):
    """mobgt_rank_metrics_masked's contract per row, summed in row order as the finish kernel sums (f64, one row after the
    other): [3, 11].  gain[lo] = 1 / log2(lo + 2)."""
    G, V = s.shape
    bits = (words.long()[:, :, None] >> torch.arange(32)) & 1             # decoded here, not by the code under test
    cand = bits.reshape(G, -1)[:, :V].bool()
    if exclude_hist:
        for g in range(G):
            for p in hist[g].tolist():
                if p != 0 and 0 <= p - 1 < V:
                    cand[g, p - 1] = False
    out = np.zeros((3, 11))
    stopped = False
    for g in range(G):
        t = int(y[g]) - 1
        ok = 0 <= t < V
        in_hist = ok and t + 1 in [p for p in hist[g].tolist() if p != 0]
        stopped = stopped or t == 0
        for sl in (0, 2 if in_hist else 1):
            out[sl, 0] += 1.0
        if not (ok and bool(cand[g, t])):
            continue
        gt = int(((s[g] > s[g, t]) & cand[g]).sum())
        eq = (s[g] == s[g, t]) & cand[g]
        lo, hi = gt + int(eq[:t].sum()), gt + int(eq[t + 1:].sum())
        for sl in (0, 2 if in_hist else 1):
            out[sl, 10] += 1.0
            if not stopped and lo < 20:
                for q, kk in enumerate((1, 5, 10, 20)):
                    if lo < kk:
                        out[sl, 1 + q] += 1.0
                        out[sl, 5 + q] += gain[lo]
            out[sl, 9] += 1.0 / (hi + 1.0)
    return torch.from_numpy(out)


def _rank_case(rng, G, V):
    s = rng.integers(-3, 4, (G, V)).astype(np.float32) * 0.5 if V < 100 else rng.standard_normal((G, V)).astype(np.float32)
    y = rng.integers(1, V + 1, G)
    h = rng.integers(-2, V + 4, (G, 24))
    h[:, ::4] = 0
    y[::2] = np.where(h[::2, 1] >= 1, np.minimum(h[::2, 1], V), 1)           # revisits
    if G > 4:
        y[3] = V + 3                                                         # out of range
        y[G // 2] = 1                                                        # column 0: the batch's hits stop here
    for g in range(G):
        c = int(y[g]) - 1
        for d in (-1, 1):                                                    # ties on both sides of the target
            if 0 <= c < V and 0 <= c + d < V:
                s[g, c + d] = s[g, c]
    return torch.from_numpy(s), torch.from_numpy(y), torch.from_numpy(h)


@pytest.mark.parametrize("G,V", [(16, 1), (16, 63), (16, 1025), (16, 3680), (16, 100001), (2, 300000)])
def test_rank_metrics_kernel_with_words_per_row_is_the_contract_bit_for_bit(G, V):
    """Counts against metrics.restricted_sums; every field, bit for bit, against the contract summed in the finish kernel's
    order (f64 sums depend on their order; the gains 1 / log2(lo + 2) are taken from torch on the device, whose log2 the
    kernel calls).  300 000 columns walk each workgroup's range in sub-ranges of 2 048."""
    rng = np.random.default_rng(V)
    W = (V + 31) // 32
    gain = (1.0 / torch.log2(torch.arange(2, 22, dtype=torch.float64, device=DEV))).cpu().numpy()
    s, y, h = _rank_case(rng, G, V)
    wide = _row_words(rng, G, V)
    wd = wide.to(DEV)[:, :W]
    for hist_dtype in (torch.int32, torch.int64):
        for excl, split in ((True, True), (False, True), (False, False)):
            acc = metrics.new_restricted_accumulator(DEV, split)
            ops.rank_metrics_masked(s.to(DEV), y.to(DEV), acc, target_offset=-1, allow=wd, hist=h.to(hist_dtype).to(DEV),
                                    exclude_hist=excl, split=split)
            got = acc.cpu()
            want = metrics.restricted_sums(s, y, -1, wide[:, :W], h, 1, excl, split)
            counts = [0, 1, 2, 3, 4, 10]
            assert torch.equal(got[:, counts], want[:, counts]), (G, V, excl, split)
            seq = _rank_statement(s, y, wide[:, :W], h, excl, gain)[:3 if split else 1]
            print("rank_rows", G, V, excl, split, "max |got - statement|", float((got - seq).abs().max()))
            assert torch.equal(got, seq), (G, V, excl, split, got, seq)
    assert 0 < int(got[0, 10]) < G or V == 1


def test_rows_kernels_are_their_siblings_on_shared_words():
    """ld_allow = 0 is the sibling's call; the same words in every row give the sibling's result -- bit for bit"""
    rng = np.random.default_rng(5)
    L = _lib.lib()
    for G, V, k in ((16, 3680, 20), (5, 63, 10), (16, 100001, 64)):
        W = (V + 31) // 32
        s, y, h = _rank_case(rng, G, V)
        s, y, h = s.to(DEV), y.to(DEV), h.to(DEV)
        shared = ops.pack_allow(torch.from_numpy(rng.random(V) < 0.4), V).to(DEV)
        rows = shared[None, :].repeat(G, 1)
        a = ops.topk_rows(s, k, col_offset=1, allow=shared, exclude=h)
        b = ops.topk_rows(s, k, col_offset=1, allow=rows, exclude=h)
        ids = torch.empty(G, k, dtype=torch.int64, device=DEV)
        vals = torch.empty(G, k, device=DEV)
        work = torch.empty(ops.topk_work_bytes(G, V, k), dtype=torch.uint8, device=DEV)
        ops.check(L.mobgt_topk_rows_masked_rows(ops._p(s), V, G, V, k, 1, ops._p(shared), 0, ops._p(h), I64, h.shape[1], h.shape[1],
                                                1, ops._p(ids), ops._p(vals), ops._p(work), ops._stream()), "ld_allow = 0")
        for i, v in (b, (ids, vals)):
            assert torch.equal(i, a[0]) and torch.equal(v.view(torch.int32), a[1].view(torch.int32)), (G, V)
        accs = [metrics.new_restricted_accumulator(DEV, True) for _ in range(3)]
        ops.rank_metrics_masked(s, y, accs[0], target_offset=-1, allow=shared, hist=h, exclude_hist=True, split=True)
        ops.rank_metrics_masked(s, y, accs[1], target_offset=-1, allow=rows, hist=h, exclude_hist=True, split=True)
        work = torch.empty(ops.rank_metrics_masked_work_bytes(G, V), dtype=torch.uint8, device=DEV)
        ops.check(L.mobgt_rank_metrics_masked_rows(ops._p(s), ops._p(y), -1, G, V, ops._p(shared), 0, ops._p(h), I64, h.shape[1],
                                                   h.shape[1], 1, 3, ops._p(accs[2]), ops._p(work), ops._stream()), "ld_allow = 0")
        assert torch.equal(accs[0], accs[1]) and torch.equal(accs[0], accs[2]), (G, V)
        assert float(accs[0][0, 10]) > 0
        # a row stride below ceil(V / 32) is refused, with or without a list of ids
        if W > 1:
            assert L.mobgt_topk_rows_masked_rows(ops._p(s), V, G, V, k, 1, ops._p(rows), W - 1, None, I64, 0, 0, 0, ops._p(ids),
                                                 ops._p(vals), ops._p(work), ops._stream()) == -1
            assert L.mobgt_rank_metrics_masked_rows(ops._p(s), ops._p(y), -1, G, V, ops._p(rows), W - 1, ops._p(h), I64, h.shape[1],
                                                    h.shape[1], 1, 3, ops._p(accs[2]), ops._p(work), ops._stream()) == -1
        assert L.mobgt_topk_rows_masked_rows(ops._p(s), V, G, V, k, 1, ops._p(rows), -1, None, I64, 0, 0, 0, ops._p(ids),
                                             ops._p(vals), ops._p(work), ops._stream()) == -1
    torch.cuda.synchronize()


def test_near_words_and_per_row_topk_replay_in_a_captured_graph():
    G, V, k, n = 16, 7857, 20, 64
    rng = np.random.default_rng(3)
    pos = _city(rng, V).to(DEV)
    c2 = ops.chord2_of_km(R_KM)
    src = torch.empty(G, V, device=DEV)
    x = torch.zeros(G, n, dtype=torch.int32, device=DEV)
    words = torch.zeros(G, (V + 31) // 32, dtype=torch.int32, device=DEV)
    out = (torch.empty(G, k, dtype=torch.int64, device=DEV), torch.empty(G, k, device=DEV))
    work = torch.empty(ops.topk_work_bytes(G, V, k), dtype=torch.uint8, device=DEV)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        ops.near_words(pos, x, 1, c2, "last", out=words)
        ops.topk_rows(src, k, col_offset=1, work=work, out=out, allow=words, exclude=x)
    torch.cuda.current_stream().wait_stream(st)
    listed = 0
    for kind in ("random", "ties", "special"):
        src.copy_(torch.from_numpy(_scores(rng, G, V, kind)))
        x.copy_(_ids(rng, G, n, V, torch.int32))
        g.replay()
        ew = ops.near_words(pos, x, 1, c2, "last")
        ei, ev = ops.topk_rows(src, k, col_offset=1, allow=ew, exclude=x)
        torch.cuda.synchronize()
        assert torch.equal(words, ew), kind
        assert torch.equal(out[0], ei) and torch.equal(out[1].view(torch.int32), ev.view(torch.int32)), kind
        listed += int((ei >= 0).sum())
    assert listed > 0


# ------------------------------------------------------------------------------------------------ the model
def _coords(uni):
    c = np.zeros((uni.P + 1, 2))
    c[1:] = uni.poi_table[:, 2:4]
    return c


def _km(c, a, ids):
    """float64 haversine from POI a to POIs ids"""
    ids = np.asarray(ids)
    return synth.haversine_km(c[a, 0], c[a, 1], c[ids, 0], c[ids, 1])


@pytest.mark.parametrize("dataset", ["toyotagraph", "gowalla_nevda"])
def test_steps_with_near_on_both_label_spaces(dataset):
    uni, model, coll = workloads.build("fsq", DEV, seed=2, P=1500, dtype="f32", gemm_dtype="f32",
                                       model_overrides=dict(n_layers=2, dataset_name=dataset))
    model.eval()
    c = _coords(uni)
    data = _eval_dataset(uni, n=40, seed=71)[:16]
    for t in data:
        t["user"] = t["user"] % model.user_embed_model.user_embedding.num_embeddings     # (toyotagraph's smaller user table)
    for i in (1, 4, 6, 9, 12):                                 # targets close to the anchor: the nearest other POI
        a = int(data[i]["node_name"][-1])
        d = _km(c, a, np.arange(1, uni.P + 1))
        d[a - 1] = np.inf
        data[i]["target"] = np.array([int(np.argmin(d)) + 1], dtype=np.int64)
    b = coll(data, n_pad=bucket_nodes(max(len(t["node_name"]) for t in data)))
    G, k, V = b.x.shape[0], 20, model.out_proj.out_features
    off = 0 if dataset == "toyotagraph" else 1
    pos = ops.pack_positions(torch.from_numpy(c), V, off).to(DEV)
    x = b.x.reshape(G, -1)
    y = b.y.reshape(-1).cpu()
    with torch.no_grad():
        scores = model(b)[0].float().cpu()
    rng = np.random.default_rng(1)
    cand = torch.from_numpy(rng.choice(np.arange(1, uni.P + 1), uni.P // 2, replace=False))
    shared = ops.pack_allow(cand, V, offset=off).to(DEV)
    ids = torch.empty(G, k, dtype=torch.int64, device=DEV)
    vals = torch.empty(G, k, device=DEV)
    words = torch.full((G, (V + 31) // 32), -1, dtype=torch.int32, device=DEV)
    short = hits = 0
    for r_km, mode, excl, al in ((1.0, "last", False, None), (1.0, "any", True, None), (0.3, "last", True, shared),
                                 (3.0, "last", False, shared)):
        near = (pos, ops.chord2_of_km(r_km), mode, words)
        model.recommend_step(b, ids, vals, exclude_visited=excl, allow=al, near=near)
        acc = metrics.new_restricted_accumulator(DEV, True)
        model.metric_step(b, acc, exclude_visited=excl, allow=al, split_revisits=True, near=near)
        got = ids.cpu()
        # the torch statement on the same scores
        ww = ops.near_words(pos.cpu(), x.cpu(), off, near[1], mode, allow=None if al is None else al.cpu())
        assert torch.equal(words.cpu(), ww)
        wi, wv = ops.topk_rows(scores, k, col_offset=off, allow=ww, exclude=x.cpu() if excl else None)
        assert torch.equal(got, wi) and torch.equal(vals.cpu().view(torch.int32), wv.view(torch.int32)), (r_km, mode)
        for g, t in enumerate(data):
            assert [int(p) for p in x[g].tolist() if p != 0] == [int(p) for p in t["node_name"]]
            anchors = [int(p) for p in t["node_name"]] if mode == "any" else [int(t["node_name"][-1])]
            row = [p for p in got[g].tolist() if p >= 0]
            assert got[g].tolist() == row + [-1] * (k - len(row))              # -1 only after the row's last candidate
            short += len(row) < k
            if row:
                d = np.min([_km(c, a, row) for a in anchors], 0)
                assert d.max() <= r_km + 0.005, (g, r_km, mode, d.max())        # float64 haversine, or inside the 5 m band
            # every POI that is surely inside (and allowed) is a candidate: a short row lists all of them
            inside = np.min([_km(c, a, np.arange(1, uni.P + 1)) for a in anchors], 0) < r_km - 0.005
            sure = set((np.nonzero(inside)[0] + 1).tolist())
            if al is not None:
                sure &= set(cand.tolist())
            if excl:
                sure -= set(int(p) for p in t["node_name"])
            if len(row) < k:
                assert sure <= set(row), (g, r_km, mode)
        a = acc.cpu()
        h = _topk_hits(got, y, -off)                           # a hit at k <=> y is in the restricted list's first k
        assert np.array_equal(a[0, 1:5].numpy(), h), (r_km, mode, a[0, 1:5], h)
        hits += h[3]
        want = metrics.restricted_sums(scores, y, -off, ww, x.cpu(), off, excl, True)
        assert torch.equal(a[:, [0, 1, 2, 3, 4, 10]], want[:, [0, 1, 2, 3, 4, 10]]), (r_km, mode)
        assert int(a[0, 0]) == G and int(a[0, 10]) < G         # targets outside the radius count in n only
    assert short > 0 and hits > 0


# ------------------------------------------------------------------------------------------------ the loops on S-FSQ
def _eager_lists(model, coll, data, batches, k, pos, c2, mode, excl, shared):
    """per batch: recommend scores on the device, then the torch statement (near_words, topk_rows) on the host"""
    out = {}
    for idx in batches:
        trajs = [data[i] for i in idx if len(data[i]["node_name"]) <= coll.max_node]
        b = coll(trajs, n_pad=bucket_nodes(max(len(t["node_name"]) for t in trajs)))
        with torch.no_grad():
            s = model(b)[0].float().cpu()
        x = b.x.reshape(len(trajs), -1).cpu()
        ww = ops.near_words(pos, x, 1, c2, mode, allow=shared)
        wi, wv = ops.topk_rows(s, k, col_offset=1, allow=ww, exclude=x if excl else None)
        acc = metrics.restricted_sums(s, b.y.reshape(-1).cpu(), -1, ww, x, 1, excl, True)
        out[tuple(idx)] = (wi, wv, acc)
    return out


def test_loops_within_km_on_sfsq(fsq_predict):
    uni, model, coll, data = fsq_predict
    data = data[:64]
    assert coll.coords is None                                 # S-FSQ: a bin table, no coordinates on the collator
    c = torch.from_numpy(_coords(uni))
    V, k = model.out_proj.out_features, 10
    pos = ops.pack_positions(c, V, 1)
    rng = np.random.default_rng(4)
    cand = torch.from_numpy(rng.choice(np.arange(1, V + 1), V // 2, replace=False))
    short = 0
    for r_km, mode, excl, cd in ((1.5, "last", False, None), (0.8, "any", True, cand)):
        kw = dict(batch_size=16, exclude_visited=excl, candidates=cd, within_km=r_km, coords=c, near=mode)
        loop = PredictLoop(model, coll, data, k=k, **kw)
        a = loop.run()
        n_graphs = loop.captures
        assert n_graphs >= 1 and len(loop.graphs) == n_graphs
        b = loop.run()
        assert loop.captures == n_graphs                       # replayed, nothing captured again
        e = PredictLoop(model, coll, data, k=k, use_graph=False, **kw).run()
        for p, q, r in zip(a, b, e):
            assert torch.equal(p, q) and torch.equal(p, r)
        model.eval()
        shared = None if cd is None else ops.pack_allow(cd, V, offset=1)
        want = _eager_lists(model, coll, data, loop.batches(), k, pos, ops.chord2_of_km(r_km), mode, excl, shared)
        assert a[0].cpu().tolist() == [i for idx in loop.batches() for i in idx]
        ids, vals = a[1].cpu(), a[2].cpu()
        off = 0
        total = torch.zeros(3, 11, dtype=torch.float64)
        for idx in loop.batches():
            wi, wv, acc = want[tuple(idx)]
            assert torch.equal(ids[off:off + len(idx)], wi), (r_km, mode, off)
            assert torch.equal(vals[off:off + len(idx)].view(torch.int32), wv.view(torch.int32))
            off += len(idx)
            total += acc
        assert bool((ids >= 0).any())
        short += int((ids == -1).sum())
        ev = EvalLoop(model, coll, data, split_revisits=True, **kw)
        res = ev.run()
        n_graphs = ev.captures
        assert n_graphs >= 1 and ev.run() == res and ev.captures == n_graphs
        assert res == EvalLoop(model, coll, data, split_revisits=True, use_graph=False, **kw).run()
        ref = metrics.finalize_restricted(total)
        for part in (None, "new", "revisit"):
            r_, w_ = (res, ref) if part is None else (res[part], ref[part])
            for key, v in w_.items():
                if not isinstance(v, dict):
                    assert r_[key] == pytest.approx(v, rel=1e-12, abs=0), (part, key)
        assert res["n"] == 64 and res["reachable"] < res["n"]
    assert short > 0                                           # rows with fewer than k POIs in their radius
    # Graphormer.recommend / evaluate pass the arguments on
    i2 = model.recommend(data, coll, k=k, within_km=0.8, coords=c, near="any", exclude_visited=True, candidates=cand)
    assert torch.equal(i2[1], a[1])
    assert model.evaluate(data, coll, within_km=0.8, coords=c, near="any", exclude_visited=True, candidates=cand,
                          split_revisits=True) == res
    with pytest.raises(ValueError):
        PredictLoop(model, coll, data, within_km=1.0)          # no coordinates anywhere


def test_default_loops_are_untouched(fsq_predict, monkeypatch):
    """Without within_km a loop holds no words buffer and its captures launch no near_words: today's tensors"""
    uni, model, coll, data = fsq_predict
    data = data[:64]
    c = torch.from_numpy(_coords(uni))
    calls = []
    real = ops.near_words
    monkeypatch.setattr(ops, "near_words", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    plain = PredictLoop(model, coll, data, k=20, batch_size=16)
    assert plain.near is None
    p = plain.run()
    ev_plain = EvalLoop(model, coll, data, batch_size=16)
    assert ev_plain.near is None and not ev_plain.restricted
    e = ev_plain.run()
    assert not calls
    # a radius that holds every POI lists what the plain loop lists; the default loop after it gives its former result
    wide = PredictLoop(model, coll, data, k=20, batch_size=16, within_km=1e5, coords=c).run()
    assert calls
    for u, v in zip(p, wide):
        assert torch.equal(u, v)
    n = len(calls)
    again = PredictLoop(model, coll, data, k=20, batch_size=16).run()
    for u, v in zip(p, again):
        assert torch.equal(u, v)
    assert EvalLoop(model, coll, data, batch_size=16).run() == e and len(calls) == n
    assert set(e) == set(metrics.finalize(metrics.new_accumulator("cpu")))
