"""The CSR form of the POI graph (S-BIG, BASELINE configs[4]: P = 100 000, where no dense P x P adjacency exists):
csrc/spmm.hip against dense products, the coordinate-based distance bins against np.digitize on the dense distance
matrix, and the whole fq model on a sparse universe against the oracle fed with the SAME universe densified
(reference: modelGNN.py:38-74, model_fqandtoyo.py:456-486, collator.py:428-437)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mobgt_amd import synth, workloads                                # noqa: E402
from mobgt_amd.data import DeviceCollator                              # noqa: E402
from mobgt_amd.modelGNN import CsrAdj, spmm, _SpConvFn                 # noqa: E402
from oracle import model_oracle as mo                                   # noqa: E402

DEV = "cuda"


def _csr(P, seed):
    from scipy import sparse
    rng = np.random.RandomState(seed)
    a = sparse.random(P, P, density=0.01, random_state=rng, format="csr", dtype=np.float32)
    a.data = rng.rand(a.nnz).astype(np.float32) + 0.1
    return a


def test_spmm_kernels_match_dense_products():
    P, C = 1500, 128
    a = _csr(P, 0)
    adj = CsrAdj(*[t.to(DEV) for t in CsrAdj.from_scipy(a)])
    dense = torch.from_numpy(a.toarray()).to(DEV)
    g = torch.Generator().manual_seed(1)
    b = torch.randn(P, C, generator=g).to(DEV)
    bias = torch.randn(C, generator=g).to(DEV)
    np.testing.assert_allclose(spmm(adj, b, bias).cpu().numpy(), (dense @ b + bias).cpu().numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(spmm(adj, b, transposed=True).cpu().numpy(), (dense.t() @ b).cpu().numpy(), rtol=1e-5, atol=1e-5)
    rows = torch.randperm(P, generator=g)[:333].to(DEV)
    np.testing.assert_allclose(spmm(adj, b, None, rows).cpu().numpy(), (dense[rows] @ b).cpu().numpy(), rtol=1e-5, atol=1e-5)
    # autograd of the layer: all rows, a row subset, and a subset that names rows twice (a POI visited twice in a batch);
    # the subsets' transposed product both as the gather over the stored transpose and as the atomic scatter
    from mobgt_amd import forms
    rows_dup = torch.cat([rows, rows[:50], rows[:7]])
    for rws, gather in ((None, True), (rows, True), (rows, False), (rows_dup, True), (rows_dup, False)):
        with forms.using(sp_gather=gather):
            x = torch.randn(P, 64, generator=g).to(DEV)
            w = (torch.randn(64, C, generator=g) * 0.1).to(DEV)
            up = torch.randn(P if rws is None else rws.numel(), C, generator=g).to(DEV)
            xa, wa, ba = (t.clone().requires_grad_(True) for t in (x, w, bias))
            ref = (dense if rws is None else dense[rws]) @ (xa @ wa) + ba
            (ref * up).sum().backward()
            xb, wb, bb = (t.clone().requires_grad_(True) for t in (x, w, bias))
            out = _SpConvFn.apply(xb, wb, bb, adj, rws)
            (out * up).sum().backward()
            np.testing.assert_allclose(out.detach().cpu().numpy(), ref.detach().cpu().numpy(), rtol=1e-4, atol=1e-4)
            np.testing.assert_allclose(xb.grad.cpu().numpy(), xa.grad.cpu().numpy(), rtol=1e-3, atol=1e-3)
            np.testing.assert_allclose(bb.grad.cpu().numpy(), ba.grad.cpu().numpy(), rtol=1e-4, atol=1e-3)
            # dW goes through the bf16-operand weight-gradient kernel (K = P rows)
            scale = float(wa.grad.abs().max())
            np.testing.assert_allclose(wb.grad.cpu().numpy(), wa.grad.cpu().numpy(), rtol=0, atol=2e-2 * scale)
    assert bool((adj._rows_head == -1).all())                # the per-row lists are unthreaded again after every call


@pytest.mark.parametrize("C", [64, 128, 96, 256])
def test_spmm_row_widths_and_empty_rows(C):
    """csrc/spmm.hip: C = 64 / 128 take spmm_narrow_kernel (the wave's 4 / 2 lane groups gather different neighbours and meet in a
    shuffle), any other width the one-neighbour-per-instruction kernel; rows without neighbours (an isolated POI) give the bias;
    neighbour counts that are not multiples of the group count or of the unroll (1 .. 40 per row) exercise both loop tails."""
    from scipy import sparse
    P = 700
    rng = np.random.RandomState(C)
    rows_, cols_, vals_ = [], [], []
    for i in range(P):
        k = 0 if i % 17 == 0 else 1 + (i * 7) % 40
        cs = rng.choice(P, size=k, replace=False)
        rows_ += [i] * k
        cols_ += list(cs)
        vals_ += list(rng.rand(k).astype(np.float32) + 0.1)
    a = sparse.csr_matrix((np.array(vals_, np.float32), (np.array(rows_), np.array(cols_))), shape=(P, P))
    adj = CsrAdj(*[t.to(DEV) for t in CsrAdj.from_scipy(a)])
    dense = torch.from_numpy(a.toarray()).to(DEV)
    g = torch.Generator().manual_seed(C)
    b = torch.randn(P, C, generator=g).to(DEV)
    bias = torch.randn(C, generator=g).to(DEV)
    out = spmm(adj, b, bias)
    np.testing.assert_allclose(out.cpu().numpy(), (dense @ b + bias).cpu().numpy(), rtol=1e-5, atol=1e-5)
    assert torch.equal(out[0], bias) and torch.equal(out[17], bias)              # isolated rows
    sub = torch.randperm(P, generator=g)[:123].to(DEV)
    np.testing.assert_allclose(spmm(adj, b, None, sub).cpu().numpy(), (dense[sub] @ b).cpu().numpy(), rtol=1e-5, atol=1e-5)


def _cpu_batch(b):
    c = SimpleNamespace()
    for f in ("attn_bias", "rel_pos", "poi_pos", "edge_input", "x", "in_degree", "out_degree", "user", "y", "time_normal"):
        t = getattr(b, f).cpu()
        setattr(c, f, t.float() if t.dtype.is_floating_point else t.long())
    return c


def test_sparse_universe_model_matches_oracle_on_the_densified_universe():
    from mobgt_amd.model_fqandtoyo import Graphormer
    P = 1500
    uni = synth.make_sparse_universe(P=P, n_cat=20, n_user=1080, seed=2)
    dense = synth.densify(uni)
    torch.manual_seed(4)
    args = dict(workloads.COMMON, n_layers=2, hidden_dim=128, dataset_name="foursquaregraph", ffn_dim=256)
    model = Graphormer(universe=uni, num_bins=uni.num_bins + 2, **args).to(DEV).eval()
    coll = DeviceCollator(DEV, coords=uni.coords, bin_edges=uni.bin_edges)
    trajs = synth.make_batch_of_trajectories(seed=5, G=6, P=P, n_user=1080, cat_of_poi=uni.cat_of_poi, n_nodes=[40, 3, 17, 64, 9, 25])
    batch = coll(trajs)
    # distance bins from coordinates == np.digitize on the dense distance matrix
    x = batch.x[:, :, 0].cpu().numpy()
    want = np.digitize(dense.distance[x[:, :, None], x[:, None, :]], uni.bin_edges)
    want[(x[:, :, None] == 0) | (x[:, None, :] == 0)] = 0
    assert np.array_equal(batch.poi_pos.cpu().numpy().astype(np.int64), want)
    # G*N*2 <= P: the rows-only last layer; then the full-table path on a larger batch fraction
    assert batch.x.shape[0] * batch.x.shape[1] * 2 <= P
    consts = mo.fq_constants(dense, "foursquaregraph", diag_inverse=True, num_bins=uni.num_bins + 2)
    sd = {k: v.detach().float().cpu().clone().requires_grad_(True) for k, v in model.state_dict().items()}
    cb = _cpu_batch(batch)
    ref, _ = mo.graphormer_fq_forward(sd, cb, consts, n_layers=2, H=8, D=20)
    ref_loss = mo.gradient_tail_loss(ref, cb.y - 1, 0.2)
    ref_loss.backward()
    logits = model(batch)[0]
    np.testing.assert_allclose(logits.detach().cpu().numpy(), ref.detach().numpy(), rtol=2e-2, atol=2e-2)
    loss = model.training_step(batch, 0)
    np.testing.assert_allclose(float(loss.detach()), float(ref_loss.detach()), rtol=1e-3)
    loss.backward()
    for name in ("poi_distance_model.gcn.0.weight", "poi_distance_model.gcn.1.weight", "poi_distance_model.gcn.2.weight",
                 "poi_distance_model.gcn.1.bias", "poi_distance_model.gcn.2.bias"):
        got = dict(model.named_parameters())[name].grad.cpu().numpy().astype(np.float64)
        want = sd[name].grad.numpy().astype(np.float64)
        rel = np.sqrt(((got - want) ** 2).sum()) / np.sqrt((want ** 2).sum())
        assert rel <= 3e-2, (name, rel)


def test_big_workload_builds_and_steps_at_reduced_p():
    """workloads.build("big") end to end (CSR universe, coordinate bins, C = 256 / d = 32 / 12 layers) at P = 5 000 and
    N = 96 so that it runs in seconds: finite loss, parameters move."""
    from mobgt_amd.train import TrainStep
    uni, model, coll = workloads.build("big", DEV, seed=1, P=5000)
    trajs = synth.make_batch_of_trajectories(seed=8, G=4, P=5000, n_user=1080, cat_of_poi=uni.cat_of_poi, n_nodes=[96, 50, 7, 96])
    batches = [coll(trajs)]
    ts = TrainStep(model, batches, use_graph=True, seed=1)
    ts.prepare()
    p0 = ts.flat_params.tensor.detach().clone()
    losses = [float(ts.step(i)) for i in range(3)]
    assert all(np.isfinite(losses)), losses
    assert float((ts.flat_params.tensor.detach() - p0).abs().max()) > 0


def test_mask_gemm_matches_the_dense_normalised_adjacency():
    """csrc/maskgemm.hip: (D+I)^-1 (A+I) @ X and its transpose from a bitmask + row scale, against the dense fp32
    expression (model_fqandtoyo.py:481-486) with X rounded to bf16 (the kernel's MFMA operand), and the layer's autograd."""
    from mobgt_amd.modelGNN import MaskAdj, mask_gemm, _MaskConvFn
    from mobgt_amd.model_fqandtoyo import calculate_laplacian_matrix
    for P in (333, 1000):
        uni = synth.make_universe(P=P, n_cat=8, n_user=8, seed=P)
        dense = torch.from_numpy(calculate_laplacian_matrix(uni.graph_dist)).float().to(DEV)
        adj = MaskAdj(*[t.to(DEV) for t in MaskAdj.from_dense01(uni.graph_dist)])
        g = torch.Generator().manual_seed(P)
        dense01 = torch.from_numpy(np.asarray(uni.graph_dist) + np.eye(P)).float().to(DEV)
        for N in (16, 32, 48, 64):
            x = torch.randn(P, N, generator=g).to(DEV)
            xr = x.bfloat16().float()
            np.testing.assert_allclose(mask_gemm(adj, x).cpu().numpy(), (dense @ xr).cpu().numpy(), rtol=1e-4, atol=1e-5)
            want_t = dense01.t() @ (x * adj.scale[:, None]).bfloat16().float()     # (the operand's rows are scaled BEFORE rounding)
            got_t = mask_gemm(adj, x, transposed=True)
            np.testing.assert_allclose(got_t.cpu().numpy(), want_t.cpu().numpy(), rtol=1e-4, atol=1e-5)
        x = torch.randn(P, 16, generator=g).to(DEV)
        w = (torch.randn(16, 64, generator=g) * 0.2).to(DEV)
        b = torch.randn(64, generator=g).to(DEV)
        up = torch.randn(P, 64, generator=g).to(DEV)
        xa, wa, ba = (t.clone().requires_grad_(True) for t in (x, w, b))
        ref = dense @ (xa @ wa) + ba
        (ref * up).sum().backward()
        xb, wb, bb = (t.clone().requires_grad_(True) for t in (x, w, b))
        out = _MaskConvFn.apply(xb, wb, bb, adj)
        (out * up).sum().backward()
        for got, want, n in ((out, ref, "out"), (xb.grad, xa.grad, "dx"), (wb.grad, wa.grad, "dW"), (bb.grad, ba.grad, "db")):
            scale = float(want.detach().abs().max())
            np.testing.assert_allclose(got.detach().cpu().numpy(), want.detach().cpu().numpy(), rtol=0, atol=2e-2 * scale, err_msg=n)
    assert MaskAdj.from_dense01(uni.graph_dist * 2.0) is None       # not a 0/1 matrix: the dense path stays


@pytest.mark.gpu
@pytest.mark.parametrize("n,k0,training", [(300, 300, True), (300, 300, False), (37, 21, True), (513, 40, True), (300, 400, False)])
def test_small_gcn_single_launch_matches_the_layer_by_layer_path(n, k0, training, monkeypatch):
    """csrc/smallgcn.hip (the category GCN as one persistent launch each way) against the same GCN evaluated layer by
    layer (GraphConvolution + bias_act launches) and against plain torch fp32: same dropout mask, same values."""
    from mobgt_amd.modelGNN import GCN
    from mobgt_amd import ops
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(n)
    a = (torch.rand(n, n, generator=g) < 0.05).float() + torch.eye(n)
    a = (a / a.sum(1, keepdim=True)).to(dev)
    x = torch.rand(n, k0, generator=g).to(dev)
    ax, a_t = (a @ x).contiguous(), a.t().contiguous()
    net = GCN(k0, [16, 64], 32, dropout=0.1).to(dev).train(training)
    gout = torch.randn(n, 32, generator=g).to(dev)

    def run(single):
        monkeypatch.setenv("MOBGT_NO_SMALL_GCN", "0" if single else "1")
        torch.manual_seed(5)                                   # the host seed of the dropout site is drawn from torch's RNG
        net.zero_grad()
        out = net(x, a, ax, adj_t=a_t)
        out.backward(gout)
        return out.detach().clone(), [p.grad.clone() for p in net.parameters()]

    o1, g1 = run(True)
    o0, g0 = run(False)
    torch.testing.assert_close(o1, o0, rtol=2e-5, atol=2e-6)
    for (name, _), u, v in zip(net.named_parameters(), g1, g0):
        torch.testing.assert_close(u, v, rtol=2e-4, atol=2e-5 * float(v.abs().max()) + 1e-7, msg=lambda m: f"{name}: {m}")
    if not training:                                            # no dropout: plain torch is a second reference
        ws = [p.detach().clone().requires_grad_(True) for p in net.parameters()]
        h = torch.nn.functional.leaky_relu(ax @ ws[0] + ws[1], 0.2)
        h = torch.nn.functional.leaky_relu(a @ h @ ws[2] + ws[3], 0.2)
        ref = a @ h @ ws[4] + ws[5]
        ref.backward(gout)
        torch.testing.assert_close(o1, ref.detach(), rtol=2e-5, atol=2e-6)
        for u, w in zip(g1, ws):
            torch.testing.assert_close(u, w.grad, rtol=2e-4, atol=2e-5 * float(w.grad.abs().max()) + 1e-7)
    # the hand-over counter is bounded: a second call on fresh counters works, and so does a call inside a graph replay
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        net.zero_grad()
        monkeypatch.setenv("MOBGT_NO_SMALL_GCN", "0")
        net(x, a, ax, adj_t=a_t).backward(gout)
    s.synchronize()
    assert all(torch.isfinite(p.grad).all() for p in net.parameters())


@pytest.mark.gpu
@pytest.mark.parametrize("training", [True, False])
def test_gcn_hidden_layers_without_activation_launches_match_the_bias_act_path(training, monkeypatch):
    """modelGNN._ConvActFn (bias + LeakyReLU + dropout in the small GEMM's epilogue; their derivative applied while the
    backward's weight-gradient kernel and data-gradient GEMM load the incoming gradient) against the same GCN with
    separate mobgt_bias_act launches: same dropout masks, so values and every gradient agree (bf16 operand rounding of
    the weight gradients aside)."""
    from mobgt_amd.modelGNN import GCN, MaskAdj
    dev = torch.device("cuda")
    P = 1000
    g = torch.Generator().manual_seed(7)
    a01 = (torch.rand(P, P, generator=g) < 0.02)
    a01 = (a01 | a01.t()).float()
    a01.fill_diagonal_(0)
    madj = MaskAdj(*[t.to(dev) for t in MaskAdj.from_dense01(a01.numpy())])
    deg = a01.sum(1) + 1
    a = ((a01 + torch.eye(P)) / deg[:, None]).to(dev)
    x = torch.rand(P, 32, generator=g).to(dev)
    ax = (a @ x).contiguous()
    net = GCN(32, [16, 64], 128, dropout=0.3).to(dev).train(training)
    gout = torch.randn(P, 128, generator=g).to(dev)

    def run(fused):
        monkeypatch.setenv("MOBGT_NO_CONV_ACT", "0" if fused else "1")
        torch.manual_seed(5)
        net.zero_grad()
        out = net(x, a.bfloat16(), ax, adj_t=a.t().contiguous().bfloat16(), mask_adj=madj)
        out.backward(gout)
        return out.detach().clone(), [p.grad.clone() for p in net.parameters()]

    o1, g1 = run(True)
    o0, g0 = run(False)
    torch.testing.assert_close(o1, o0, rtol=2e-2, atol=2e-2 * float(o0.abs().max()))
    for (name, _), u, v in zip(net.named_parameters(), g1, g0):
        scale = float(v.abs().max()) + 1e-12
        assert float((u - v).abs().max()) <= 2e-2 * scale, (name, float((u - v).abs().max()), scale)
