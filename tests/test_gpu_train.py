"""`train.TrainStep` on a real MI355X: the graph-replayed optimizer trajectory against torch.optim.AdamW +
PolynomialDecayLR (model_fqandtoyo.py:1599-1616, lr.py:7-34), bf16 shadow-weight maintenance across checkpoint loads,
and the data-parallel invariant (identical parameters and Adam moments on every rank) with two ranks."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mobgt_amd import synth                                          # noqa: E402
from mobgt_amd.data import DeviceCollator, make_bin_table           # noqa: E402

DEV = "cuda"
ARGS = dict(n_layers=2, num_heads=8, hidden_dim=64, dropout_rate=0.1, intput_dropout_rate=0.1, weight_decay=0.01,
            ffn_dim=128, warmup_updates=4, tot_updates=100, peak_lr=1e-3, end_lr=1e-9, edge_type="multi_hop",
            multi_hop_max_dist=20, attention_dropout_rate=0.1, dataset_name="foursquaregraph")


def _setup(seed=0, **over):
    from mobgt_amd.model_fqandtoyo import Graphormer
    uni = synth.make_universe(P=400, n_cat=12, n_user=1080, seed=3)
    nb, _, table = make_bin_table(uni.distance)
    torch.manual_seed(seed)
    model = Graphormer(universe=uni, num_bins=nb + 2, bias_dtype=torch.bfloat16, gcn_dtype=torch.bfloat16,
                       act_dtype=torch.bfloat16, **dict(ARGS, **over)).to(DEV)
    coll = DeviceCollator(DEV, bin_table=table)
    batches = [coll(synth.make_batch_of_trajectories(seed=10 + i, G=4, P=400, n_user=1080, cat_of_poi=uni.cat_of_poi))
               for i in range(2)]
    return model, batches


@pytest.mark.parametrize("use_graph", [True, False])
def test_train_step_trajectory_matches_torch_adamw_and_polynomial_decay(use_graph):
    """Five steps at a realistic learning rate: feeding each step's gradient (as the step computed it) to
    torch.optim.AdamW + the reference's scheduler reproduces the parameters -- i.e. the first replayed step is AdamW's
    t = 1 on zero moments at lr(1), the k-th at lr(k) (the old warm-up consumed t = 1 on a stale gradient)."""
    from mobgt_amd.lr import PolynomialDecayLR
    from mobgt_amd.train import TrainStep
    model, batches = _setup()
    ts = TrainStep(model, batches, use_graph=use_graph, seed=5)
    ts.prepare()
    assert float(ts.exp_avg.abs().max()) == 0.0 and float(ts.exp_avg_sq.abs().max()) == 0.0
    ref = torch.nn.Parameter(ts.flat_params.tensor.detach().double().clone())
    opt = torch.optim.AdamW([ref], lr=ARGS["peak_lr"], weight_decay=ARGS["weight_decay"])
    sched = PolynomialDecayLR(opt, ARGS["warmup_updates"], ARGS["tot_updates"], ARGS["peak_lr"], ARGS["end_lr"], 1.0)
    for i in range(6):
        ts.step(i)
        ref.grad = ts.flat.flat.double().clone()
        opt.step()
        sched.step()
        got, want = ts.flat_params.tensor.detach().double().cpu().numpy(), ref.detach().cpu().numpy()
        # fp32 parameters vs a float64 reference: an ulp or two of the parameter per step (values reach |4|)
        np.testing.assert_allclose(got, want, rtol=1.5e-7 * (i + 1), atol=2e-7 * (i + 1) + 1e-6 * ARGS["peak_lr"])
    if ts.shadow_flat is not None:
        assert torch.equal(ts.shadow_flat, ts.flat_params.tensor.detach().bfloat16())


def test_shadows_follow_checkpoint_loads_made_after_the_trainer_exists():
    """TrainStep owns the fused layers' bf16 shadow weights; load_lightning_checkpoint after its
    construction must refresh them, otherwise the next forward multiplies with the OLD weights."""
    from mobgt_amd import checkpoint
    from mobgt_amd.train import TrainStep
    model, batches = _setup()
    ts = TrainStep(model, batches, use_graph=False, seed=5)
    assert ts.shadow_flat is not None and all(getattr(l, "_shadow_external", False) for l in model.layers)
    sd = {k: (v.detach().cpu() * 1.5 if "ffn.layer1.weight" in k or "linear_q.weight" in k else v.detach().cpu())
          for k, v in model.state_dict().items()}
    checkpoint.load_lightning_checkpoint(model, {"state_dict": sd})
    for layer in model.layers:
        wqkv = layer.self_attention.fuse_qkv_storage()[0]
        assert torch.equal(layer._shadows[0], wqkv.detach().bfloat16())
        assert torch.equal(layer._shadows[4], layer.ffn.layer1.weight.detach().bfloat16())
    model.eval()
    with torch.no_grad():
        a = model(batches[0])[0].clone()
        ts.shadow_flat.zero_()                      # prove the forward really reads the shadows ...
        b = model(batches[0])[0].clone()
        ts.sync_shadows()                           # ... and that sync_shadows restores them
        c = model(batches[0])[0]
    assert not torch.equal(a, b) and torch.equal(a, c)


def test_out_of_range_indices_raise_like_nn_embedding():
    """the gather kernels do not bounds-check; the model validates each batch object once."""
    model, batches = _setup()
    model.eval()
    b = batches[0]
    model(b)
    import copy
    bad = copy.copy(b)
    bad.in_degree = b.in_degree.clone()
    bad.in_degree[0, 0] = 128
    bad._mobgt_validated = None
    with pytest.raises(IndexError):
        model(bad)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_two_ranks(tmp_path, steps, extra_env=None):
    port = _free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY="0", **(extra_env or {}))
        procs.append(subprocess.Popen([sys.executable, os.path.join(os.path.dirname(__file__), "_ddp_worker.py"), str(tmp_path), str(steps)],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(o.decode(errors="replace"))
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
    return [torch.load(os.path.join(tmp_path, f"rank{r}.pt")) for r in range(2)]


def _run_one_rank(tmp_path, steps, extra_env=None):
    port = _free_port()
    env = dict(os.environ, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
               HSA_ENABLE_IPC_MODE_LEGACY="0", **(extra_env or {}))
    p = subprocess.Popen([sys.executable, os.path.join(os.path.dirname(__file__), "_ddp_worker.py"), str(tmp_path), str(steps)],
                         env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    try:
        o, _ = p.communicate(timeout=300)
    except subprocess.TimeoutExpired:
        p.kill()
        raise
    assert p.returncode == 0, o.decode(errors="replace")[-4000:]
    return torch.load(os.path.join(tmp_path, "rank0.pt"))


def test_rccl_branch_executes_on_one_gpu(tmp_path):
    """VERDICT r3 (a15, "the nccl branch has never executed anywhere"): a process group of ONE rank over RCCL ("nccl") on this
    box's GPU, `MOBGT_FORCE_COMM=1` so that TrainStep takes its data-parallel path: communicator creation with `device_id`,
    the parameter broadcast, the layout all-gather, then every form of the data-parallel step (train.TrainStep.__init__):
      fp32 / bf16   the default -- ONE graph per batch with the all-reduce captured on the step's own stream (in place, then
                    through the bf16 exchange buffer);
      ovl / ovl16   MOBGT_DDP_OVERLAP=1, MOBGT_DDP_PARTS=3: three step graphs per batch, the layer-wise buckets' asynchronous
                    all-reduces on RCCL's stream beside the replays;
      host          MOBGT_DDP_HOST_EXCHANGE=1: the all-reduce issued by the host between the backward and the optimizer graph.
    A sum over one rank changes nothing: losses / gradients must be those of the same worker WITHOUT the forced exchange, up to
    what two runs of one step differ by (f32 atomics in front of bf16 rounding points) -- bf16 exchange: up to bf16 rounding."""
    runs = {}
    ovl = {"MOBGT_FORCE_COMM": "1", "MOBGT_DDP_OVERLAP": "1", "MOBGT_DDP_PARTS": "3"}
    for tag, env in (("plain", {}), ("fp32", {"MOBGT_FORCE_COMM": "1"}), ("bf16", {"MOBGT_FORCE_COMM": "1", "MOBGT_TEST_GRAD_COMM": "bf16"}),
                     ("ovl", ovl), ("ovl16", dict(ovl, MOBGT_TEST_GRAD_COMM="bf16")),
                     ("host", {"MOBGT_FORCE_COMM": "1", "MOBGT_DDP_HOST_EXCHANGE": "1"})):
        d = tmp_path / tag
        d.mkdir()
        runs[tag] = _run_one_rank(d, 3, env)
    a, b, c = runs["plain"], runs["fp32"], runs["bf16"]
    for tag in ("ovl", "ovl16", "host"):
        r = runs[tag]
        assert r["backend"] == "nccl" and r["forced"] and not r["one_graph"]
        assert r["overlap"] == (tag != "host") and (r["parts"] >= 2) == (tag != "host")
        assert all(np.isfinite(r["losses"]))
        np.testing.assert_allclose(r["losses"], a["losses"], rtol=2e-2)
        assert float((r["grads"] - a["grads"]).norm() / a["grads"].norm()) < 5e-2
    print("backend", b["backend"], "one graph", b["one_graph"], "losses", a["losses"], b["losses"], c["losses"])
    assert a["backend"] == b["backend"] == c["backend"] == "nccl"
    assert not a["forced"] and not a["overlap"] and not a["one_graph"]
    assert b["forced"] and b["one_graph"] and not b["overlap"] and b["comm_dtype"] is None
    assert c["forced"] and c["one_graph"] and c["comm_dtype"] == "torch.bfloat16"
    for r in (b, c):
        assert all(np.isfinite(r["losses"]))
        np.testing.assert_allclose(r["losses"], a["losses"], rtol=2e-2)
        rel = float((r["grads"] - a["grads"]).norm() / a["grads"].norm())
        assert rel < 5e-2, rel


def test_bf16_gradient_exchange_tracks_the_fp32_exchange(tmp_path):
    """`TrainStep(grad_comm_dtype=torch.bfloat16)` (half the all-reduce bytes): replicas stay bit-identical, and after three
    steps the parameters are those of the fp32 exchange up to bf16 rounding of the exchanged gradients: the update per step
    is lr * m_hat / sqrt(v_hat) ~ lr (AdamW normalises the gradient scale away), so a relative gradient error of 2^-8 moves
    a parameter by ~lr * 2^-8; bound: 5 % of the total parameter movement."""
    d32, d16 = tmp_path / "f32", tmp_path / "bf16"
    d32.mkdir()
    d16.mkdir()
    a32, _ = _run_two_ranks(d32, 3)
    a16, b16 = _run_two_ranks(d16, 3, {"MOBGT_TEST_GRAD_COMM": "bf16"})
    for k in ("params", "exp_avg", "exp_avg_sq", "grads"):
        assert torch.equal(a16[k], b16[k]), k
    rel_g = float((a16["grads"] - a32["grads"]).norm() / a32["grads"].norm())
    assert rel_g < 5e-2, rel_g      # (third-step gradients after two slightly different updates; same dropout masks; measured 2.1 %)
    dp = float((a16["params"] - a32["params"]).norm())
    # the worker's schedule (peak 1e-3, 4 warm-up updates): lr = 2.5e-4, 5e-4, 7.5e-4 -> every parameter moves by <= 1.5e-3
    n = a32["params"].numel()
    assert dp < 0.05 * 1.5e-3 * n ** 0.5, (dp, n)


@pytest.mark.parametrize("form", ["default", "overlap"])
def test_two_rank_train_step_keeps_replicas_identical(tmp_path, form):
    """Two data-parallel ranks of TrainStep (RCCL when the box has two GPUs, otherwise gloo with both ranks on cuda:0):
    after three steps on different per-rank data every rank holds bit-identical parameters, Adam moments and bf16
    shadows, and the averaged gradient buffer is the same on both.  `default`: one graph with the captured all-reduce over
    RCCL, the host-issued exchange over gloo; `overlap`: MOBGT_DDP_OVERLAP=1 with three layer-wise parts."""
    a, b = _run_two_ranks(tmp_path, 3, {} if form == "default" else {"MOBGT_DDP_OVERLAP": "1", "MOBGT_DDP_PARTS": "3"})
    print("backend", a["backend"], "overlap", a["overlap"], "one graph", a["one_graph"], "losses", a["losses"], b["losses"])
    assert a["overlap"] == b["overlap"] == (form == "overlap")
    assert a["one_graph"] == (form == "default" and a["backend"] == "nccl")
    assert a["losses"] != b["losses"]                          # different data per rank
    for k in ("params", "exp_avg", "exp_avg_sq", "grads", "shadow"):
        assert torch.equal(a[k], b[k]), k
    assert float(a["exp_avg"].abs().max()) > 0 and all(np.isfinite(a["losses"]))


@pytest.mark.parametrize("comm", ["fp32", "bf16"])
def test_exchanged_gradient_is_the_mean_of_the_two_ranks_gradients(tmp_path, comm):
    """the two-rank test above shows the replicas AGREE; this one shows WHAT they agree on.  After one step of
    two data-parallel ranks on different batches, the gradient buffer every rank holds must be (g_rank0 + g_rank1) / 2 --
    entry.py:141,161's DDP mean -- where g_r is the gradient ONE process computes alone on rank r's batch from the same
    (broadcast) initial parameters and the same dropout stream.  fp32 exchange in place and the bf16 exchange buffer
    (`grad_comm_dtype`).  Bounds: relative L2 of the whole flat buffer <= 1e-5 (fp32 exchange; measured 2e-8: the solo runs
    reproduce the ranks' gradients to f32 round-off) / 5e-3 (bf16 buffer: 2^-9 per entry; measured 2.3e-3); 99.9 % of the entries
    within 0.1 rms + 5 %; and the buffer is far from either rank's own gradient and from their SUM (a missing or un-averaged
    exchange)."""
    env = {"MOBGT_TEST_GRAD_COMM": "bf16"} if comm == "bf16" else {}
    d2, d0, d1 = tmp_path / "two", tmp_path / "solo0", tmp_path / "solo1"
    for d in (d2, d0, d1):
        d.mkdir()
    a, b = _run_two_ranks(d2, 1, env)
    s0 = _run_one_rank(d0, 1, {"MOBGT_TEST_DATA_RANK": "0"})
    s1 = _run_one_rank(d1, 1, {"MOBGT_TEST_DATA_RANK": "1"})
    assert torch.equal(a["grads"], b["grads"])
    assert a["losses"] != b["losses"] and abs(a["losses"][0] - s0["losses"][0]) < 1e-3 * abs(s0["losses"][0]) \
        and abs(b["losses"][0] - s1["losses"][0]) < 1e-3 * abs(s1["losses"][0])      # each rank computed ITS batch's loss
    g, g0, g1 = a["grads"].double(), s0["grads"].double(), s1["grads"].double()
    mean = (g0 + g1) / 2
    rel = float((g - mean).norm() / mean.norm())
    print("backend", a["backend"], "one graph", a["one_graph"], "comm dtype", a["comm_dtype"], "relative L2 to the mean %.2e" % rel,
          " to rank 0 alone %.2f  rank 1 alone %.2f  the sum %.2f" % tuple(float((g - x).norm() / x.norm()) for x in (g0, g1, g0 + g1)))
    assert rel <= (5e-3 if comm == "bf16" else 1e-5), rel       # (measured: 2.3e-3 / 2.2e-8)
    nz = mean != 0
    rms = float(mean[nz].pow(2).mean().sqrt())
    ratio = ((g - mean).abs()[nz] / (0.1 * rms + 0.05 * mean[nz].abs()))
    assert float(torch.quantile(ratio[:: max(1, ratio.numel() // 1000000)], 0.999)) <= 1.0
    assert float(g[~nz].abs().max()) <= 1e-3 * rms if bool((~nz).any()) else True
    for other in (g0, g1, g0 + g1):
        assert float((g - other).norm() / other.norm()) > 0.2


def test_bench_launches_two_ranks_and_reports_them(tmp_path):
    """`python bench.py --gpus 2` as the driver calls it (no torch.distributed environment): the script launches its own two
    ranks through torch.distributed.run, both take part in the gradient all-reduce, rank 0 prints ONE JSON line.  On a
    one-GPU box MOBGT_TEST_SHARED_GPU=1 puts both ranks on cuda:0 over gloo -- the launcher, the rendezvous, the bucketed
    pool dealing, the two-phase overlapped step and the exposed-all-reduce measurement are the code an 8-GPU node runs;
    only the collective's transport differs (VERDICT r2 #5a)."""
    import json
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    if torch.cuda.device_count() < 2:
        env["MOBGT_TEST_SHARED_GPU"] = "1"
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "5", "--warmup", "2", "--full", "--no-cpu-baseline",
           "--no-stress", "--no-parity", "--no-gemm-autotune", "--n-batches", "2"]
    r = subprocess.run(cmd, env=env, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0, out[-2000:] + r.stderr.decode(errors="replace")[-4000:]
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out[-2000:]
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["comm_ranks"] == 2 and j["config"]["global_batch"] == 32 and j["scaling"] == "weak"
    # the line says which transport carried the gradients; `rccl_ranks` is filled only by a real RCCL ("nccl") run
    if env.get("MOBGT_TEST_SHARED_GPU") == "1":
        assert j["comm_backend"] == "gloo" and j["rccl_ranks"] is None
    else:
        assert j["comm_backend"] == "nccl" and j["rccl_ranks"] == 2
    assert j["steps"] == 5 and j["value"] > 0 and np.isfinite(j["final_loss"]) and j["allreduce_exposed_us"] is not None
    assert j["long_run"]["steps"] == 200
    # (round 6) the form of the data-parallel step was MEASURED on this job's ranks -- one graph / two-phase overlap / three parts,
    # 20 steps each behind a barrier, max over ranks -- and agreed on across them (train.choose_ddp_form)
    assert set(j["ddp_form_ms_per_step"]) == {"one_graph", "overlap_2", "overlap_3"} and j["ddp_form"] in j["ddp_form_ms_per_step"]
    assert all(v > 0 and np.isfinite(v) for v in j["ddp_form_ms_per_step"].values())
    assert j["ddp_form_ms_per_step"][j["ddp_form"]] == min(j["ddp_form_ms_per_step"].values())
    print("forms (ms / step):", j["ddp_form_ms_per_step"], "->", j["ddp_form"], "| exposed all-reduce", j["allreduce_exposed_us"], "us")



def test_encoder_input_backward_as_one_launch_equals_the_three_launches(monkeypatch):
    """csrc/tokbwd.hip (assemble_tokens' backward + the data gradients of FuseEmbeddings-4 / -2, parked across three autograd
    nodes and run as ONE launch inside the trainer's backward) against the three launches (MOBGT_NO_TOKEN_BWD_CHAIN=1): every
    parameter gradient of one dropout-on S-FSQ batch, same masks; f32 products in another summation order.  The first pass
    takes the one launch (mobgt_token_bwd_chain is called once), the second never."""
    from mobgt_amd import _lib, ops, workloads
    from mobgt_amd.step_state import STEP
    uni, model, coll = workloads.build("fsq", "cuda", seed=1, model_overrides=dict(n_layers=2))
    batch = coll(workloads.make_pool("fsq", 1, 16, uni)[0])
    model.train()
    sd = torch.zeros(1, dtype=torch.int64, device="cuda")
    ops.set_dropout_state(sd, 99)
    for m in model.modules():
        if hasattr(m, "seed_dev"):
            m.seed_dev = sd
    res = []
    launches = []
    real = _lib.lib()

    class _Spy:
        def __getattr__(self, name):
            if name == "mobgt_token_bwd_chain":
                launches.append(name)
            return getattr(real, name)
    monkeypatch.setattr(_lib, "lib", lambda: _Spy())
    try:
        for off in ("0", "1"):
            monkeypatch.setenv("MOBGT_NO_TOKEN_BWD_CHAIN", off)
            del launches[:]
            for p in model.parameters():
                p.grad = None
            with ops.recording_wgrads():             # (flushes behind the body)
                loss = model.training_step(batch, 0)
                parked_before = len(STEP.token_pending)
                loss.backward()
                assert not STEP.token_pending, "the parked chain must have been completed inside backward"
            torch.cuda.synchronize()
            res.append({n: p.grad.detach().float().clone() for n, p in model.named_parameters() if p.grad is not None})
            assert parked_before == 0
            print("MOBGT_NO_TOKEN_BWD_CHAIN=%s: %d mobgt_token_bwd_chain launch(es)" % (off, len(launches)))
            assert len(launches) == (1 if off == "0" else 0), (off, launches)
    finally:
        ops.set_dropout_state(None, 0)
    a, b = res
    assert a.keys() == b.keys() and len(a) > 50
    worst = 0.0
    for n in a:
        if n.endswith("linear_k.bias"):
            continue            # exactly 0 in exact arithmetic (softmax is shift-invariant over keys): round-off on both sides
        sc = float(b[n].abs().max())
        err = float((a[n] - b[n]).abs().max())
        worst = max(worst, err / (sc + 1e-30))
        # the parameters whose gradient flows THROUGH the fused launch are held to 2e-3 (f32 atomics of the scatters land in another
        # order from run to run: ~5e-4); the rest of the model only has to be the same step (run-to-run atomics noise, up to 1e-2
        # on tables with tiny gradients)
        through = n.split(".")[0] in ("embed_fuse_model4", "embed_fuse_model2", "poi_distance_model", "poi_cat_model", "time_embed_model_48",
                                      "in_degree_encoder", "out_degree_encoder", "fre_embed_model", "pos_embed", "graph_token")
        assert err <= (2e-3 if through else 2e-2) * sc + 1e-9, (n, err, sc)
    print("largest relative difference %.2e" % worst)
    # the one-launch form really ran: its registration exists for this forward pass and the switch removes it
    assert STEP.token_chain is None                             # (last pass ran with the switch on)
    monkeypatch.setenv("MOBGT_NO_TOKEN_BWD_CHAIN", "0")
    model.training_step(batch, 0)
    assert STEP.token_chain is not None


def test_bias_tables_backward_as_passenger_of_the_category_gcn_launch(monkeypatch):
    """mobgt_small_gcn_bwd_bias: the bias tables' backward (csrc/bias.hip: build_bias_bwd_body) carried by the category GCN's
    backward launch as passenger workgroups, against its own launch (MOBGT_NO_BIAS_BWD_PASSENGER=1): the gradients of the five
    bias tables and of the category GCN's weights on a dropout-on S-FSQ batch (f32 atomics in another order: ~5e-4)."""
    from mobgt_amd import ops, workloads
    uni, model, coll = workloads.build("fsq", "cuda", seed=1, model_overrides=dict(n_layers=2))
    batch = coll(workloads.make_pool("fsq", 1, 16, uni)[0])
    model.train()
    sd = torch.zeros(1, dtype=torch.int64, device="cuda")
    ops.set_dropout_state(sd, 99)
    for m in model.modules():
        if hasattr(m, "seed_dev"):
            m.seed_dev = sd
    res, took = [], []
    real_take = ops.take_bias_bwd_job

    def spy():
        j = real_take()
        took.append(j is not None)
        return j
    monkeypatch.setattr(ops, "take_bias_bwd_job", spy)
    try:
        for off in ("0", "1"):
            monkeypatch.setenv("MOBGT_NO_BIAS_BWD_PASSENGER", off)
            for p in model.parameters():
                p.grad = None
            model.training_step(batch, 0).backward()
            torch.cuda.synchronize()
            res.append({n: p.grad.detach().float().clone() for n, p in model.named_parameters() if p.grad is not None})
    finally:
        ops.set_dropout_state(None, 0)
    assert took == [True, False], took                 # the passenger form ran in the first pass, not in the second
    a, b = res
    names = [n for n in a if n.split(".")[0] in ("rel_pos_encoder", "poi_pos_encoder", "edge_encoder", "edge_dis_encoder",
                                                  "graph_token_virtual_distance", "poi_cat_model")]
    assert len(names) >= 8, names
    for n in names:
        sc = float(b[n].abs().max())
        err = float((a[n] - b[n]).abs().max())
        # (the edge tables' entries are multiples of fp16's smallest subnormal at the plain loss -- the emulated round trip of
        #  model_fqandtoyo.py:1178-1198 --: an ulp of difference in the f32 sums moves an entry by one or two of those steps)
        quanta = 2 * 5.97e-8 if n.startswith("edge_") else 0.0
        assert sc > 0 and err <= 2e-3 * sc + quanta, (n, err, sc)


def test_encoder_input_forward_in_one_launch_is_bit_identical_to_the_four_launches(monkeypatch):
    """Round 4: gather + FuseEmbeddings-2 / -4 + token assembly + first QKV as ONE launch (mobgt_token_fwd_chain; the first three
    autograd nodes only record their launches, ops.token_fwd_deferral) against the four launches (MOBGT_NO_TOKEN_FWD_CHAIN=1):
    the same f32 MFMA order, the same masks -> the encoder input, its bf16 copy, the first layer's QKV and every buffer the
    backward pass reads (pt, x4, nf, add: seen through the gradients) are bit-identical, in eval mode and with the dropouts on;
    eval logits bit-identical; gradients to the run-to-run noise of the atomics in the backward pass.  (Train-mode LOGITS are
    not compared: the encoder layers draw fresh host seeds per forward pass.)"""
    from mobgt_amd import ops, workloads
    from mobgt_amd.step_state import STEP
    uni, model, coll = workloads.build("fsq", "cuda", seed=1, model_overrides=dict(n_layers=2))
    batch = coll(workloads.make_pool("fsq", 1, 16, uni)[0])
    seen = []
    real_nf = model.node_features

    def spy(*a, **k):
        out = real_nf(*a, **k)
        seen.append((out.detach().float().clone(), out._mobgt_act.float().clone(), out._mobgt_qkv.float().clone()))
        return out
    monkeypatch.setattr(model, "node_features", spy)
    res = {}
    for mode in ("eval", "train"):
        model.train(mode == "train")
        for off in ("0", "1"):
            monkeypatch.setenv("MOBGT_NO_TOKEN_FWD_CHAIN", off)
            ops.set_dropout_state(torch.tensor([3], dtype=torch.int64, device="cuda"), 11)
            for p in model.parameters():
                p.grad = None
            before = STEP.token_fwd_fused_calls
            del seen[:]
            try:
                logits = model(batch)[0]
                loss = model.training_step(batch, 0)
                loss.backward()
            finally:
                ops.set_dropout_state(None, None)
            torch.cuda.synchronize()
            took = STEP.token_fwd_fused_calls - before
            assert took == (2 if off == "0" else 0), (mode, off, took)
            res[(mode, off)] = (logits.detach().float().clone(), seen[0], {n: p.grad.detach().float().clone()
                                                                          for n, p in model.named_parameters() if p.grad is not None})
        (la, sa, ga), (lb, sb, gb) = res[(mode, "0")], res[(mode, "1")]
        for x, y, what in zip(sa, sb, ("encoder input", "bf16 copy", "first qkv")):
            assert torch.equal(x, y), (mode, what)
        if mode == "eval":
            assert torch.equal(la, lb)
            assert ga.keys() == gb.keys()
            for n in ga:
                if n.endswith("linear_k.bias"):
                    continue        # exactly 0 in exact arithmetic (softmax is shift-invariant over keys): round-off on both sides
                d = float((ga[n] - gb[n]).norm() / (gb[n].norm() + 1e-30))
                assert d < 5e-3, (mode, n, d)


def test_forward_passengers_of_the_category_gcn_launch_change_nothing(monkeypatch):
    """The weight pack, the hop table's forward and the gather indices carried by the category GCN's forward launch
    (mobgt_small_gcn_fwd_pack; the model runs that launch first) against their own launches (MOBGT_NO_PACK_PASSENGER=1,
    MOBGT_NO_FRONT_PASSENGERS=1): bit-identical logits, hop table and indices -- and the launch did take the jobs.  Round 4: the
    same switch pair covers the distance GCN's first layer riding in the bias assembly's launch (MOBGT_NO_L0_RIDE=1)."""
    from mobgt_amd import ops, workloads
    uni, model, coll = workloads.build("fsq", "cuda", seed=1, model_overrides=dict(n_layers=2))
    batch = coll(workloads.make_pool("fsq", 1, 16, uni)[0])
    model.eval()
    took = []
    real_take = ops.take_front_jobs

    def spy():
        hop, ni = real_take()
        took.append((hop is not None, ni is not None))
        return hop, ni
    monkeypatch.setattr(ops, "take_front_jobs", spy)
    outs = []
    for off in ("0", "1"):
        monkeypatch.setenv("MOBGT_NO_FRONT_PASSENGERS", off)
        monkeypatch.setenv("MOBGT_NO_PACK_PASSENGER", off)
        monkeypatch.setenv("MOBGT_NO_L0_RIDE", off)        # (round 4: the distance GCN's first layer in the bias assembly's launch)
        with torch.no_grad():
            logits = model(batch)[0]
            hop = model.hop_table(batch)                         # (direct calls: launched at once)
            idx, real, _ = model.gather_indices(batch)
        torch.cuda.synchronize()
        outs.append((logits.float().clone(), hop.clone(), idx.clone(), real.clone()))
    # (the GCN's launch looks, then the model's flush_front: two looks per pass; the jobs are found by the first look of pass 1)
    assert took == [(True, True), (False, False), (False, False), (False, False)], took
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert torch.isfinite(outs[0][0]).all()


def test_long_batch_weight_gradients_sum_their_split_k_partials_in_one_launch(monkeypatch):
    """Round 4: past 4 096 rows the layers' weight gradients are the library's batched GEMMs over row slices + a sum over the
    slices; inside a train step the sums are parked and run as ONE launch into the gradients' sinks at the flush
    (mobgt_partial_sum_multi; S-BIG: 36 `.sum(0)` launches per step).  Against the immediate sums (MOBGT_NO_PSUM_DEFER=1) from
    one fixed state: the layers' weight gradients agree as closely as two runs of one form; the launch happened."""
    from mobgt_amd import _lib, workloads, synth
    from mobgt_amd.train import TrainStep
    uni, model, coll = workloads.build("fsq", DEV, seed=1, P=1500, model_overrides=dict(n_layers=2))
    batch = coll(synth.make_batch_of_trajectories(seed=5, G=8, P=1500, n_user=1080, cat_of_poi=uni.cat_of_poi, n_nodes=[560] * 8))
    ts = TrainStep(model, [batch], use_graph=False, seed=1)
    ts.prepare()
    seen = []
    real = _lib.lib()

    class _Spy:
        def __getattr__(self, name):
            if name == "mobgt_partial_sum_multi":
                seen.append(name)
            return getattr(real, name)
    monkeypatch.setattr(_lib, "lib", lambda: _Spy())
    state = _state_of(ts)
    names = {id(p): n for n, p in model.named_parameters()}
    pick = [n for n in names.values() if n.startswith("layers.") and n.endswith(".weight") and ("linear_" in n or "layer1" in n or "layer2" in n
                                                                                                  or "output_layer" in n)]
    assert len(pick) == 12, pick

    def grads():
        del seen[:]
        g, loss = _fixed_step_grads(ts, state)
        by = {names[id(p)]: v.detach().clone() for p, v in zip(ts.flat.params, ts.flat.views)}
        return {n: by[n] for n in pick}, loss, len(seen)
    monkeypatch.delenv("MOBGT_NO_PSUM_DEFER", raising=False)
    ga, la, na = grads()
    ga2, _, _ = grads()
    monkeypatch.setenv("MOBGT_NO_PSUM_DEFER", "1")
    gb, lb, nb = grads()
    assert na == 1 and nb == 0, (na, nb)
    assert abs(la - lb) <= 2e-5 * abs(lb)
    for n in pick:
        rep = float((ga2[n] - ga[n]).norm() / (ga[n].norm() + 1e-30))
        rel = float((gb[n] - ga[n]).norm() / (ga[n].norm() + 1e-30))
        print("%-44s parked vs immediate relL2 %.2e (two runs of one form %.2e)" % (n, rel, rep))
        assert float(ga[n].abs().max()) > 0 and rel < max(3 * rep, 3e-3), (n, rel, rep)


def test_stock_tail_as_one_grid_gives_the_gradients_of_its_two_launches(monkeypatch):
    """Round 4: the backward of the stock encoder input and the hop table's backward (1 537 edge ids: too wide for the grouped
    weight-gradient launch's hop slot) are parked by the trainer's backward pass and issued as ONE grid at the flush
    (mobgt_stock_tail_bwd, csrc/layer.hip stock_tail_kernel) -- against their own launches (MOBGT_NO_STOCK_TAIL=1), from one
    fixed state: the gradients of the six tables agree as closely as two runs of ONE form do (f32 atomics in varying order),
    and the launch did happen once per step."""
    from mobgt_amd import _lib, workloads
    from mobgt_amd.train import TrainStep
    uni, model, coll = workloads.build("fsq", DEV, seed=1, variant="stock", model_overrides=dict(n_layers=2))
    batches = [coll(t) for t in workloads.make_pool("fsq", 1, 16, uni)]
    ts = TrainStep(model, batches, use_graph=False, seed=1)
    ts.prepare()
    seen = []
    real = _lib.lib()

    class _Spy:
        def __getattr__(self, name):
            if name in ("mobgt_stock_tail_bwd", "mobgt_stock_tokens_bwd", "mobgt_hop_table_bwd"):
                seen.append(name)
            return getattr(real, name)
    monkeypatch.setattr(_lib, "lib", lambda: _Spy())
    state = _state_of(ts)
    names = {id(p): n for n, p in model.named_parameters()}
    tabs = ("atom_encoder.weight", "in_degree_encoder.weight", "out_degree_encoder.weight", "graph_token.weight",
            "edge_encoder.weight", "edge_dis_encoder.weight")

    def grads():
        del seen[:]
        g, loss = _fixed_step_grads(ts, state)
        by = {names[id(p)]: v.detach().clone() for p, v in zip(ts.flat.params, ts.flat.views)}
        return {n: by[n] for n in tabs}, loss, list(seen)
    monkeypatch.delenv("MOBGT_NO_STOCK_TAIL", raising=False)
    ga, la, sa = grads()
    ga2, _, _ = grads()
    monkeypatch.setenv("MOBGT_NO_STOCK_TAIL", "1")
    gb, lb, sb = grads()
    assert sa == ["mobgt_stock_tail_bwd"], sa
    assert sorted(sb) == ["mobgt_hop_table_bwd", "mobgt_stock_tokens_bwd"], sb
    assert abs(la - lb) <= 2e-5 * abs(lb)
    for n in tabs:
        rep = float((ga2[n] - ga[n]).norm() / (ga[n].norm() + 1e-30))
        rel = float((gb[n] - ga[n]).norm() / (ga[n].norm() + 1e-30))
        print("%-28s one grid vs two launches relL2 %.2e (two runs of one form %.2e)" % (n, rel, rep))
        assert float(ga[n].abs().max()) > 0 and rel < max(3 * rep, 3e-3), (n, rel, rep)
    assert float(ga["atom_encoder.weight"][0].abs().max()) == 0.0 and float(ga["edge_encoder.weight"][0].abs().max()) == 0.0   # padding rows


@pytest.mark.parametrize("use_graph", [False, True])
def test_parameter_reached_twice_per_pass_gets_no_gradient_sink(use_graph):
    """gradient sinks are handed to the op that asks in its forward and written as that op's own buffer,
    also by launches deferred to the end of the backward pass.  A Linear applied TWICE per forward has two producers of its
    weight gradient; with a sink both would write one buffer and autograd would add that buffer to itself (2 x one
    contribution, or garbage under deferral).  `train.used_parameters` counts the requests per pass and leaves such a parameter
    out of `ops.set_grad_sinks`: the gradient must be the SUM of both applications -- checked against torch's own autograd."""
    import torch.nn.functional as F
    from mobgt_amd import ops
    from mobgt_amd.train import TrainStep

    class Tied(torch.nn.Module):
        peak_lr, end_lr, warmup_updates, tot_updates, weight_decay = 1e-3, 1e-9, 2, 10, 0.0

        def __init__(self):
            super().__init__()
            torch.manual_seed(5)
            self.a = torch.nn.Linear(64, 64)
            self.b = torch.nn.Linear(64, 32)

        def training_step(self, x, idx):
            h = ops.linear_splitk(x, self.a.weight, self.a.bias, bf16_wgrad=True, slope=0.2)
            h = ops.linear_splitk(h, self.a.weight, self.a.bias, bf16_wgrad=True, slope=0.2)      # the same layer again
            y = ops.linear_splitk(h, self.b.weight, self.b.bias, bf16_wgrad=True)
            return (y * y).mean()

    model = Tied().to(DEV)
    x = torch.randn(96, 64, generator=torch.Generator().manual_seed(1)).to(DEV)
    ts = TrainStep(model, [x], use_graph=use_graph, seed=3)
    assert getattr(model.a.weight, "_mobgt_multi_use") and getattr(model.a.bias, "_mobgt_multi_use")
    assert not getattr(model.b.weight, "_mobgt_multi_use")
    assert ops.grad_sink(model.a.weight) is None and ops.grad_sink(model.b.weight) is not None
    w0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    ts.prepare()
    ts.step(0)
    ref = Tied().to(DEV)
    ref.load_state_dict(w0)
    h = F.leaky_relu(F.linear(x, ref.a.weight, ref.a.bias), 0.2)
    h = F.leaky_relu(F.linear(h, ref.a.weight, ref.a.bias), 0.2)
    y = F.linear(h, ref.b.weight, ref.b.bias)
    (y * y).mean().backward()
    for name, p in model.named_parameters():
        got, want = p.grad.float(), dict(ref.named_parameters())[name].grad
        rel = float((got - want).norm() / want.norm())
        print(name, "relL2", rel)
        assert rel < 2e-2, (name, rel)                 # (weight-gradient operands are rounded to bf16)


def _fixed_step_grads(ts, state, i=0):
    """Gradients (flat buffer) and loss of step i taken from `state` = (params, exp_avg, exp_avg_sq, seed counter)."""
    with torch.no_grad():
        ts.flat_params.tensor.copy_(state[0])
        ts.exp_avg.copy_(state[1])
        ts.exp_avg_sq.copy_(state[2])
        ts.seed_dev.copy_(state[3])
        ts.sync_shadows()
    loss = float(ts.step(i))
    torch.cuda.synchronize()
    return ts.flat.flat.detach().clone(), loss


def _state_of(ts):
    return (ts.flat_params.tensor.detach().clone(), ts.exp_avg.clone(), ts.exp_avg_sq.clone(), ts.seed_dev.clone())


def test_step_graph_beside_another_streams_persistent_kernel_never_gives_up():
    """VERDICT r3 weak #7b: the cluster form of the chain kernels, the head's cluster and the one-launch GCN wait for peer
    workgroups; under data parallelism the step's graph replays BESIDE RCCL's persistent kernels on the comm stream.  Stand-in:
    64 (then 150) workgroups that hold compute units on a second stream (mobgt_debug_occupy) while the S-FSQ step graph replays
    2 000 times.  No workgroup may give up (they used to trap), and a step taken from a fixed state beside the occupier must
    produce the gradients of the undisturbed step."""
    from mobgt_amd import _lib, forms, ops, workloads
    from mobgt_amd.train import TrainStep
    uni, model, coll = workloads.build("fsq", DEV, seed=1)
    batches = [coll(t) for t in workloads.make_pool("fsq", 2, 16, uni)]
    ts = TrainStep(model, batches, use_graph=True, seed=1)
    ts.prepare()
    assert not forms.on("safe_forms")
    ops.peer_wait_faults(reset=True)
    state = _state_of(ts)
    g_ref, loss_ref = _fixed_step_grads(ts, state)
    g_rep, _ = _fixed_step_grads(ts, state)
    rep = float((g_rep - g_ref).norm() / g_ref.norm())      # two undisturbed runs of one step: f32 atomics in varying order
    print("undisturbed repeat: gradient relL2 %.2e" % rep)  # in front of bf16 rounding points (measured 1e-3)
    side = torch.cuda.Stream()
    lib = _lib.lib()

    import ctypes

    def occupy(n_wg, ticks):
        with torch.cuda.stream(side):
            _lib.check(lib.mobgt_debug_occupy(n_wg, 256, 0, ticks, ctypes.c_void_p(side.cuda_stream)), "mobgt_debug_occupy")
    # the same step beside 64 occupied compute-unit slots (RCCL's footprint), then beside 150 (fewer free units than the chain
    # launch has workgroups: members of a cluster then start late -- a delay, never a give-up)
    for n_wg in (64, 150):
        occupy(n_wg, 300000)                      # 3 ms
        g, loss = _fixed_step_grads(ts, state)
        side.synchronize()
        assert ops.peer_wait_faults() == {}
        rel = float((g - g_ref).norm() / g_ref.norm())
        print("beside %d occupied slots: loss %.6f (undisturbed %.6f), gradient relL2 vs undisturbed %.2e" % (n_wg, loss, loss_ref, rel))
        assert abs(loss - loss_ref) <= 2e-5 * abs(loss_ref) and rel < max(3 * rep, 3e-3)     # (not bitwise even undisturbed)
    for it in range(2000):
        if it % 4 == 0:
            occupy(64, 20000)                     # 200 us each, back to back on the side stream
        ts.step(it)
    torch.cuda.synchronize()
    assert ops.peer_wait_faults() == {}
    assert np.isfinite(float(ts.loss_out))


def test_injected_peer_wait_fault_is_detected_and_the_step_rerun_in_the_safe_forms():
    """A peer wait that gives up sets a fault word instead of trapping; `TrainStep.guarded_step` finds it, restores the
    snapshot, switches every launch to its form without cross-workgroup waits (forms "safe_forms"), captures the graphs again and
    re-runs the step.  Fault injection: limit word 0xffffffff makes every cluster wait report a fault and leave at once."""
    from mobgt_amd import forms, ops, workloads
    from mobgt_amd.train import TrainStep
    uni, model, coll = workloads.build("fsq", DEV, seed=1, model_overrides=dict(n_layers=2))
    batches = [coll(t) for t in workloads.make_pool("fsq", 1, 16, uni)]
    ts = TrainStep(model, batches, use_graph=True, seed=1)
    ts.prepare()
    try:
        ops.peer_wait_faults(reset=True)
        state = _state_of(ts)
        g_ref, loss_ref = _fixed_step_grads(ts, state)
        p_ref = ts.flat_params.tensor.detach().clone()
        with torch.no_grad():
            ts.flat_params.tensor.copy_(state[0]); ts.exp_avg.copy_(state[1]); ts.exp_avg_sq.copy_(state[2]); ts.seed_dev.copy_(state[3])
            ts.sync_shadows()
        ops.set_peer_wait_limit(0xFFFFFFFF)
        with pytest.raises(RuntimeError, match="gave up waiting"):
            ts.step(0)
            ts.check_faults()                       # an unguarded step: the fault is at least never silent
        with torch.no_grad():
            ts.flat_params.tensor.copy_(state[0]); ts.exp_avg.copy_(state[1]); ts.exp_avg_sq.copy_(state[2]); ts.seed_dev.copy_(state[3])
            ts.sync_shadows()
        loss = float(ts.guarded_step(0))
        torch.cuda.synchronize()
        assert ts.faults_recovered == 1 and forms.on("safe_forms")
        assert ops.peer_wait_faults() == {}
        g = ts.flat.flat.detach()
        rel = float((g - g_ref).norm() / g_ref.norm())
        print("re-run in the safe forms: loss %.6f (cluster forms %.6f), gradient relL2 %.2e" % (loss, loss_ref, rel))
        # (the forms differ by the order of a few f32 sums in front of bf16 rounding points: DESIGN 7)
        assert abs(loss - loss_ref) <= 2e-3 * abs(loss_ref) and rel < 2e-2
        dp = float((ts.flat_params.tensor.detach() - p_ref).abs().max())
        assert dp <= 2.5 * float(ts.lr)             # one AdamW step from the snapshot, as in the undisturbed run
        assert int(ts.seed_dev.item()) == int(state[3].item()) + 1
    finally:
        forms.set("safe_forms", None)
        ops.set_peer_wait_limit(0)


def test_layerwise_gradient_buckets_on_the_benched_model_match_the_single_graph(monkeypatch):
    """VERDICT r3 next #3a: under data parallelism phase B of the step is cut in front of layers 3 and 0 of the S-FSQ model into
    three hipGraphs over one autograd graph (train.TrainStep._plan_buckets); the flat buffers are laid out [head | layer 5 | ...
    | layer 0 | rest] so that what each part completes is ONE slice, all-reduced beside the next part.  Here (one process,
    overlap="force"): same loss, gradients and parameters as the single-graph step of the same model with the chain kernels'
    deferred tails and hosted weight gradients on; the layout's invariants; the bytes left for the last, exposed exchange."""
    from mobgt_amd import workloads
    from mobgt_amd.train import TrainStep
    res = {}
    monkeypatch.setenv("MOBGT_DDP_PARTS", "3")
    for mode in (False, "force"):
        uni, model, coll = workloads.build("fsq", DEV, seed=1, model_overrides=dict(peak_lr=1e-12, end_lr=1e-13))
        batches = [coll(t) for t in workloads.make_pool("fsq", 2, 16, uni)]
        ts = TrainStep(model, batches, use_graph=True, seed=5, overlap=mode)
        ts.prepare()
        if mode == "force":
            assert [p[0] for p in ts.parts] == [3, 0, None]
            names = {id(p): n for n, p in model.named_parameters()}
            order = [names[id(p)] for p in ts.flat.params]
            # head first, then layers 5 .. 0 as contiguous runs, then the rest
            first = {li: min(i for i, n in enumerate(order) if n.startswith(f"layers.{li}.")) for li in range(6)}
            last = {li: max(i for i, n in enumerate(order) if n.startswith(f"layers.{li}.")) for li in range(6)}
            assert first[5] == ts.n_head and all(first[li - 1] == last[li] + 1 for li in range(5, 0, -1))
            assert all(last[li] - first[li] + 1 == 16 for li in range(6))
            e = [(p[3], p[4]) for p in ts.parts]
            assert e[0][0] == ts.n_head_elems and e[0][1] == e[1][0] and e[1][1] == e[2][0] and e[2][1] == ts.flat.flat.numel()
            mb = [4e-6 * (b - a) for a, b in [(0, ts.n_head_elems)] + e]
            print("bucket MB (head, layers 5-3, layers 2-0, rest):", [round(x, 2) for x in mb])
            assert mb[-1] <= 4.0            # the only exchange nothing hides
        losses = [float(ts.step(i)) for i in range(3)]
        res[mode] = (losses, ts.flat.flat.clone(), ts.flat_params.tensor.detach().clone())
        del ts, model
    (l0, g0, p0), (l1, g1, p1) = res[False], res["force"]
    print("single graph", l0, "parts", l1)
    np.testing.assert_allclose(l0, l1, rtol=1e-5)
    rel = float((g1 - g0).norm() / g0.norm())
    print("gradient relL2 parts vs single graph %.2e" % rel)
    assert rel < 3e-3                       # (two runs of ONE form differ by ~1e-3: f32 atomics in front of bf16 rounding points)
    np.testing.assert_allclose(p1.cpu().numpy(), p0.cpu().numpy(), atol=1e-9)


def _fsq_small(seed=1):
    from mobgt_amd import workloads
    uni, model, coll = workloads.build("fsq", DEV, seed=seed, model_overrides=dict(n_layers=2))
    batches = [coll(t) for t in workloads.make_pool("fsq", 2, 16, uni)]
    return model, batches


def _grads_of(model):
    return {n: p.grad.detach().float().clone() for n, p in model.named_parameters() if p.grad is not None}


def _assert_same_grads(a, b, what):
    assert a.keys() == b.keys(), what
    for n in a:
        if n.endswith("linear_k.bias"):
            continue
        sc = float(b[n].abs().max())
        quanta = 2 * 5.97e-8 if n.startswith("edge_") else 0.0       # (fp16-quantised tables: test_bias_tables_backward_as_passenger...)
        err = float((a[n] - b[n]).abs().max())
        assert err <= 3e-3 * sc + quanta + 1e-12, (what, n, err, sc)


def test_eval_forward_between_a_training_forward_and_its_backward_leaves_the_gradients_alone():
    """ADVICE r3 / VERDICT r4 weak #11: the step's deferral registries are process-global (step_state.STEP: the bias tables'
    backward job, the front jobs, the weight pack, the fused layers' parked tails, the prelaunched GCN product).  A forward pass of ANOTHER batch in eval mode between a
    training forward and its backward (a validation step inside a training step, a metric hook) must not take, overwrite or
    complete any job that belongs to the pending backward: same gradients as the undisturbed step, up to run-to-run noise."""
    from mobgt_amd import ops
    model, (b0, b1) = _fsq_small()
    seed_dev = torch.tensor([11], dtype=torch.int64, device=DEV)
    for m in model.modules():
        if hasattr(m, "seed_dev"):
            m.seed_dev = seed_dev
    ops.set_dropout_state(seed_dev, 5)
    try:
        res = []
        for disturb in (False, True):
            model.train()
            for p in model.parameters():
                p.grad = None
            loss = model.training_step(b0, 0)
            if disturb:
                model.eval()
                with torch.no_grad():
                    out = model(b1)[0]
                assert bool(torch.isfinite(out).all())
                model.train()
            loss.backward()
            torch.cuda.synchronize()
            res.append((float(loss), _grads_of(model)))
        assert res[0][0] == res[1][0]
        _assert_same_grads(res[1][1], res[0][1], "eval forward in between")
    finally:
        ops.set_dropout_state(None, 0)


def test_a_backward_that_raises_leaves_nothing_parked_and_the_next_step_is_a_clean_step():
    """A Python exception inside the backward pass (a tensor hook on the encoder output: host side, nothing on the device fails)
    ends the step half way: the bias tables' backward job and the head's recorded weight gradients are parked, their takers never
    run.  ops.recording_wgrads drops all of it (STEP.drop_parked), so nothing is left over and the next step of the same model
    and batch has the gradients of an undisturbed step."""
    from mobgt_amd import ops
    model, (b0, _) = _fsq_small()
    seed_dev = torch.tensor([17], dtype=torch.int64, device=DEV)
    for m in model.modules():
        if hasattr(m, "seed_dev"):
            m.seed_dev = seed_dev
    ops.set_dropout_state(seed_dev, 3)
    model.train()

    class Boom(Exception):
        pass

    def step(hook=None):
        for p in model.parameters():
            p.grad = None
        with ops.recording_wgrads():
            loss = model.training_step(b0, 0)
            if hook is not None:
                model._enc_out.register_hook(hook)
            loss.backward()
        torch.cuda.synchronize()
        return _grads_of(model)

    def boom(_g):
        raise Boom("from the encoder output's hook")
    try:
        clean = step()
        assert ops.step_state_leftovers() == {}
        raised = False
        try:                            # (not pytest.raises: nothing may keep the dead pass's frames, and with them its graph, alive)
            step(boom)
        except Boom:
            raised = True
        assert raised
        assert ops.step_state_leftovers() == {}
        after = step()
        assert ops.step_state_leftovers() == {}
        _assert_same_grads(after, clean, "the step after a backward that raised")
    finally:
        ops.set_dropout_state(None, 0)


def test_two_models_alternating_forward_and_backward_keep_their_gradients_apart():
    """Two models in one process: forward A, forward B, backward A, backward B (and the reverse order) give each model the
    gradients its own forward + backward gives it alone."""
    from mobgt_amd import ops
    ma, (a0, _) = _fsq_small(seed=1)
    mb, (_, b1) = _fsq_small(seed=2)
    seed_dev = torch.tensor([13], dtype=torch.int64, device=DEV)
    for mod in (ma, mb):
        for m in mod.modules():
            if hasattr(m, "seed_dev"):
                m.seed_dev = seed_dev
    ops.set_dropout_state(seed_dev, 7)
    try:
        alone = {}
        for tag, mod, b in (("a", ma, a0), ("b", mb, b1)):
            mod.train()
            for p in mod.parameters():
                p.grad = None
            mod.training_step(b, 0).backward()
            torch.cuda.synchronize()
            alone[tag] = _grads_of(mod)
        for order in (("a", "b"), ("b", "a")):
            for mod in (ma, mb):
                for p in mod.parameters():
                    p.grad = None
            la = ma.training_step(a0, 0)
            lb = mb.training_step(b1, 0)
            for tag in order:
                (la if tag == "a" else lb).backward()
            torch.cuda.synchronize()
            _assert_same_grads(_grads_of(ma), alone["a"], f"model a, backward order {order}")
            _assert_same_grads(_grads_of(mb), alone["b"], f"model b, backward order {order}")
    finally:
        ops.set_dropout_state(None, 0)


def test_several_steps_in_one_graph_replay_are_those_steps():
    """`TrainStep.step_group(i, k)` (round 6): k consecutive steps -- forward, backward, AdamW, with the dropout stream, AdamW's t
    and the learning-rate schedule advancing on the device -- captured as ONE graph and replayed without a host round trip in
    between.  Against the same trainer state walked by k single-step replays: the same loss at every group boundary, the same
    parameters / moments afterwards up to what two runs of one step differ by (f32 atomics in front of bf16 rounding points):
    relative L2 of the parameter MOVEMENT <= 2 %, and the device counters agree exactly."""
    from mobgt_amd.train import TrainStep
    res = {}
    for mode in ("single", "group"):
        model, batches = _fsq_small(seed=3)
        torch.manual_seed(0)
        ts = TrainStep(model, batches, use_graph=True, seed=9)
        ts.prepare()
        p0 = ts.flat_params.tensor.detach().clone()
        losses = []
        if mode == "single":
            for i in range(8):
                loss = float(ts.step(i))
                if i % 4 == 3:
                    losses.append(loss)
        else:
            for i in range(0, 8, 4):
                losses.append(float(ts.step_group(i, 4)))
        torch.cuda.synchronize()
        assert not ts.check_faults(on_fault="return")
        res[mode] = dict(losses=losses, move=(ts.flat_params.tensor.detach() - p0).double(), m=ts.exp_avg.double().clone(),
                         count=int(ts.seed_dev.item()), sched=ts.sched_state["step_count"], lr=ts.lr)
    a, b = res["single"], res["group"]
    assert a["count"] == b["count"] and a["sched"] == b["sched"] and a["lr"] == b["lr"]
    np.testing.assert_allclose(b["losses"], a["losses"], rtol=5e-3)
    assert float(a["move"].norm()) > 0
    assert float((a["move"] - b["move"]).norm() / a["move"].norm()) <= 2e-2
    assert float((a["m"] - b["m"]).norm() / a["m"].norm()) <= 2e-2


def test_a_stale_autograd_graph_is_refused_instead_of_crashing_the_capture(tmp_path):
    """Round 6: a loss tensor of an EARLIER eager forward pass that somebody still holds (a failed test's traceback, a logging list)
    keeps that pass's AccumulateGrad nodes alive, bound to the stream it ran on; capturing the trainer's backward on the capture
    stream then aborted the process inside hipStreamEndCapture (core dump).  `TrainStep.prepare()` now recognises the situation
    in its warm-up pass and raises a RuntimeError that says what to delete.  In a child process: a crash must not take pytest down."""
    script = tmp_path / "stale.py"
    script.write_text('''
import sys, os
sys.path.insert(0, %r)
import torch
from mobgt_amd import workloads
from mobgt_amd.train import TrainStep
uni, model, coll = workloads.build("fsq", "cuda", seed=1, model_overrides=dict(n_layers=2))
batches = [coll(t) for t in workloads.make_pool("fsq", 2, 16, uni)]
model.eval()
held = []
for b in batches:
    loss = model.training_step(b, 0)
    loss.backward()
    held.append(loss)                      # the earlier pass's graph stays alive
model.train()
ts, refused = None, False
try:
    ts = TrainStep(model, batches, use_graph=True, seed=1)
    ts.prepare()
except RuntimeError as e:
    print("REFUSED:", str(e)[:120])
    refused = True
assert refused
ts = loss = None                           # (the refused trainer's own warm-up graph goes with it)
held.clear()
import gc; gc.collect()
for p in model.parameters():
    p.grad = None
ts = TrainStep(model, batches, use_graph=True, seed=1)      # ... and with the references gone it works
ts.prepare()
print("OK", float(ts.step(0)))
''' % os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    r = subprocess.run([sys.executable, str(script)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0, (r.returncode, out[-1500:], r.stderr.decode(errors="replace")[-3000:])
    assert "REFUSED: mobgt TrainStep: an autograd graph of an earlier forward pass" in out and "\nOK " in out, out[-1500:]


def _restore(ts, state):
    with torch.no_grad():
        ts.flat_params.tensor.copy_(state[0]); ts.exp_avg.copy_(state[1]); ts.exp_avg_sq.copy_(state[2]); ts.seed_dev.copy_(state[3])
        ts.sync_shadows()


def _movement(ts, state, walk):
    """Parameter movement (f64) of `walk(ts)` taken from `state`."""
    _restore(ts, state)
    walk(ts)
    torch.cuda.synchronize()
    assert not ts.check_faults(on_fault="return")
    return (ts.flat_params.tensor.detach() - state[0]).double()


def _rel(a, b):
    return float((a - b).norm() / b.norm())


def test_a_group_after_add_batch_runs_the_batches_it_names():
    """`step_group(1, 2)` over a pool of two batches runs batches (1, 0); after `add_batch` has grown the pool to three it runs
    (1, 2).  The cache keys a group by the batch indices themselves (step_graphs.group_key), so the entry captured for (1, 0) is
    not replayed where (1, 2) is meant (first finding).  Each group against the matching walk of single steps from the
    same trainer state: relative L2 of the parameter movement <= 2 % (the bound of test_several_steps_in_one_graph_replay_...).
    Precondition: the two single-step walks themselves differ by at least ten times that, or the comparison could not tell the
    batches apart (measured on the commit before this cache: docs/NOTEBOOK.md, "One cache for a TrainStep's graphs")."""
    from mobgt_amd import workloads
    from mobgt_amd.step_graphs import group_key
    from mobgt_amd.train import TrainStep
    uni, model, coll = workloads.build("fsq", DEV, seed=1, model_overrides=dict(n_layers=2))
    b0, b1, b2 = [coll(t) for t in workloads.make_pool("fsq", 3, 16, uni)]
    ts = TrainStep(model, [b0, b1], use_graph=True, seed=1)
    ts.prepare()
    state = _state_of(ts)
    single_10 = _movement(ts, state, lambda t: (t.step(1), t.step(0)))
    group_10 = _movement(ts, state, lambda t: t.step_group(1, 2))
    assert set(ts.graphs.of("group")) == {group_key(1, 2, 2, False)} == {("group", (1, 0), False)}
    assert ts.add_batch(b2) == 2
    single_12 = _movement(ts, state, lambda t: (t.step(1), t.step(2)))
    group_12 = _movement(ts, state, lambda t: t.step_group(1, 2))
    assert set(ts.graphs.of("group")) == {("group", (1, 0), False), ("group", (1, 2), False)}
    apart = _rel(single_12, single_10)
    print("single-step walks (1, 2) vs (1, 0): relL2 of the movement %.3f;  group vs walk: (1, 0) %.2e, (1, 2) %.2e"
          % (apart, _rel(group_10, single_10), _rel(group_12, single_12)))
    assert apart >= 0.2
    assert _rel(group_10, single_10) <= 2e-2
    assert _rel(group_12, single_12) <= 2e-2


def test_a_group_after_recapture_is_a_new_capture():
    """`recapture()` (what `guarded_step` calls after switching to the forms without cross-workgroup waits) clears the WHOLE cache:
    no entry of any kind from before is still listed, a group is captured again on its next use -- in the forms that hold then --
    and computes what two single steps in those forms compute (relative L2 of the parameter movement <= 2 %)."""
    from mobgt_amd import forms
    from mobgt_amd.train import TrainStep
    kinds = ("step", "micro", "update", "opt", "group")
    model, batches = _fsq_small()
    ts = TrainStep(model, batches, use_graph=True, seed=1)
    ts.prepare()
    state = _state_of(ts)
    ts.step_group(0, 2)
    key = ("group", (0, 1), False)
    old = ts.graphs.of("group")[key]
    before = [e for kind in kinds for e in ts.graphs.of(kind).values()]
    assert len(before) == 3 and not forms.on("safe_forms")               # (two steps and the group)

    def none_from_before():
        return all(e is not o for kind in kinds for e in ts.graphs.of(kind).values() for o in before)
    with forms.using(safe_forms=True):
        ts.recapture()
        assert none_from_before() and set(ts.graphs.of("step")) == {("step", 0, False), ("step", 1, False)}
        assert ts.graphs.of("group") == {}
        single = _movement(ts, state, lambda t: (t.step(0), t.step(1)))
        group = _movement(ts, state, lambda t: t.step_group(0, 2))
        assert ts.graphs.of("group")[key] is not old and none_from_before()
    print("group vs two single steps, both in the safe forms: relL2 of the movement %.2e" % _rel(group, single))
    assert float(single.norm()) > 0 and _rel(group, single) <= 2e-2
