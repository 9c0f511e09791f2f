"""Worker of tests/test_gpu_accum.py: one data-parallel rank of `train.TrainStep(accumulate=k, clip_norm=c)`, the model, data
and process-group set-up of tests/_ddp_worker.py.

    argv: output directory, number of micro-steps (a final `flush()` ends a short window).
    MOBGT_TEST_ACCUM / MOBGT_TEST_CLIP / MOBGT_TEST_GRAD_COMM / MOBGT_TEST_DATA_RANK from the environment.
Writes rank<r>.pt: every micro-step's own gradient (the flat buffer before it is added to the window), the parameters before
and after, both Adam moments, grad_norm and the counters."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402


def main():
    out_dir, steps = sys.argv[1], int(sys.argv[2])
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    multi = torch.cuda.device_count() >= world
    dev = torch.device("cuda", rank if multi else 0)
    torch.cuda.set_device(dev)
    from mobgt_amd.train import recommended_env
    for k_, v_ in recommended_env().items():
        os.environ.setdefault(k_, v_)
    if multi:
        dist.init_process_group("nccl", device_id=dev)
    else:
        dist.init_process_group("gloo")
    from mobgt_amd import synth
    from mobgt_amd.data import DeviceCollator, make_bin_table
    from mobgt_amd.model_fqandtoyo import Graphormer
    from mobgt_amd.train import TrainStep, broadcast_parameters
    args = dict(n_layers=2, num_heads=8, hidden_dim=64, dropout_rate=0.1, intput_dropout_rate=0.1, weight_decay=0.01,
                ffn_dim=128, warmup_updates=4, tot_updates=100, peak_lr=1e-3, end_lr=1e-9, edge_type="multi_hop",
                multi_hop_max_dist=20, attention_dropout_rate=0.1, dataset_name="foursquaregraph")
    uni = synth.make_universe(P=400, n_cat=12, n_user=1080, seed=3)
    nb, _, table = make_bin_table(uni.distance)
    torch.manual_seed(100 + rank)                         # different init per rank, equalised by the broadcast
    model = Graphormer(universe=uni, num_bins=nb + 2, bias_dtype=torch.bfloat16, gcn_dtype=torch.bfloat16,
                       act_dtype=torch.bfloat16, **args).to(dev)
    broadcast_parameters(model)
    coll = DeviceCollator(dev, bin_table=table)
    drank = int(os.environ.get("MOBGT_TEST_DATA_RANK", rank))
    batches = [coll(synth.make_batch_of_trajectories(seed=10 + 7 * drank + i, G=4, P=400, n_user=1080, cat_of_poi=uni.cat_of_poi))
               for i in range(2)]                         # different data per rank
    comm = os.environ.get("MOBGT_TEST_GRAD_COMM")
    clip = os.environ.get("MOBGT_TEST_CLIP")
    ts = TrainStep(model, batches, use_graph=True, seed=5, grad_comm_dtype=torch.bfloat16 if comm == "bf16" else None,
                   accumulate=int(os.environ.get("MOBGT_TEST_ACCUM", "1")), clip_norm=float(clip) if clip else None)
    # every collective counted where it is issued, independently of the trainer's own bookkeeping: per capture of a micro-step
    # graph, per capture of an update graph (a captured all_reduce is a node of that graph), and per host call of step / flush
    calls = {"n": 0}
    real_all_reduce = dist.all_reduce

    def counting_all_reduce(*a, **k):
        calls["n"] += 1
        return real_all_reduce(*a, **k)
    dist.all_reduce = counting_all_reduce
    in_micro_captures, in_update_captures = [], []
    for name, log in (("_capture_micro", in_micro_captures), ("_capture_update", in_update_captures)):
        def wrapped(*a, _f=getattr(ts, name), _log=log, **k):
            n0 = calls["n"]
            out = _f(*a, **k)
            _log.append(calls["n"] - n0)
            return out
        setattr(ts, name, wrapped)
    ts.prepare()
    params0 = ts.flat_params.tensor.detach().cpu().clone()
    losses, micro = [], []
    per_step = []
    for i in range(steps):
        n0 = calls["n"]
        losses.append(float(ts.step(i)))
        per_step.append(calls["n"] - n0)
        micro.append(ts.flat.flat.detach().cpu().clone())
    n0 = calls["n"]
    ts.flush()
    in_flush = calls["n"] - n0
    dist.all_reduce = real_all_reduce
    torch.cuda.synchronize()
    ts.check_faults(on_fault="raise")
    torch.save(dict(losses=losses, micro=micro, params0=params0, params=ts.flat_params.tensor.detach().cpu(),
                    exp_avg=ts.exp_avg.cpu(), exp_avg_sq=ts.exp_avg_sq.cpu(), backend=dist.get_backend(), forced=ts.force_comm,
                    one_graph=ts.one_graph, overlap=ts.overlap, exchanges=ts.exchanges_done, updates=ts.updates_done,
                    window_pos=ts.window_pos, all_reduce_per_step=per_step, all_reduce_in_flush=in_flush,
                    all_reduce_in_micro_captures=in_micro_captures, all_reduce_in_update_captures=in_update_captures,
                    grad_norm=None if ts.grad_norm is None else ts.grad_norm.cpu(),
                    upd_dev=int(ts.upd_dev.item()), acc_max=0.0 if ts.acc is None else float(ts.acc.abs().max()),
                    comm_dtype=str(ts.comm_buf.dtype) if ts.comm_buf is not None else None,
                    shadow=None if ts.shadow_flat is None else ts.shadow_flat.float().cpu()),
               os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
