"""Worker of tests/test_gpu_eval.py::test_two_rank_gloo_evaluation_returns_the_pooled_result: one rank of `train.EvalLoop`.

RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT from the environment.  Both ranks share cuda:0 over gloo (MOBGT_TEST_SHARED_GPU=1 or a
one-GPU box); otherwise RCCL with one GPU per rank.  Writes rank<r>.json: the pooled dict run() returns, and the dict of ONE rank
(world = 1) evaluating both ranks' shards back to back."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402


def main():
    out_dir = sys.argv[1]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    shared = os.environ.get("MOBGT_TEST_SHARED_GPU") == "1" or torch.cuda.device_count() < world
    dev = torch.device("cuda", 0 if shared else rank)
    torch.cuda.set_device(dev)
    if shared:
        dist.init_process_group("gloo")
    else:
        dist.init_process_group("nccl", device_id=dev)
    from mobgt_amd import workloads
    from mobgt_amd.train import EvalLoop
    from test_gpu_eval import _eval_dataset
    uni, model, coll = workloads.build("fsq", dev, seed=1, P=1500, model_overrides=dict(n_layers=2))   # same weights on both ranks
    data = _eval_dataset(uni, n=63, seed=64)                     # 32 samples per rank: two batches each
    pooled = EvalLoop(model, coll, data, batch_size=16).run()   # rank / world from the process group
    cat = [data[i] for r in range(world) for b in EvalLoop(model, coll, data, batch_size=16, rank=r, world=world).batches() for i in b]
    one = EvalLoop(model, coll, cat, batch_size=16, rank=0, world=1).run()
    with open(os.path.join(out_dir, f"rank{rank}.json"), "w") as f:
        json.dump(dict(pooled=pooled, one_rank=one), f)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
