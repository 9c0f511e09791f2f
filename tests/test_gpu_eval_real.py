"""train.EvalLoop on the reference's own numbers for a trained model (golden G10, tests/golden/make_golden_traj.py): the f32
TrainStep walks the reference's 30-update training trajectory on real Gowalla data (as tests/test_gpu_real.py does), then EvalLoop
evaluates the 256 real test trajectories in batches of 16.  Its ACC / NDCG @1/5/10/20 and MRR meet the golden metrics at that
test's gates (atol 1/256; MRR rtol 2e-2) and equal metrics.evaluate_outputs over test_step outputs of the same batches exactly."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_real import DeviceCollator, g8, real_trajs, seeded_state   # noqa: E402,F401  (g8: the module's fixture)
from test_gpu_eval import _eager_eval, _same                              # noqa: E402

DEV = "cuda"


def test_eval_loop_after_the_references_training_trajectory_g10(g8, golden_dir):
    from mobgt_amd.model_fqandtoyo import Graphormer
    from mobgt_amd.train import EvalLoop, TrainStep
    z8, uni, table = g8
    z = np.load(os.path.join(golden_dir, "g10_traj.npz"))
    steps, batch, n_test = (int(v) for v in z["args/steps_batch_ntest"])
    warm, tot, peak, end, wd = (float(v) for v in z["args/lr"])
    m = Graphormer(n_layers=6, num_heads=8, hidden_dim=128, dropout_rate=0.0, intput_dropout_rate=0.0, weight_decay=wd,
                   ffn_dim=1024, dataset_name="gowalla_nevda", warmup_updates=int(warm), tot_updates=int(tot), peak_lr=peak,
                   end_lr=end, edge_type="multi_hop", multi_hop_max_dist=20, attention_dropout_rate=0.0, universe=uni)
    names = [str(n) for n in z["param_names"]]
    shapes = [eval(str(s)) for s in z["param_shapes"]]
    m.load_state_dict({k: v.detach() for k, v in seeded_state(list(zip(names, shapes)), int(z["seed"])).items()}, strict=True)
    m = m.to(DEV).train()
    m.poi_distance_model.dropout = 0.0
    m.poi_cat_model.dropout = 0.0
    m.pos_embed.dropout.p = 0.0
    coll = DeviceCollator(DEV, bin_table=table, multi_hop_max_dist=20, rel_pos_max=1024)
    trajs = real_trajs(z, "train")
    ts = TrainStep(m, [coll(trajs[s * batch:(s + 1) * batch], idx0=s * batch) for s in range(steps)], use_graph=True, seed=1)
    ts.prepare()
    for s in range(steps):
        loss = float(ts.step(s))
        assert abs(loss - float(z["losses"][s])) <= 1e-4 * float(z["losses"][s]), (s, loss)
    tt = real_trajs(z, "test")[:n_test]
    ev = EvalLoop(m, coll, tt, batch_size=batch)
    r = ev.run()
    assert r["n"] == n_test == 256
    got = np.array([r["acc@1"], r["acc@5"], r["acc@10"], r["ndcg@1"], r["ndcg@5"], r["ndcg@10"], r["acc@20"], r["ndcg@20"]])
    print("EvalLoop metrics", got, "mrr", r["mrr"], "reference", z["metrics/acc1_5_10_ndcg1_5_10_acc20_ndcg20"], float(z["metrics/mrr"]))
    np.testing.assert_allclose(got, z["metrics/acc1_5_10_ndcg1_5_10_acc20_ndcg20"], atol=1.0 / n_test + 1e-12)
    np.testing.assert_allclose(r["mrr"], float(z["metrics/mrr"]), rtol=2e-2)
    _same(r, _eager_eval(m, coll, tt, ev.batches()))
