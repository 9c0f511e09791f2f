"""`bench.py --dump-outputs DIR` on the host: one float32 .npy per output of the step (its loss and every trained parameter),
named by parameter; under a byte budget the largest are sampled -- the same elements in every run -- and the files stay within
the budget."""
import os
import types

import numpy as np
import torch

import bench


def _fake_step():
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(300, 200), torch.nn.Linear(200, 5))
    params = list(model.parameters())
    with torch.no_grad():
        for p in params:                          # distinct values within a parameter: a sampled value names its index
            p.copy_(torch.randperm(p.numel()).float().view_as(p))
    flat = types.SimpleNamespace(params=params, views=[torch.randn_like(p) for p in params])
    return model, types.SimpleNamespace(loss_out=torch.tensor(1.25), flat=flat)


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_whole_outputs_within_budget(tmp_path):
    model, ts = _fake_step()
    bench.dump_outputs(ts, model, str(tmp_path))
    got = _load(tmp_path)
    assert set(got) == {"loss"} | {"param." + n for n, _ in model.named_parameters()}
    assert all(a.dtype == np.float32 for a in got.values())
    assert got["loss"].tolist() == [1.25]
    for n, p in model.named_parameters():
        np.testing.assert_array_equal(got["param." + n], p.detach().numpy())


def test_sampled_outputs_are_fixed(tmp_path):
    model, ts = _fake_step()
    budget = 100_000
    bench.dump_outputs(ts, model, str(tmp_path / "a"), budget=budget)
    bench.dump_outputs(ts, model, str(tmp_path / "b"), budget=budget)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sum(x.nbytes for x in a.values()) <= budget
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    w = model[0].weight.detach().numpy().reshape(-1)
    assert 0 < a["param.0.weight"].size < w.size
    # the sample is elements of the parameter, in their flat order
    idx = np.nonzero(np.isin(w, a["param.0.weight"]))[0]
    np.testing.assert_array_equal(w[idx], a["param.0.weight"])
    np.testing.assert_array_equal(a["param.1.weight"], model[1].weight.detach().numpy())
