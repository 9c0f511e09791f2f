"""Gradient accumulation and global-norm clipping of the train step on a real MI355X (`TrainStep(accumulate=k, clip_norm=c)`,
DESIGN 13): the three kernels through the C ABI against torch, the update trajectory against torch.optim.AdamW +
clip_grad_norm_ + PolynomialDecayLR, the dropout stream per micro-step, the untouched default path, data parallelism (one
exchange per window), the epoch loop's flush, guarded_step's snapshot, and the error paths.

Bounds.  Norm: every f32 partial is a sum of B = mobgt_grad_norm_block() non-negative products, so its relative error is at
most B * 2^-24 (the f64 finish and the square root only shrink it): the tests compute that bound from the exported constant.
Trajectory: the per-update tolerances of test_gpu_train.py's AdamW trajectory test.  Data parallel: that file's gates (1e-5 /
5e-3 relative L2 of the exchanged gradient for the fp32 / bf16 exchange, 5 % of the parameter movement)."""
import math
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


def _setup(seed=0, f32=False, **over):
    """The small fq model and the two batches of tests/test_gpu_train.py::_setup (`f32`: the f32 configuration instead)."""
    from mobgt_amd.model_fqandtoyo import Graphormer
    uni = synth.make_universe(P=400, n_cat=12, n_user=1080, seed=3)
    nb, _, table = make_bin_table(uni.distance)
    torch.manual_seed(seed)
    dtypes = {} if f32 else dict(bias_dtype=torch.bfloat16, gcn_dtype=torch.bfloat16, act_dtype=torch.bfloat16)
    model = Graphormer(universe=uni, num_bins=nb + 2, **dtypes, **dict(ARGS, **over)).to(DEV)
    coll = DeviceCollator(DEV, bin_table=table)
    batches = [coll(synth.make_batch_of_trajectories(seed=10 + i, G=4, P=400, n_user=1080, cat_of_poi=uni.cat_of_poi))
               for i in range(2)]
    return model, batches


# ---- the kernels through the C ABI ---------------------------------------------------------------------------------------
def _abi():
    from mobgt_amd import _lib
    from mobgt_amd.ops import _p, _stream
    return _lib, _lib.lib(), _p, _stream


def _accumulate(acc, g, part):
    _lib, lib, _p, _stream = _abi()
    _lib.check(lib.mobgt_grad_accumulate(_p(acc), _p(g), acc.numel(), _p(part), _stream()), "mobgt_grad_accumulate")


def _finish(part, inv_k, clip, gn, sc, cnt):
    _lib, lib, _p, _stream = _abi()
    _lib.check(lib.mobgt_grad_norm_finish(_p(part), 0 if part is None else part.numel(), inv_k, clip, _p(gn), _p(sc), _p(cnt),
                                          _stream()), "mobgt_grad_norm_finish")


def _norm_bound():
    return int(_abi()[1].mobgt_grad_norm_block()) * 2.0 ** -24


@pytest.mark.parametrize("n", [1, 5, 1023, 1024, 4099, 6_500_000, 42_000_000])
def test_accumulate_and_norm_kernels_against_torch(n):
    """acc += g is torch's f32 add bit for bit (with and without the partial sums); the norm is within B * 2^-24 of the f64
    value; the same input gives the same bits; the norm-only form sees what the fused form saw; the scaled AdamW leaves the
    accumulator all zeros."""
    _lib, lib, _p, _stream = _abi()
    blk = int(lib.mobgt_grad_norm_block())
    npart = (n + blk - 1) // blk
    gen = torch.Generator(device=DEV).manual_seed(1 + n % 997)
    acc0 = torch.randn(n, device=DEV, generator=gen)
    g = torch.randn(n, device=DEV, generator=gen) * 3.0
    want = acc0 + g
    ref = float(want.double().norm())
    runs = []
    for _ in range(2):
        acc = acc0.clone()
        part = torch.full((npart,), float("nan"), device=DEV)
        _accumulate(acc, g, part)
        gn, sc = torch.zeros((), device=DEV), torch.zeros((), device=DEV)
        cnt = torch.tensor([7], dtype=torch.int64, device=DEV)
        _finish(part, 1.0, 1e30, gn, sc, cnt)
        assert torch.equal(acc, want)
        assert int(cnt.item()) == 8 and float(sc) == 1.0
        runs.append((part, gn.clone()))
    rel = abs(float(runs[0][1]) - ref) / ref
    print("n = %d: norm %.9g (f64 %.9g), relative error %.2e, bound %.2e" % (n, float(runs[0][1]), ref, rel, _norm_bound()))
    assert rel <= _norm_bound()
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    acc = acc0.clone()
    _accumulate(acc, g, None)                                   # add only
    assert torch.equal(acc, want)
    part = torch.full((npart,), float("nan"), device=DEV)
    _accumulate(acc, None, part)                                # norm only, of what is there
    assert torch.equal(acc, want) and torch.equal(part, runs[0][0])
    # the scaled AdamW consumes the accumulator and leaves zeros; with lr > 0 every parameter with a gradient moves
    p = torch.zeros(n, device=DEV)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    lr_dev, sc = torch.full((), 1e-3, device=DEV), torch.full((), 0.5, device=DEV)
    cnt = torch.tensor([1], dtype=torch.int64, device=DEV)
    _lib.check(lib.mobgt_adamw_flat_scaled(_p(p), _p(acc), _p(m), _p(v), None, n, _p(lr_dev), None, _p(cnt), 0, _p(sc), 1,
                                           0.9, 0.999, 1e-8, 0.01, _stream()), "mobgt_adamw_flat_scaled")
    assert float(acc.abs().max()) == 0.0
    one_minus_beta1 = float(np.float32(1.0) - np.float32(0.9))   # (the kernel's f32 constant)
    assert torch.equal(m, one_minus_beta1 * (0.5 * want))        # (halving is exact, the other product one f32 rounding)
    assert bool(((p != 0) == (want != 0)).all())


@pytest.mark.parametrize("inv_k", [1.0, 0.25])
def test_scale_and_grad_norm_match_clip_grad_norm(inv_k):
    """grad_norm and scale = inv_k * coef against torch.nn.utils.clip_grad_norm_ on g = inv_k * acc, for norms below, at and far
    above c, a NaN and an inf entry (error_if_nonfinite=False: the non-finite norm propagates)."""
    n = 4099
    acc = torch.randn(n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(4)) * 2.0
    blk = int(_abi()[1].mobgt_grad_norm_block())
    norm = float((acc.double() * inv_k).norm())
    tol = _norm_bound()       # (the scale inherits the norm's relative error; torch's own f32 result is ~1e-7 from the f64 value)
    for what, c, poison in (("below", norm * 2.0, None), ("at", norm, None), ("far above", norm / 1000.0, None),
                            ("nan", 1.0, float("nan")), ("inf", 1.0, float("inf"))):
        a = acc.clone()
        if poison is not None:
            a[5] = poison
        p = torch.nn.Parameter(torch.zeros(n, device=DEV))
        p.grad = a * inv_k
        total = torch.nn.utils.clip_grad_norm_([p], c, norm_type=2.0, error_if_nonfinite=False)
        coef = torch.clamp(c / (total + 1e-6), max=1.0)
        part = torch.zeros((n + blk - 1) // blk, device=DEV)
        gn, sc = torch.zeros((), device=DEV), torch.zeros((), device=DEV)
        cnt = torch.zeros(1, dtype=torch.int64, device=DEV)
        _accumulate(a, None, part)
        _finish(part, inv_k, c, gn, sc, cnt)
        print(what, "torch", float(total), float(coef), "device", float(gn), float(sc) / inv_k)
        assert int(cnt.item()) == 1
        if what == "nan":
            assert math.isnan(float(total)) and math.isnan(float(gn)) and math.isnan(float(coef)) and math.isnan(float(sc))
        elif what == "inf":
            assert math.isinf(float(total)) and math.isinf(float(gn)) and float(coef) == 0.0 and float(sc) == 0.0
        else:
            assert abs(float(gn) - float(total)) <= tol * float(total)
            assert abs(float(sc) - inv_k * float(coef)) <= tol * inv_k * float(coef)
            assert float(sc) == inv_k if what == "below" else float(sc) <= inv_k
            assert float(sc) < 0.01 * inv_k if what == "far above" else True
    # without clipping: scale = inv_k, grad_norm untouched
    gn, sc = torch.full((), -1.0, device=DEV), torch.zeros((), device=DEV)
    _finish(None, inv_k, 0.0, gn, sc, cnt)
    assert float(sc) == np.float32(inv_k) and float(gn) == -1.0 and int(cnt.item()) == 2


@pytest.mark.parametrize("with_sched", [False, True])
def test_scaled_adamw_with_scale_one_is_the_plain_kernel_bit_for_bit(with_sched):
    """Five steps of mobgt_adamw_flat_scaled (scale 1.0 written by the finish kernel, t from the update counter) against
    mobgt_adamw_flat (t from the step counter): parameters, moments and the bf16 shadow are identical bits."""
    _lib, lib, _p, _stream = _abi()
    gen = torch.Generator().manual_seed(3)
    n = 10007
    p0 = torch.randn(n, generator=gen)
    pa, pb = p0.clone().to(DEV), p0.clone().to(DEV)
    ma, va, mb, vb = (torch.zeros(n, device=DEV) for _ in range(4))
    sha, shb = (torch.zeros(n, dtype=torch.bfloat16, device=DEV) for _ in range(2))
    lr_dev = torch.zeros((), device=DEV)
    sched = torch.tensor([3.0, 50.0, 1e-3, 1e-9, 0.0], device=DEV) if with_sched else None
    step_dev = torch.tensor([40], dtype=torch.int64, device=DEV)
    upd_dev = torch.zeros(1, dtype=torch.int64, device=DEV)
    sc = torch.zeros((), device=DEV)
    for it in range(5):
        g = (torch.randn(n, generator=gen) * (0.1 + it)).to(DEV)
        lr_dev.fill_(1e-3 * (it + 1))
        step_dev.add_(1)
        _lib.check(lib.mobgt_adamw_flat(_p(pa), _p(g), _p(ma), _p(va), _p(sha), n, _p(lr_dev), _p(sched), _p(step_dev), 40,
                                        0.9, 0.999, 1e-8, 0.01, _stream()), "mobgt_adamw_flat")
        acc = g.clone()
        _finish(None, 1.0, 0.0, None, sc, upd_dev)
        _lib.check(lib.mobgt_adamw_flat_scaled(_p(pb), _p(acc), _p(mb), _p(vb), _p(shb), n, _p(lr_dev), _p(sched), _p(upd_dev), 0,
                                               _p(sc), 1, 0.9, 0.999, 1e-8, 0.01, _stream()), "mobgt_adamw_flat_scaled")
        assert float(sc) == 1.0 and int(upd_dev.item()) == it + 1 and float(acc.abs().max()) == 0.0
        assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb) and torch.equal(sha, shb), it
    assert not torch.equal(pa, p0.to(DEV))


def test_scaled_adamw_matches_torch_adamw_fed_the_scaled_gradient():
    """scale = (1 / k) * coef from the finish kernel; torch.optim.AdamW is fed scale * g in f64 (tolerances of
    tests/test_gpu_layer.py::test_adamw_flat_matches_torch_adamw); zero_grads = 0 leaves the gradient alone."""
    _lib, lib, _p, _stream = _abi()
    gen = torch.Generator().manual_seed(3)
    n = 10007
    blk = int(lib.mobgt_grad_norm_block())
    p0 = torch.randn(n, generator=gen)
    ref = torch.nn.Parameter(p0.clone().double())
    opt = torch.optim.AdamW([ref], lr=1e-3, weight_decay=0.01)
    p = p0.clone().to(DEV)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    sh = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
    lr_dev = torch.zeros((), device=DEV)
    upd_dev = torch.zeros(1, dtype=torch.int64, device=DEV)
    gn, sc = torch.zeros((), device=DEV), torch.zeros((), device=DEV)
    part = torch.zeros((n + blk - 1) // blk, device=DEV)
    scales = []
    for it in range(5):
        g = (torch.randn(n, generator=gen) * (0.1 + it)).to(DEV)
        keep = g.clone()
        lr = 1e-3 * (it + 1)
        _accumulate(g, None, part)
        _finish(part, 0.5, 60.0, gn, sc, upd_dev)               # ||g / 2|| runs from ~5 to ~205: some steps clip, some do not
        scales.append(float(sc))
        for grp in opt.param_groups:
            grp["lr"] = lr
        ref.grad = g.double().cpu() * float(sc)
        opt.step()
        lr_dev.fill_(lr)
        _lib.check(lib.mobgt_adamw_flat_scaled(_p(p), _p(g), _p(m), _p(v), _p(sh), n, _p(lr_dev), None, _p(upd_dev), 0, _p(sc), 0,
                                               0.9, 0.999, 1e-8, 0.01, _stream()), "mobgt_adamw_flat_scaled")
        assert torch.equal(g, keep)
        np.testing.assert_allclose(p.cpu().numpy(), ref.detach().float().numpy(), rtol=2e-5, atol=2e-6)
    assert torch.equal(sh, p.bfloat16())
    assert scales[0] == 0.5 and scales[-1] < 0.5, scales


# ---- the trainer ----------------------------------------------------------------------------------------------------------
def _slack_mask(ts):
    """True for the elements of the flat buffers that belong to no parameter (alignment padding, slack behind a slot)."""
    mask = torch.ones(ts.flat.flat.numel(), dtype=torch.bool, device=DEV)
    for p, off in zip(ts.flat.params, ts.flat.offsets):
        mask[off:off + p.numel()] = False
    return mask


_CLIP = {}


def _clip_between_the_window_norms():
    """A clip_norm that some of the trajectory's updates exceed and some do not: the median of the unclipped run's norms."""
    if "c" not in _CLIP:
        from mobgt_amd.train import TrainStep
        model, batches = _setup()
        ts = TrainStep(model, batches, use_graph=False, seed=5, accumulate=3, clip_norm=1e9)
        norms = []
        for i in range(12):
            ts.step(i)
            if ts.window_pos == 0:
                norms.append(float(ts.grad_norm))
        s = sorted(norms)
        _CLIP["c"] = 0.5 * (s[1] + s[2])
        print("window norms without clipping", norms, "-> clip_norm", _CLIP["c"])
    return _CLIP["c"]


@pytest.mark.parametrize("use_graph", [True, False])
def test_accumulated_clipped_trajectory_matches_torch(use_graph):
    """accumulate=3 with clipping, windows of 3, 3, 3, a flushed one of 2, then 3: after every update the parameters are
    torch.optim.AdamW + PolynomialDecayLR stepped on clip_grad_norm_(mean of the window's micro-gradients / 3 in f64), at the
    per-update tolerances of test_train_step_trajectory_matches_torch_adamw_and_polynomial_decay; grad_norm is torch's returned
    norm; the parameters stand still between updates; the bf16 shadow follows; slack elements never carry anything."""
    from mobgt_amd.lr import PolynomialDecayLR
    from mobgt_amd.train import TrainStep
    c = _clip_between_the_window_norms()
    model, batches = _setup()
    ts = TrainStep(model, batches, use_graph=use_graph, seed=5, accumulate=3, clip_norm=c)
    ts.prepare()
    assert float(ts.exp_avg.abs().max()) == 0.0 and float(ts.acc.abs().max()) == 0.0 and ts.updates_done == 0
    slack = _slack_mask(ts)
    ref = torch.nn.Parameter(ts.flat_params.tensor.detach().double().clone())
    opt = torch.optim.AdamW([ref], lr=ARGS["peak_lr"], weight_decay=ARGS["weight_decay"])
    sched = PolynomialDecayLR(opt, ARGS["warmup_updates"], ARGS["tot_updates"], ARGS["peak_lr"], ARGS["end_lr"], 1.0)
    plan = [3, 3, 3, 2, 3]                                  # (the window of 2 is ended by flush)
    i, clipped = 0, []
    for u, size in enumerate(plan):
        before = ts.flat_params.tensor.detach().clone()
        total = torch.zeros_like(ref)
        for j in range(size):
            assert ts.window_pos == j and ts.updates_done == u
            assert torch.equal(ts.flat_params.tensor.detach(), before)          # no movement inside a window
            ts.step(i)
            i += 1
            micro = ts.flat.flat.detach().clone()
            assert float(micro[slack].abs().max()) == 0.0 if bool(slack.any()) else True
            total += micro.double()
        if size < 3:
            assert ts.window_pos == size and torch.equal(ts.flat_params.tensor.detach(), before)
            ts.flush()
        assert ts.window_pos == 0 and ts.updates_done == u + 1 and ts.sched_state["step_count"] == u + 2
        assert int(ts.upd_dev.item()) == u + 1 and int(ts.seed_dev.item()) == 5 + i
        ref.grad = total / 3.0                              # the divisor is k also for the short window
        norm = torch.nn.utils.clip_grad_norm_([ref], c, norm_type=2.0)
        clipped.append(float(norm) > c)
        opt.step()
        sched.step()
        rel = abs(float(ts.grad_norm) - float(norm)) / float(norm)
        print("update %d (%d micro-steps): norm %.6g (torch %.6g, rel %.1e) clipped %s" % (u + 1, size, float(ts.grad_norm), float(norm),
                                                                                          rel, clipped[-1]))
        assert rel <= _norm_bound()
        assert float(ts.acc.abs().max()) == 0.0             # the accumulator contract: zero again behind the update
        got, want = ts.flat_params.tensor.detach().double().cpu().numpy(), ref.detach().cpu().numpy()
        np.testing.assert_allclose(got, want, rtol=1.5e-7 * (u + 1), atol=2e-7 * (u + 1) + 1e-6 * ARGS["peak_lr"])
        assert not torch.equal(ts.flat_params.tensor.detach(), before)
        if ts.shadow_flat is not None:
            assert torch.equal(ts.shadow_flat, ts.flat_params.tensor.detach().bfloat16())
    assert any(clipped) and not all(clipped), clipped
    ts.flush()                                              # an empty window: nothing happens
    assert ts.updates_done == len(plan) and int(ts.upd_dev.item()) == len(plan)
    with pytest.raises(NotImplementedError):
        ts.step_group(0, 2)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def test_every_micro_step_draws_fresh_masks_those_of_the_plain_steps():
    """Three micro-steps of ONE window on the same batch give three different gradients, and micro-step j's gradient is plain
    step j's (same seed, a learning rate too small to move a weight): compared at the run-to-run gate of the two-run tests in
    test_gpu_train.py (f32 atomics in front of bf16 rounding points: not bitwise in this configuration)."""
    from mobgt_amd.train import TrainStep
    tiny = dict(peak_lr=1e-12, end_lr=1e-13)
    res = {}
    for tag, kw in (("plain", {}), ("plain2", {}), ("accum", dict(accumulate=3))):
        model, batches = _setup(**tiny)
        ts = TrainStep(model, batches[:1], use_graph=True, seed=5, **kw)
        ts.prepare()
        res[tag] = []
        for j in range(3):
            ts.step(0)
            res[tag].append(ts.flat.flat.detach().clone())
        assert ts.updates_done == (1 if kw else 3) and int(ts.seed_dev.item()) == 8
    rep = max(_rel(a, b) for a, b in zip(res["plain2"], res["plain"]))
    gate = max(3 * rep, 3e-3)
    for j in range(3):
        same = _rel(res["accum"][j], res["plain"][j])
        print("micro-step %d vs plain step %d: relL2 %.2e (two plain runs %.2e)" % (j, j, same, rep))
        assert same < gate
        for k in range(j):
            assert _rel(res["accum"][j], res["accum"][k]) > 10 * gate           # other masks, the same batch


@pytest.mark.parametrize("cfg", ["f32", "bf16"])
def test_default_arguments_are_the_plain_step_and_launch_nothing_new(monkeypatch, cfg):
    """`TrainStep(accumulate=1, clip_norm=None)` and a TrainStep constructed as before, same seed, five steps, in the f32
    configuration and in the bf16 one: no accumulator, no new buffer, the OLD optimizer entry point and none of the new ones
    (captures and replays included), the same counters.  The backward pass is not bit-reproducible in either configuration
    (float atomics: DESIGN 8; whether the two trainers came out bitwise equal is printed), so the bits are pinned where they do
    not depend on it -- at the AdamW inputs: replaying `mobgt_adamw_flat` with t = 1, 2, ... and the trainer's schedule on the
    very gradients each step left in the flat buffer reproduces that trainer's parameters, both moments and the bf16 shadow
    with torch.equal after every step."""
    from mobgt_amd import _lib
    from mobgt_amd.ops import _p, _stream
    from mobgt_amd.train import TrainStep
    real = _lib.lib()
    seen = []

    class _Spy:
        def __getattr__(self, name):
            seen.append(name)
            return getattr(real, name)
    res = []
    for kw in ({}, dict(accumulate=1, clip_norm=None)):
        model, batches = _setup(f32=(cfg == "f32"))
        monkeypatch.setattr(_lib, "lib", lambda: _Spy())
        del seen[:]
        ts = TrainStep(model, batches, use_graph=True, seed=5, **kw)
        ts.prepare()
        assert (ts.shadow_flat is None) == (cfg == "f32") and ts.sched_dev is not None
        n = ts.flat.flat.numel()
        rp = ts.flat_params.tensor.detach().clone()
        rm, rv = torch.zeros_like(rp), torch.zeros_like(rp)
        rsh = None if ts.shadow_flat is None else torch.zeros_like(ts.shadow_flat)
        cnt = torch.zeros(1, dtype=torch.int64, device=DEV)
        for i in range(5):
            ts.step(i)
            g = ts.flat.flat.detach().clone()
            cnt.add_(1)
            _lib.check(real.mobgt_adamw_flat(_p(rp), _p(g), _p(rm), _p(rv), _p(rsh), n, _p(ts.lr_dev), _p(ts.sched_dev), _p(cnt), 0,
                                             ts.betas[0], ts.betas[1], ts.eps, float(model.weight_decay), _stream()), "mobgt_adamw_flat")
            assert torch.equal(ts.flat_params.tensor.detach(), rp), i
            assert torch.equal(ts.exp_avg, rm) and torch.equal(ts.exp_avg_sq, rv), i
            if rsh is not None:
                assert torch.equal(ts.shadow_flat, rsh), i
        torch.cuda.synchronize()
        monkeypatch.setattr(_lib, "lib", lambda: real)
        assert float(rm.abs().max()) > 0
        assert ts.acc is None and ts.partials is None and ts.grad_norm is None and ts.upd_dev is None and not ts.graphs.of("update")
        assert ts.fused_opt and ts.updates_done == 5 and ts.window_pos == 0 and ts.sched_state["step_count"] == 6
        ts.flush()
        assert ts.updates_done == 5
        names = set(seen)
        assert "mobgt_adamw_flat" in names and "mobgt_step_prologue_skip" in names
        assert not names & {"mobgt_grad_accumulate", "mobgt_grad_norm_finish", "mobgt_adamw_flat_scaled"}, names
        res.append((sorted(names), rp, rm, rv, int(ts.seed_dev.item()), ts.lr))
    (na, pa, ma, va, ca, la), (nb, pb, mb, vb, cb, lb) = res
    assert na == nb and ca == cb and la == lb
    print(cfg, "the two trainers are bitwise equal after five steps:", torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb))


def test_overlap_form_and_bad_arguments_are_refused():
    from mobgt_amd.train import EpochLoop, TrainStep
    model, _ = _setup()
    for bad in (dict(accumulate=0), dict(clip_norm=0.0), dict(clip_norm=-1.0)):
        with pytest.raises(ValueError):
            TrainStep(None, [], **bad)
        with pytest.raises(ValueError):
            EpochLoop(model, None, [], **bad)
    for kw in (dict(accumulate=2), dict(clip_norm=1.0)):
        model, batches = _setup()
        with pytest.raises(NotImplementedError, match="overlap"):
            TrainStep(model, batches, use_graph=True, seed=5, overlap="force", **kw)


def test_epoch_loop_flushes_the_last_window_and_mixes_buckets():
    """EpochLoop(accumulate=4, clip_norm=...) over six batches: ceil(6 / 4) updates, the second from a flushed window of two;
    batches of different shape buckets share a window; no peer wait gave up."""
    from mobgt_amd import workloads
    from mobgt_amd.train import EpochLoop, TrainStep
    uni, model, coll = workloads.build("fsq", DEV, seed=1, model_overrides=dict(n_layers=2, peak_lr=2e-5, warmup_updates=4,
                                                                             tot_updates=100))
    data = [t for trajs in workloads.make_pool("fsq", 6, 16, uni, seed0=7000) for t in trajs]
    loop = EpochLoop(model, coll, data, batch_size=16, seed=3, use_graph=True, accumulate=4, clip_norm=0.5)
    order, real_step = [], TrainStep.step

    def spy(self, i):
        order.append(i)
        return real_step(self, i)
    TrainStep.step = spy
    try:
        seq = []
        res = loop.run_epoch(0, on_step=lambda k, l: seq.append(l))
    finally:
        TrainStep.step = real_step
    ts = loop.ts
    assert res["steps"] == 6 and len(order) == 6
    assert ts.updates_done == math.ceil(res["steps"] / 4) == 2 and ts.window_pos == 0
    assert int(ts.upd_dev.item()) == 2 and ts.sched_state["step_count"] == 3 and int(ts.seed_dev.item()) == 3 + 6
    assert len(loop.slots) >= 2 and len(set(order[:4])) >= 2, order        # several buckets inside the first window
    assert float(ts.acc.abs().max()) == 0.0 and math.isfinite(float(ts.grad_norm)) and float(ts.grad_norm) > 0
    assert all(math.isfinite(float(l)) for l in seq)
    assert ts.check_faults(on_fault="return") == {}
    res = loop.run_epoch(1, max_steps=3)                                    # a second epoch: 3 batches -> one flushed window
    assert ts.updates_done == 3 and ts.window_pos == 0


def test_guarded_step_rerun_counts_the_micro_step_once(monkeypatch):
    """A fault report (simulated: ops.peer_wait_faults patched to return one, once) on the micro-step that ends a window:
    guarded_step restores parameters, moments, accumulator, window position and update counter, re-captures and re-runs -- the
    counters read what an undisturbed run reads and the update moved the parameters once."""
    from mobgt_amd import forms, ops, workloads
    from mobgt_amd.train import TrainStep
    runs = {}
    try:
        for tag in ("undisturbed", "faulted"):
            uni, model, coll = workloads.build("fsq", DEV, seed=1, model_overrides=dict(n_layers=2))
            batches = [coll(t) for t in workloads.make_pool("fsq", 2, 16, uni)]
            ts = TrainStep(model, batches, use_graph=True, seed=1, accumulate=2, clip_norm=0.5)
            ts.prepare()
            p0 = ts.flat_params.tensor.detach().clone()
            real = ops.peer_wait_faults
            pending = [tag == "faulted"]
            calls = []

            def fake(reset=True, real=real, pending=pending, calls=calls, ts=ts):
                out = real(reset=reset)
                calls.append(ts.window_pos)
                if pending[0] and len(calls) == 2:          # the check behind the SECOND micro-step, the one that updated
                    pending[0] = False
                    return {"simulated": 1}
                return out
            monkeypatch.setattr(ops, "peer_wait_faults", fake)
            trace = []
            for i in range(3):
                ts.guarded_step(i)
                trace.append((ts.window_pos, ts.updates_done, int(ts.upd_dev.item()), int(ts.seed_dev.item()), ts.sched_state["step_count"]))
            monkeypatch.setattr(ops, "peer_wait_faults", real)
            assert ts.faults_recovered == (1 if tag == "faulted" else 0)
            runs[tag] = (trace, (ts.flat_params.tensor.detach() - p0).double(), ts.acc.clone(), float(ts.grad_norm))
            forms.set("safe_forms", None)
            ops.set_peer_wait_limit(0)
    finally:
        forms.set("safe_forms", None)
        ops.set_peer_wait_limit(0)
    (ta, da, acca, na), (tb, db, accb, nb) = runs["undisturbed"], runs["faulted"]
    print("counters", ta, tb, "norms", na, nb)
    assert ta == tb == [(1, 0, 0, 2, 1), (0, 1, 1, 3, 2), (1, 1, 1, 4, 2)]
    # one update each; the re-run took the forms without cross-workgroup waits (a few f32 sums in another order: DESIGN 7)
    assert float((da - db).norm() / da.norm()) <= 2e-2 and abs(na - nb) <= 2e-2 * na
    # the open window holds ONE micro-gradient: a micro-step added twice would show as a relative difference of order 1
    assert _rel(accb, acca) <= 0.1


# ---- data parallel -----------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_ranks(tmp_path, world, steps, extra_env):
    """Every rank a fresh child process (tests/_accum_worker.py)."""
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY="0", **extra_env)
        procs.append(subprocess.Popen([sys.executable, os.path.join(os.path.dirname(__file__), "_accum_worker.py"), str(tmp_path), str(steps)],
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
    assert all(p.returncode == 0 for p in procs), "\n".join(o[-4000:] for o in outs)
    return [torch.load(os.path.join(tmp_path, f"rank{r}.pt")) for r in range(world)]


CLIP_DDP = 0.05


def _assert_one_exchange_per_window(r, window_ends, flushed):
    """The collectives the worker counted itself (dist.all_reduce wrapped; the trainer's `exchanges_done` is not consulted): no
    micro-step graph holds one; in the captured form the update graph holds exactly one and the host issues none; in the
    host-exchange forms (gloo, MOBGT_DDP_HOST_EXCHANGE) the host issues exactly one in the call that ends a window and none in
    any other.  `window_ends`: per step() call whether it ended a window; `flushed`: whether flush() ended one."""
    ddp = r["forced"] or r["backend"] == "gloo" or r["one_graph"]
    assert r["all_reduce_in_micro_captures"] and not any(r["all_reduce_in_micro_captures"]), r["all_reduce_in_micro_captures"]
    if r["one_graph"]:
        assert r["all_reduce_in_update_captures"] == [1]
        assert not any(r["all_reduce_per_step"]) and r["all_reduce_in_flush"] == 0
    else:
        assert not any(r["all_reduce_in_update_captures"]) and len(r["all_reduce_in_update_captures"]) == 1
        want = [int(e and ddp) for e in window_ends]
        assert r["all_reduce_per_step"] == want and r["all_reduce_in_flush"] == int(flushed and ddp), (r["all_reduce_per_step"], want)
_SOLO = {}


def _solo_micro_gradients(tmp_path_factory):
    """The four micro-gradients ONE process computes alone: rank r's two batches from the broadcast initial parameters, dropout
    counters 1 and 2 (accumulate=2 holds the update back until both are taken)."""
    if not _SOLO:
        for r in (0, 1):
            d = tmp_path_factory.mktemp(f"solo{r}")
            _SOLO[r] = _run_ranks(d, 1, 2, {"MOBGT_TEST_ACCUM": "2", "MOBGT_TEST_DATA_RANK": str(r)})[0]
    return _SOLO


@pytest.mark.parametrize("comm", ["fp32", "bf16"])
def test_two_ranks_accumulate_two_equals_the_mean_of_four_solo_micro_gradients(tmp_path, tmp_path_factory, comm):
    """accumulate=2 over two ranks (RCCL with one GPU per rank where the box has two, else gloo with both on one GPU) is a
    global batch of four micro-batches: after the single update exp_avg / (1 - beta1) -- the gradient AdamW was fed -- is
    coef * the f64 mean of the four solo micro-gradients (gates of test_exchanged_gradient_is_the_mean_of_the_two_ranks_gradients),
    grad_norm is that mean's norm, torch.optim.AdamW on it gives the parameters (within 5 % of the movement, the gate of the
    bf16-exchange test), ONE exchange happened, and both ranks hold identical bits."""
    env = {"MOBGT_TEST_ACCUM": "2", "MOBGT_TEST_CLIP": str(CLIP_DDP)}
    if comm == "bf16":
        env["MOBGT_TEST_GRAD_COMM"] = "bf16"
    a, b = _run_ranks(tmp_path, 2, 2, env)
    solo = _solo_micro_gradients(tmp_path_factory)
    for r in (a, b):
        assert r["exchanges"] == 1 and r["updates"] == 1 and r["upd_dev"] == 1 and r["window_pos"] == 0 and r["acc_max"] == 0.0
        assert not r["overlap"] and r["one_graph"] == (r["backend"] == "nccl")
        _assert_one_exchange_per_window(r, [False, True], False)
    for k in ("params", "exp_avg", "exp_avg_sq", "grad_norm", "shadow"):
        assert torch.equal(a[k], b[k]), k
    assert a["losses"] != b["losses"]
    gate = 5e-3 if comm == "bf16" else 1e-5
    micro = [solo[0]["micro"][0], solo[0]["micro"][1], solo[1]["micro"][0], solo[1]["micro"][1]]
    # each rank really added ITS two micro-gradients (they are the solo ones up to f32 round-off)
    assert _rel(a["micro"][0], micro[0]) < 1e-3 and _rel(b["micro"][1], micro[3]) < 1e-3
    mean = sum(m.double() for m in micro) / 4
    total = float(mean.norm())
    coef = min(1.0, CLIP_DDP / (total + 1e-6))
    fed = a["exp_avg"].double() / (1.0 - 0.9)
    rel = _rel(fed, coef * mean)
    rel_n = abs(float(a["grad_norm"]) - total) / total
    print("backend", a["backend"], "one graph", a["one_graph"], "comm", a["comm_dtype"], "fed gradient vs coef * mean relL2 %.2e" % rel,
          "grad_norm %.6g vs %.6g (rel %.1e) coef %.4f" % (float(a["grad_norm"]), total, rel_n, coef))
    assert rel <= gate, rel
    assert rel_n <= gate + _norm_bound()
    for other in (micro[0].double(), 2 * mean, 4 * mean):            # not one micro-gradient, not an un-averaged sum
        assert _rel(fed, coef * other) > 0.2
    ref = torch.nn.Parameter(a["params0"].double().clone())
    opt = torch.optim.AdamW([ref], lr=2.5e-4, weight_decay=0.01)       # the worker's schedule at update 1: 1e-3 * 1 / 4
    ref.grad = coef * mean
    opt.step()
    move = (a["params"].double() - a["params0"].double())
    assert float(move.norm()) > 0
    assert float((a["params"].double() - ref.detach()).norm()) <= 0.05 * float(move.norm())


def test_one_forced_rccl_rank_exchanges_once_per_window(tmp_path):
    """MOBGT_FORCE_COMM=1 with a process group of ONE rank over RCCL: the captured form (the exchange is a node of the update
    graph) and the host-exchange form, four micro-steps + a fifth flushed: three windows, three exchanges; a sum over one rank
    changes nothing, so the parameters are those of the same worker without the forced exchange up to run-to-run noise."""
    runs = {}
    for tag, env in (("plain", {}), ("captured", {"MOBGT_FORCE_COMM": "1"}),
                     ("host", {"MOBGT_FORCE_COMM": "1", "MOBGT_DDP_HOST_EXCHANGE": "1"})):
        d = tmp_path / tag
        d.mkdir()
        runs[tag] = _run_ranks(d, 1, 5, dict(env, MOBGT_TEST_ACCUM="2", MOBGT_TEST_CLIP=str(CLIP_DDP)))[0]
    a = runs["plain"]
    assert a["exchanges"] == 0 and not a["forced"] and a["updates"] == 3
    _assert_one_exchange_per_window(a, [False, True, False, True, False], True)
    move = (a["params"] - a["params0"]).double()
    for tag in ("captured", "host"):
        r = runs[tag]
        assert r["backend"] == "nccl" and r["forced"] and r["one_graph"] == (tag == "captured")
        assert r["exchanges"] == 3 and r["updates"] == 3 and r["upd_dev"] == 3 and r["window_pos"] == 0 and r["acc_max"] == 0.0
        _assert_one_exchange_per_window(r, [False, True, False, True, False], True)
        assert all(np.isfinite(r["losses"]))
        np.testing.assert_allclose(r["losses"], a["losses"], rtol=2e-2)
        assert float(((r["params"] - r["params0"]).double() - move).norm()) <= 0.05 * float(move.norm())
        assert abs(float(r["grad_norm"]) - float(a["grad_norm"])) <= 5e-2 * float(a["grad_norm"])
