"""Train-step driver: what Lightning's fit loop + DDP plugin do for the reference (`entry.py:141-161`,
`model_fqandtoyo.py:1434-1478, 1599-1616`), written for one process per GPU over RCCL.

* `FlatGrads`: every trainable parameter's `.grad` is a view into ONE flat fp32 buffer, so zeroing is one
  memset and the data-parallel exchange is ONE all-reduce (RCCL over xGMI).  Parameters the model never
  uses (25 tensors in the fq variant) keep `grad = None`, exactly as under the reference, so
  AdamW skips them the same way.  DEVIATION (documented in DESIGN.md section 7): a parameter that is used by the model but
  receives no gradient on ONE particular batch has a zero-filled slot that step and is updated like any other slot (weight
  decay, moment decay, one global step count), where torch.optim.AdamW would skip it for that step and keep a per-parameter
  step count.  In the fq / stock models every trained parameter is reached on every batch (tables are reached row-wise:
  an untouched ROW has a zero gradient under the reference too), so the two agree; a model for which that does not hold
  should use `configure_optimizers()` instead of the flat kernel.
* `TrainStep`: forward + loss + backward (+ all-reduce) + AdamW + PolynomialDecayLR.  With
  `use_graph=True` the forward/backward and the optimizer step are captured in hipGraphs per batch
  (static shapes per pre-collated batch); the learning rate and the dropout seed live in device scalars
  so a replay sees new values without re-capture.
"""
import contextlib
import itertools
import os

import torch
import torch.distributed as dist

from . import forms, ops
from .restriction import Restriction
from .step_state import STEP
from .step_graphs import Entry, StepGraphs, group_key
from .model import sync_external_shadows
from .lr import polynomial_decay_lr
from .accum import UpdateWindow, check_accum_args, scheduled_lr


def flat_offsets(params, align=8):
    """Element offset of every parameter inside the flat buffers (each slot starts on a multiple of `align` elements,
    so f32 slices are 32-byte and bf16 shadow slices 16-byte aligned) and the total length.  A parameter may ask for unused
    elements behind its slot (`p._mobgt_flat_slack`): a weight-gradient kernel whose operand is zero-padded by a column (the
    distance GCN's 303-wide first layer as 304 columns) writes one more row of (zero) products than the parameter has, straight
    into its gradient sink.  (Slack behind EVERY slot would separate q / k / v and the small per-layer gradients, which the fused
    layers need adjacent.)"""
    offs, off = [], 0
    for p in params:
        offs.append(off)
        off += (p.numel() + int(getattr(p, "_mobgt_flat_slack", 0)) + align - 1) // align * align
    return offs, off


class FlatGrads:
    def __init__(self, params, dtype=torch.float32):
        self.params = [p for p in params if p.requires_grad]
        self.offsets, n = flat_offsets(self.params)
        dev = self.params[0].device
        self.flat = torch.zeros(n, dtype=dtype, device=dev)
        self.views = [self.flat[o:o + p.numel()].view_as(p) for p, o in zip(self.params, self.offsets)]
        self.attach()

    def attach(self):
        for p, v in zip(self.params, self.views):
            p.grad = v

    def zero(self):
        self.flat.zero_()

    def release(self):
        """Before backward: drop the views so autograd hands over its freshly computed gradient tensors
        instead of launching one `grad += new` kernel per parameter (~130 tiny launches per step)."""
        for p in self.params:
            p.grad = None

    def gather(self, start=0, stop=None, grads=None):
        """After backward: one multi-tensor copy of the gradients of params[start:stop] into the flat buffer
        (`grads`: explicit gradient tensors, e.g. from torch.autograd.grad), then re-attach those views."""
        stop = len(self.params) if stop is None else stop
        ps, vs = self.params[start:stop], self.views[start:stop]
        if grads is None:
            grads = [p.grad for p in ps]
        for k in getattr(self, "zero_if_missing", ()):        # slots the per-step zeroing skips (TrainStep._skip)
            if start <= k < stop and grads[k - start] is None:
                vs[k - start].zero_()
        # nothing to copy for a gradient that was written in place (ops.grad_sink) or that does not exist (the flat
        # buffer is zeroed before every backward)
        todo = [(v, g) for g, v in zip(grads, vs) if g is not None and g.data_ptr() != v.data_ptr()]
        if todo:
            torch._foreach_copy_([v for v, _ in todo], [g for _, g in todo])
        for p, v in zip(ps, vs):
            p.grad = v

    def all_reduce_mean(self, group=None):
        """mean of the gradients over ranks (DDP semantics); no-op for world size 1."""
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            dist.all_reduce(self.flat, op=dist.ReduceOp.SUM, group=group)
            self.flat.div_(dist.get_world_size(group))


def head_parameters(model, used):
    """The used parameters of `model.head_modules` (gradient complete once the backward has reached the encoder
    output), in `used` order; [] when the model does not declare a head."""
    names = getattr(model, "head_modules", ())
    ids = set()
    for n in names:
        m = getattr(model, n, None)
        if m is not None:
            ids |= {id(p) for p in m.parameters()}
    return [p for p in used if id(p) in ids]


def flat_order(model, used):
    """Order of the used parameters inside the flat buffers: the head's parameters first (one contiguous bucket
    whose all-reduce can start early), then the encoder layers from the LAST to the FIRST -- the order in which the backward
    pass completes their gradients, so that "everything up to layer k" is one growing prefix of the buffer and can be
    all-reduced while the layers below are still in their backward (TrainStep's layer-wise buckets) -- each layer as one
    contiguous run: q/k/v weights adjacent (the fused [3C, C] projection storage is then one slice of the flat parameter
    buffer), the block of small gradients, then the layer's remaining weights; then the rest."""
    used_ids = {id(p) for p in used}
    order, seen = [], set()
    for p in head_parameters(model, used):
        order.append(p)
        seen.add(id(p))
    def take(grp):
        if all(id(p) in used_ids and id(p) not in seen for p in grp):
            for p in grp:
                order.append(p)
                seen.add(id(p))
            return True
        return False
    layers = [m for m in model.modules() if hasattr(m, "self_attention") and hasattr(m, "ffn")]
    attn_done = set()
    for layer in reversed(layers):
        # an encoder layer: q/k/v weights, then -- in the order of the fused backward's block of small gradients
        # (fused_layer._FusedLayerFn.backward) -- q/k/v biases, output bias, FFN biases, the two LayerNorms: that block
        # is then ONE slice of the flat gradient buffer and nothing of it needs a gather copy
        m = layer.self_attention
        if not all(hasattr(m, a) for a in ("linear_q", "linear_k", "linear_v", "output_layer")):
            continue
        n1, nx = ((layer.ffn_norm1, layer.ffn_norm2) if hasattr(layer, "ffn_norm1")
                  else (getattr(layer, "ffn_norm", None), getattr(layer, "self_attention_norm", None)))
        if n1 is None or nx is None:
            continue
        if take([m.linear_q.weight, m.linear_k.weight, m.linear_v.weight, m.linear_q.bias, m.linear_k.bias, m.linear_v.bias,
                 m.output_layer.bias, layer.ffn.layer1.bias, layer.ffn.layer2.bias, n1.weight, n1.bias, nx.weight, nx.bias]):
            attn_done.add(id(m))
            for p in layer.parameters():              # the rest of this layer (Wo, W1, W2): behind its group, same bucket
                if id(p) in used_ids and id(p) not in seen:
                    order.append(p)
                    seen.add(id(p))
    for m in model.modules():
        if id(m) not in attn_done and all(hasattr(m, a) for a in ("linear_q", "linear_k", "linear_v")):
            take([m.linear_q.weight, m.linear_k.weight, m.linear_v.weight, m.linear_q.bias, m.linear_k.bias, m.linear_v.bias])
    return order + [p for p in used if id(p) not in seen]


class FlatParams:
    """All trained parameters as views of ONE fp32 buffer (same order as FlatGrads): AdamW becomes a single fused
    launch over one tensor instead of a multi-tensor sweep over ~130.  Parameter objects, names and values are
    unchanged (state_dict keeps working); untrained parameters are left alone, as the reference's optimizer
    skips them (their grad is None)."""

    def __init__(self, model, params):
        self.params = params
        self.offsets, n = flat_offsets(params)
        flat = torch.zeros(n, dtype=torch.float32, device=params[0].device)
        with torch.no_grad():
            for p, off in zip(params, self.offsets):
                v = flat[off:off + p.numel()].view_as(p)
                v.copy_(p.data)
                p.data = v
        self.tensor = torch.nn.Parameter(flat)
        # re-point the attention modules' fused-QKV handles at the new storage
        for m in model.modules():
            if hasattr(m, "fuse_qkv_storage") and hasattr(m, "_wqkv"):
                w, b = m.linear_q.weight, m.linear_q.bias
                C = w.shape[0]
                nxt_w = m.linear_k.weight.data_ptr() == w.data_ptr() + w.numel() * 4
                nxt_b = m.linear_k.bias.data_ptr() == b.data_ptr() + b.numel() * 4
                if nxt_w and nxt_b:
                    wo = (w.data_ptr() - flat.data_ptr()) // 4
                    bo = (b.data_ptr() - flat.data_ptr()) // 4
                    m._wqkv = flat[wo:wo + 3 * C * w.shape[1]].view(3 * C, w.shape[1])
                    m._bqkv = flat[bo:bo + 3 * C]


def used_parameters(model, loss_fns):
    """Dry-run backward passes: the parameters that receive a gradient from ANY of them (the others stay grad=None,
    as under the reference, whose optimizer then skips them).  `loss_fns`: one callable per pre-collated batch -- a
    parameter may be reached on some batches only."""
    if callable(loss_fns):
        loss_fns = [loss_fns]
    hit = set()
    ops.sink_census_begin()
    try:
        for fn in loss_fns:
            for p in model.parameters():
                p.grad = None
            ops.sink_census_pass()
            fn().backward()
            hit |= {id(p) for p in model.parameters() if p.grad is not None}
    finally:
        census = ops.sink_census_end()
    for p in model.parameters():
        p.grad = None
    used = [p for p in model.parameters() if id(p) in hit]
    # parameters whose gradient has MORE than one producer per pass (tied / re-applied modules): no in-place sink
    # (ops.grad_sink: the producers would overwrite each other and autograd would add a buffer to itself)
    for p in used:
        p._mobgt_multi_use = census.get(id(p), 0) > 1
    return used


def recommended_env():
    """Environment a data-parallel process should set BEFORE `init_process_group("nccl")` when its steps are captured graphs
    (bench.py and the tests' workers do): c10d's event cache off -- a recycled event that was last recorded inside a capture must
    never reach the watchdog's polling (see TrainStep._quiesce_collectives)."""
    return {"TORCH_NCCL_CUDA_EVENT_CACHE": "0"}


def broadcast_parameters(model, src=0):
    """DDP's construction-time broadcast: every rank starts from rank `src`'s weights."""
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        for t in list(model.parameters()) + list(model.buffers()):
            dist.broadcast(t.data, src)
        sync_external_shadows(model)


def assert_same_across_ranks(digest, what, device=None):
    """All-gather `digest` (bytes, same length everywhere) over the default process group; every rank raises RuntimeError
    naming the ranks that differ from rank 0.  No-op without a process group or with one rank."""
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() <= 1:
        return
    world = dist.get_world_size()
    mine = torch.frombuffer(bytearray(digest), dtype=torch.uint8).clone()
    if dist.get_backend() == "nccl":
        mine = mine.to(device if device is not None else torch.device("cuda", torch.cuda.current_device()))
    got = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(got, mine)
    got = [t.cpu() for t in got]
    bad = [r for r, t in enumerate(got) if not torch.equal(t, got[0])]
    if bad:
        raise RuntimeError(f"mobgt: {what} differs between rank 0 and ranks {bad} -- refusing to all-reduce")


def choose_ddp_form(model, batches, steps=20, warmup=5, candidates=None, **ts_kw):
    """Which form of the data-parallel step is the fastest ON THIS JOB'S RANKS (VERDICT r5 next #7b): every candidate
    -- the one-graph step with the exchange captured on the step's stream (host-issued over gloo), the two-phase overlap, the
    layer-wise overlap in three parts -- is built, prepared and timed for `steps` steps behind a barrier (MAX over ranks), the
    model's parameters are put back after each, and all ranks agree on the choice (`assert_same_across_ranks`).
    -> (name, TrainStep constructor arguments incl. the environment to set, {name: ms per step}).  With one rank or no process
    group: the default form, nothing timed.  No multi-GPU node has run this yet: the forms' order there is the measurement this
    function exists to make (the one-rank figures of rounds 4-5 cannot show what an overlap hides).  With `accumulate > 1` or
    `clip_norm` among the TrainStep arguments the overlap forms are not candidates (TrainStep does not build them)."""
    import time
    cands = candidates or [("one_graph", dict(overlap=False), {}),
                           ("overlap_2", dict(overlap="force"), {"MOBGT_DDP_PARTS": "1"}),
                           ("overlap_3", dict(overlap="force"), {"MOBGT_DDP_PARTS": "3"})]
    if candidates is None and (ts_kw.get("accumulate", 1) != 1 or ts_kw.get("clip_norm") is not None):
        cands = cands[:1]
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() <= 1:
        return cands[0][0], cands[0][1], {}
    dev = next(model.parameters()).device
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    saved_env = {k: os.environ.get(k) for _, _, env in cands for k in env}
    timings = {}
    for name, kw, env in cands:
        for k, v in env.items():
            os.environ[k] = v
        try:
            ts = TrainStep(model, batches, **dict(ts_kw, **kw))
            ts.prepare()
            for i in range(warmup):
                ts.step(i)
            torch.cuda.synchronize(dev)
            dist.barrier()
            t0 = time.perf_counter()
            for i in range(steps):
                ts.step(warmup + i)
            torch.cuda.synchronize(dev)
            el = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev if dist.get_backend() == "nccl" else "cpu")
            dist.all_reduce(el, op=dist.ReduceOp.MAX)
            timings[name] = float(el.item()) / steps * 1e3
            faults = ts.check_faults(on_fault="return")
            if faults:
                timings[name] = float("inf")
        finally:
            for k, v in saved_env.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        with torch.no_grad():
            model.load_state_dict(sd0)
        del ts
    best = min(timings, key=lambda n: (timings[n], n))
    assert_same_across_ranks(best.encode().ljust(16, b" "), "the chosen data-parallel step form", dev)
    kw, env = next((kw, env) for n, kw, env in cands if n == best)
    return best, dict(kw, _env=env), timings


class TrainStep:
    def __init__(self, model, batches, autocast_dtype=None, use_graph=True, seed=1, overlap=True, batch_fn=None,
                 grad_comm_dtype=None, keep_head_rows=False, accumulate=1, clip_norm=None):
        """`batches`: pre-collated batches resident on the device (their tensors are the static inputs of the captured
        graphs).  `batch_fn`: optional callable applied to a batch INSIDE the step (and so inside its graph) before the model
        sees it -- `EpochLoop` passes raw, un-collated arrays + `DeviceCollator.finish`, so that collating a fresh batch is
        part of the replayed step.  More batches can be added after `prepare()` with `add_batch`.

        `accumulate=k` (Lightning's `accumulate_grad_batches`): every `step(i)` is a micro-step -- forward, loss, backward, add
        into the window -- and the k-th one of a window also updates, from `sum / k`; `flush()` ends a short window (divisor
        still k).  `clip_norm=c` (Lightning's `gradient_clip_val`, norm clipping): the update's gradient is scaled by
        `min(1, c / (||g||_2 + 1e-6))` on the device (`torch.nn.utils.clip_grad_norm_`); `grad_norm` holds `||g||_2` before
        clipping.  The dropout stream advances per micro-step; AdamW's t and the schedule advance per UPDATE (`updates_done`).
        Data parallel: ONE exchange per window, of the accumulated gradient, before the norm -- built for the captured
        (`one_graph`) and the host-exchange forms; the `overlap` form raises NotImplementedError with `accumulate > 1` or
        `clip_norm`.  `accumulate=1, clip_norm=None` (the default) is the plain step: no accumulator, no extra launch."""
        self.accumulate, self.clip_norm = check_accum_args(accumulate, clip_norm)
        self._accum = self.accumulate > 1 or self.clip_norm is not None
        self.model = model
        self.batches = list(batches)
        self.batch_fn = batch_fn
        self.keep_head_rows = bool(keep_head_rows)      # tests: TrainStep.enc_outs[i] = graph-token rows of batch i's last step
        # torch.bfloat16: the gradient exchange moves bf16 (half the bytes over xGMI; RCCL then also SUMS in bf16 -- 8 ranks:
        # relative error ~2^-8 per element on top of the gradient's own bf16-operand noise); the result is widened back
        # into the fp32 flat buffer the optimizer reads.  Default None: fp32 exchange (what the parity tests pin).
        self.grad_comm_dtype = grad_comm_dtype
        self.autocast_dtype = autocast_dtype
        dev = next(model.parameters()).device
        self.device = dev
        self.seed_dev = torch.tensor([seed], dtype=torch.int64, device=dev)
        for m in model.modules():
            if hasattr(m, "seed_dev"):
                m.seed_dev = self.seed_dev
        from . import ops
        ops.set_dropout_state(self.seed_dev, seed)
        # room for every gradient that kernels accumulate into (all but the few huge matrices torch's GEMMs write)
        n_arena = sum(p.numel() for p in model.parameters() if p.numel() <= (1 << 16))
        self.arena = ops.ZeroArena(dev, n=(max(1 << 21, int(n_arena * 1.5) + (1 << 18)) + 3) // 4 * 4)
        model.train()
        # A model that already ran a backward pass on another stream may still hold that autograd graph (the fq model
        # keeps its encoder output in `_enc_out`), and with it AccumulateGrad nodes bound to THAT stream; captured on
        # ours they would put cross-stream waits into the graph (observed: abort in capture_end).  Let go of it first.
        if getattr(model, "_enc_out", None) is not None:
            model._enc_out = None
        model._bias_pack, model._cuts = None, {}
        for l in getattr(model, "layers", []):
            l._mobgt_cut = False
        for p in model.parameters():
            p.grad = None
        import gc
        gc.collect()
        # One side stream for the dry run, the warm-ups and every capture: autograd's AccumulateGrad nodes are
        # created on the stream of the first backward and must match the capture stream later on.
        self.stream = torch.cuda.Stream(device=dev) if use_graph else None
        with self._on_stream():
            used = used_parameters(model, [lambda b=b: self._loss(b) for b in batches])
        used = flat_order(model, used)
        self.flat = FlatGrads(used)
        self.n_head = len(head_parameters(model, used))              # params[:n_head] = the early bucket
        self.n_head_elems = self.flat.offsets[self.n_head] if self.n_head < len(used) else self.flat.flat.numel()
        self.flat_params = FlatParams(model, used)
        # big gradients are written in place (no gather copy) -- except those of parameters that more than one autograd
        # node produces per pass (`used_parameters`' census): they keep torch's accumulate-then-copy path
        single = [(p, v) for p, v in zip(self.flat.params, self.flat.views) if not getattr(p, "_mobgt_multi_use", False)]
        self.sinkless = [p for p in self.flat.params if getattr(p, "_mobgt_multi_use", False)]
        ops.set_grad_sinks([p for p, _ in single], [v for _, v in single])
        # ... and a model that has such parameters runs its backward WITHOUT deferred weight-gradient launches: a deferred
        # producer returns its buffer before the grouped launch fills it, and autograd would sum two still-empty buffers
        self._defer = not self.sinkless
        # The classifier's weight gradient (61 % of the S-FSQ model's gradient bytes) is OVERWRITTEN in full by every backward
        # pass -- by the skinny weight-gradient kernel writing into its sink, or by the gather's copy of a library result --
        # so the per-step zeroing leaves that slice alone (it is zeroed by hand in the one case nothing writes it: a step in
        # which the parameter received no gradient)
        self._skip = None
        w = getattr(getattr(model, "out_proj", None), "weight", None)
        if w is not None:
            for i, q in enumerate(self.flat.params):
                if q is w and w.numel() >= (1 << 20):
                    self._skip = (i, int(self.flat.offsets[i]), int(self.flat.offsets[i]) + w.numel())
                    self.flat.zero_if_missing = (i,)
        self.flat_params.tensor.grad = self.flat.flat
        self.lr_dev = torch.tensor(float(model.peak_lr), dtype=torch.float32, device=dev)
        # AdamW (model_fqandtoyo.py:1599-1616 defaults) as ONE kernel over the flat buffers that also refreshes the bf16
        # shadow weights the layer GEMMs read (csrc/layer.hip: mobgt_adamw_flat); its step count is the per-step device
        # counter `seed_dev` minus a base fixed at the first optimizer call
        n = self.flat.flat.numel()
        self.exp_avg = torch.zeros(n, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(n, dtype=torch.float32, device=dev)
        self.shadow_flat = None
        self.shadow_flat = self._attach_shadows()
        self._step_base = None
        self.betas, self.eps = (0.9, 0.999), 1e-8
        self.sched_state = dict(step_count=1, warmup=model.warmup_updates, tot=model.tot_updates, lr=model.peak_lr,
                                end_lr=model.end_lr, power=1.0)
        # PolynomialDecayLR with power 1 is evaluated inside the optimizer kernel from the device step counter (no
        # per-step host write of the learning rate); `lr_dev` mirrors it for inspection and serves any other schedule
        s = self.sched_state
        # (5th entry: offset between the kernel's step count t and the schedule's step_count; both start at 1)
        self.sched_dev = torch.tensor([float(s["warmup"]), float(s["tot"]), float(s["lr"]), float(s["end_lr"]), 0.0],
                                      dtype=torch.float32, device=dev) if s["power"] == 1.0 and s["warmup"] > 0 else None
        self.window = UpdateWindow(self.accumulate)
        self._set_lr()
        self.use_graph = use_graph
        self.graphs = StepGraphs()                            # every captured hipGraph of this trainer (step_graphs.py)
        self.fused_opt = False                                # prepare(): AdamW rides at the end of every batch's step graph
        self.faults_recovered = 0
        self._loss_ref = torch.zeros((), device=dev)          # the loss tensor of the step that ran last
        self.world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        # MOBGT_FORCE_COMM=1 (tests): a process group of ONE rank takes the data-parallel path -- buckets, exchange on the
        # collective's stream, bf16 exchange buffer -- so that the RCCL ("nccl") branch executes on a one-GPU box
        self.force_comm = (forms.on("force_comm") and dist.is_available() and dist.is_initialized())
        self.ddp = self.world > 1 or self.force_comm
        # Data parallel, three forms of one step:
        #  * default over RCCL -- `one_graph`: the WHOLE step is one hipGraph per batch: forward, backward, the gradient
        #    all-reduce issued on the step's OWN stream (a synchronous c10d collective runs on the caller's stream; inside a
        #    capture it becomes a node of the graph: no second stream, no cross-stream edge, no host call between replays),
        #    the average and AdamW.  The exchange is serial with the backward -- nothing hides it -- but the step carries no
        #    structure cost: round 4's four-replay form cost +25 % before any wire time (0.577 -> 0.724 ms with one forced
        #    rank), more than the overlap can win back on a 0.6 ms step;
        #  * MOBGT_DDP_OVERLAP=1 (or overlap="force": tests) -- `overlap`: the backward split at the encoder output (and, with
        #    MOBGT_DDP_PARTS > 1, in front of a few layers) into graphs replayed one after the other, every completed slice
        #    of the flat buffer all-reduced asynchronously on RCCL's stream beside the next replay;
        #  * gloo (host collectives are not capturable) or MOBGT_DDP_HOST_EXCHANGE=1: forward + backward graph, all-reduce
        #    issued by the host, optimizer graph.
        want_overlap = overlap == "force" or (bool(overlap) and forms.on("ddp_overlap"))
        self.overlap = bool(want_overlap and use_graph and (self.ddp or overlap == "force") and self.n_head > 0
                            and hasattr(model, "_enc_out"))
        if self.overlap and self._accum:
            raise NotImplementedError("TrainStep: accumulate > 1 / clip_norm are not built for the `overlap` form of the data-parallel "
                                      "step (its exchange runs beside the backward of every micro-step); use the default form")
        self.enc_outs = {}
        self._plan_buckets()
        self.one_graph = bool(self.ddp and use_graph and not self.overlap and dist.get_backend() == "nccl"
                              and not forms.on("ddp_host_exchange"))
        self.comm = True        # False: skip the gradient exchange (bench.py measures the exposed all-reduce time that way)
        self._prepared = False
        self.comm_buf = (torch.empty(self.flat.flat.numel(), dtype=grad_comm_dtype, device=dev)
                         if (grad_comm_dtype is not None and self.ddp) else None)
        # Accumulation / clipping: the window's accumulator (all zeros between windows: the scaled AdamW pass zeroes
        # it behind itself), the slab of per-block sums of squares, and the device scalars of an update -- its gradient norm,
        # the scale 1/k * coef the optimizer applies, and the per-UPDATE counter AdamW's t and the in-kernel schedule read.
        # With k = 1 (clipping only) the flat gradient buffer itself is what the update consumes.
        self.acc = self.partials = self.grad_norm = self.scale_dev = self.upd_dev = None
        self.exchanges_done = 0
        if self._accum:
            n = self.flat.flat.numel()
            from . import _lib
            self.acc = torch.zeros(n, dtype=torch.float32, device=dev) if self.accumulate > 1 else None
            self._gsrc = self.acc if self.acc is not None else self.flat.flat
            if self.clip_norm is not None:
                blk = int(_lib.lib().mobgt_grad_norm_block())
                self.partials = torch.zeros((n + blk - 1) // blk, dtype=torch.float32, device=dev)
                self.grad_norm = torch.zeros((), dtype=torch.float32, device=dev)
            self.scale_dev = torch.full((), 1.0 / self.accumulate, dtype=torch.float32, device=dev)
            self.upd_dev = torch.zeros(1, dtype=torch.int64, device=dev)
        self.check_layout_across_ranks()

    @property
    def updates_done(self):
        """Optimizer updates issued so far (host integer)."""
        return self.window.updates_done

    @property
    def window_pos(self):
        """Micro-steps in the open accumulation window (0 right after an update)."""
        return self.window.window_pos

    def _plan_buckets(self):
        """Layer-wise gradient buckets (data parallel; VERDICT r3 next #3a).  `flat_order` lays the buffers out as
        [head | layer L-1 | ... | layer 0 | rest]: the order in which the backward pass completes the gradients.  Phase B -- the
        backward from the encoder output down -- is cut in front of a few layers into PARTS, each its own hipGraph over the one
        autograd graph (torch.autograd.grad from the previous cut's gradient to the next cut's activation + that part's
        parameters); after every part the slice of the flat buffer it completed is all-reduced on RCCL's stream while the next
        part replays.  What is exposed at the end is the LAST bucket only (node features, GCNs, embedding and bias tables: a few
        MB) instead of everything behind the head (39 % of the bytes in round 3).  `self.parts`: [(cut layer or None, first
        parameter, end parameter, first element, end element)], in execution order; [] = the single phase B of round 3.
        MOBGT_DDP_PARTS: number of parts (default 1 = the single phase B; the layer-wise parts have run over RCCL with one rank
        and over gloo with two, never on a multi-GPU node: ADVICE r4)."""
        self.parts = []
        layers = list(getattr(self.model, "layers", []))
        n_parts = int(os.environ.get("MOBGT_DDP_PARTS", "1"))
        if not self.overlap or len(layers) < 2 or n_parts < 2:
            return
        pos = {id(p): i for i, p in enumerate(self.flat.params)}
        runs, at = [], self.n_head
        for li in reversed(range(len(layers))):
            idx = sorted(pos[id(p)] for p in layers[li].parameters() if id(p) in pos)
            if not idx or idx != list(range(at, at + len(idx))):
                return                               # (a layer whose parameters are not one run behind its successor's: keep one phase B)
            at += len(idx)
            runs.append((li, idx[0], at))
        # layer groups of (nearly) equal size, top of the stack first; the last part takes what is left of the model
        n_grp = min(n_parts - 1, len(runs))
        cuts = [runs[(g + 1) * len(runs) // n_grp - 1] for g in range(n_grp)]      # the LOWEST layer of each group
        offs = list(self.flat.offsets) + [self.flat.flat.numel()]
        lo = self.n_head
        for li, _, hi in cuts:
            self.parts.append((li, lo, hi, int(offs[lo]), int(offs[hi])))
            layers[li]._mobgt_cut = True
            lo = hi
        n = len(self.flat.params)
        self.parts.append((None, lo, n, int(offs[lo]), int(offs[n])))

    def layout_digest(self):
        """Hash of what every rank must agree on before one flat buffer can be all-reduced: which parameters are trained,
        in which order, at which offsets (`used_parameters` is computed per rank from that rank's own batches)."""
        import hashlib
        names = {id(p): n for n, p in self.model.named_parameters()}
        h = hashlib.sha256()
        for p, off in zip(self.flat.params, self.flat.offsets):
            h.update(("%s:%d:%d;" % (names.get(id(p), "?"), off, p.numel())).encode())
        h.update(("n=%d;head=%d;parts=%s" % (self.flat.flat.numel(), self.n_head_elems, [p[1:] for p in self.parts])).encode())
        return h.digest()[:8]

    def check_layout_across_ranks(self):
        """All-gather the layout digest and abort on a mismatch (a rank whose dry-run batches never reach some parameter
        would otherwise all-reduce a differently laid out buffer: silent garbage)."""
        assert_same_across_ranks(self.layout_digest(), "flat parameter / gradient layout (different sets of trained parameters?)",
                                 self.device)

    def _attach_shadows(self):
        """bf16 copy of the whole flat parameter buffer; the fused layers' shadow weights become views of it, kept
        current by the optimizer kernel instead of a per-step multi-tensor copy (model.refresh_shadows skips them)."""
        layers = [l for l in getattr(self.model, "layers", []) if getattr(l, "fused", False)
                  and getattr(l, "act_dtype", torch.float32) == torch.bfloat16]
        if not layers:
            return None
        flat = self.flat_params.tensor.detach()
        shadow = flat.to(torch.bfloat16)
        base = flat.data_ptr()
        plan = []
        for layer in layers:
            mha = layer.self_attention
            wqkv, bqkv = mha.fuse_qkv_storage()
            masters = (wqkv, bqkv, mha.output_layer.weight, mha.output_layer.bias, layer.ffn.layer1.weight,
                       layer.ffn.layer1.bias, layer.ffn.layer2.weight, layer.ffn.layer2.bias)
            views = []
            for m in masters:
                off = (m.data_ptr() - base) // 4
                if off < 0 or off + m.numel() > flat.numel() or not m.is_contiguous():
                    return None                      # not a slice of the flat buffer: every layer keeps its own copies
                views.append(shadow[off:off + m.numel()].view(m.shape))
            plan.append((layer, tuple(views)))
        for layer, views in plan:                    # all layers validated: only now hand the views over
            layer._shadows = views
            layer._shadow_external = True
        import weakref
        self.model._shadow_sync = weakref.WeakMethod(self.sync_shadows)
        return shadow

    def sync_shadows(self):
        """Re-derive the bf16 shadow weights from the fp32 masters.  The optimizer kernel keeps them current step by
        step; anything ELSE that writes parameters after this TrainStep was built (checkpoint load, broadcast, manual
        edits) must call this (checkpoint.load_lightning_checkpoint and train.broadcast_parameters do)."""
        if self.shadow_flat is not None:
            with torch.no_grad():
                self.shadow_flat.copy_(self.flat_params.tensor)

    def _opt_step(self):
        from . import _lib
        from .ops import _p, _stream
        if self._step_base is None:                  # t = 1 on this very call; the counter advances once per step
            self._step_base = int(self.seed_dev.item()) - 1
        n = self.flat.flat.numel()
        _lib.call("mobgt_adamw_flat", _p(self.flat_params.tensor), _p(self.flat.flat), _p(self.exp_avg),
                  _p(self.exp_avg_sq), _p(self.shadow_flat), n, _p(self.lr_dev),
                  _p(self.sched_dev), _p(self.seed_dev), self._step_base, self.betas[0],
                  self.betas[1], self.eps,
                  float(self.model.weight_decay), _stream())

    def _capturing(self, graph):
        """torch.cuda.graph on the trainer's stream.  With a process group, captures use the THREAD-LOCAL error mode: c10d's
        watchdog thread polls the events of earlier collectives (the layout all-gather, the eager warm-up exchange) with
        hipEventQuery, which the default global mode turns into an error of that thread while THIS one is capturing -- the
        process then dies in the watchdog (seen once in six runs of tests/test_gpu_train.py::test_rccl_branch_executes_on_one_gpu)."""
        if self.ddp:
            self._quiesce_collectives()
        return torch.cuda.graph(graph, stream=self.stream, capture_error_mode="thread_local" if self.ddp else "global")

    def _quiesce_collectives(self):
        """Let c10d's watchdog retire every eager collective before a capture starts (device idle, then two of its 100 ms polling
        rounds): a step graph captures a collective, and a watchdog that still polls events while events are being recorded into
        a capture has been seen to die on `hipErrorCapturedEvent` (one run in six; an event it held was recorded inside the
        capture -- c10d recycles its events through a cache, `TORCH_NCCL_CUDA_EVENT_CACHE=0` in `recommended_env()` switches that
        off).  Costs 0.25 s per captured graph, once."""
        import time
        if not getattr(TrainStep, "_env_warned", False) and dist.get_backend() == "nccl":
            missing = {k: v for k, v in recommended_env().items() if os.environ.get(k) != v}
            if missing:
                # (the pause below is a timing heuristic; what removes the race is the watchdog not recycling events)
                import warnings
                TrainStep._env_warned = True
                warnings.warn(f"mobgt TrainStep: capturing a step graph under a process group without {missing} in the environment "
                              "(train.recommended_env(), to be set BEFORE init_process_group): c10d's watchdog may poll an event that "
                              "is being recorded into the capture")
        torch.cuda.synchronize(self.device)
        time.sleep(0.25)

    def _on_stream(self):
        import contextlib
        if self.stream is None:
            return contextlib.nullcontext()
        self.stream.wait_stream(torch.cuda.current_stream())
        return torch.cuda.stream(self.stream)

    def _join(self):
        if self.stream is not None:
            torch.cuda.current_stream().wait_stream(self.stream)

    # learning rate of lr.py:17-31, kept in a device scalar so captured optimizer graphs see it
    def _set_lr(self):
        self.lr = scheduled_lr(self.sched_state)
        if self.sched_dev is None:
            self.lr_dev.fill_(self.lr)

    def _loss(self, batch):
        if self.batch_fn is not None:
            batch = self.batch_fn(batch)
        if self.autocast_dtype is not None:
            with torch.autocast(device_type="cuda", dtype=self.autocast_dtype):
                return self.model.training_step(batch, 0)
        return self.model.training_step(batch, 0)

    def _prologue(self):
        """Zero the flat gradient buffer (in-place gradient sinks accumulate into it; unused slots stay zero) and the
        zero arena (all small zero-initialised accumulators of the step), advance the step counter (new dropout masks,
        AdamW's t): one launch."""
        from . import _lib
        from .ops import _p, _stream
        self.flat.release()
        self.arena.off = 0
        ops.set_zero_arena(self.arena)             # valid from here to the end of this backward pass only
        lo, hi = (self._skip[1], self._skip[2]) if self._skip is not None else (0, 0)
        _lib.call("mobgt_step_prologue_skip", _p(self.flat.flat), self.flat.flat.numel(), lo, hi, _p(self.arena.buf),
                  self.arena.buf.numel(), _p(self.seed_dev), _stream())

    def _fwd_bwd(self, batch, rows=None):
        """Prologue, forward, loss, backward -> the detached loss: it stays where the loss kernel wrote it (inside a capture the
        graph's static output, no copy launch)."""
        self._prologue()
        loss = self._loss(batch)
        if rows is not None and self.keep_head_rows and getattr(self.model, "_enc_out", None) is not None:
            # (parity tests: a copy of the encoder output's graph-token rows -- what the classifier head reads -- as one more node
            #  of this batch's graph; the encoder output itself is overwritten in place by the backward pass)
            self.enc_outs[rows] = self.model._enc_out[:, 0, :].detach().clone()
        with ops.recording_wgrads(self._defer):  # leaf weight gradients are recorded and issued as ONE launch behind the pass,
            loss.backward(gradient=ops.unit_grad(loss.device))                                # before anything reads a gradient
        ops.set_zero_arena(None)
        left = ops.step_state_leftovers()
        if left:
            raise RuntimeError(f"mobgt: the step left parked work behind {left} -- its gradients are incomplete (another model's "
                               "forward / backward inside this step?)")
        self.flat.gather()
        return loss.detach()

    @property
    def loss_out(self):
        return self._loss_ref

    # ---- the same step in two phases (data parallel): [forward, loss, head backward] | [rest of the backward]; what one phase
    # hands to the next is (a tensor of the autograd graph, its gradient)
    def _phase_a(self, batch):
        self._prologue()
        loss = self._loss(batch)
        enc = self.model._enc_out
        head = self.flat.params[:self.n_head]
        with ops.recording_wgrads(self._defer):
            grads = torch.autograd.grad(loss, head + [enc], grad_outputs=ops.unit_grad(loss.device), allow_unused=True)   # frees only the nodes it ran
        self.flat.gather(0, self.n_head, grads=list(grads[:-1]))
        return loss.detach(), (enc, grads[-1])

    def _phase_b(self, hand):
        enc, g_enc = hand
        with ops.recording_wgrads(self._defer):
            torch.autograd.backward([enc], [g_enc])
        ops.set_zero_arena(None)
        self.flat.gather(self.n_head, None)

    def _phase_b_part(self, hand, s):
        """Part s of phase B (see _plan_buckets): from the gradient the previous part left at its cut down to this part's cut
        -> the hand-over to part s + 1."""
        li, lo, hi, _, _ = self.parts[s]
        src, g_src = hand
        last = li is None
        with ops.recording_wgrads(self._defer):
            if not last:
                cut = self.model._cuts[li]
                grads = torch.autograd.grad([src], self.flat.params[lo:hi] + [cut], grad_outputs=[g_src], allow_unused=True)
                hand = (cut, grads[-1])
                grads = list(grads[:-1])
            else:
                # (the bias tables' node hangs off every layer through the pack's token, not off the encoder input: name it)
                tok = getattr(getattr(self.model, "_bias_pack", None), "token", None)
                outs, gouts = [src], [g_src]
                if tok is not None and tok.requires_grad:
                    outs.append(tok)
                    gouts.append(torch.zeros_like(tok))
                torch.autograd.backward(outs, gouts)
                grads = None
        if last:
            ops.set_zero_arena(None)
        self.flat.gather(lo, hi, grads=grads)
        return hand

    def _warmup(self, i, check=False):
        """One eager pass of batch i on the capture stream (allocator, lazy initialisations) that does not count as a training
        step: the step counter (dropout stream, AdamW's t) is put back, so that a replayed sequence draws the masks an eager
        sequence draws, however many graphs were captured on the way.  `check` (add_batch): the trained-parameter set -- flat
        layout, sinks, optimizer -- was fixed by the batches given at construction; a batch that reaches a parameter outside it
        would leave that parameter silently untrained.  Looked for in THIS pass (no extra dry run: ADVICE r4).  The
        error is raised on the rank that sees it: ranks meet new shape buckets at different steps, so no collective may run here
        (it would pair with another rank's gradient exchange); under torch.distributed.run a rank that exits takes the job down."""
        batch = self.batches[i]
        known = {id(p) for p in self.flat.params}
        import warnings
        warn_always = torch.is_warn_always_enabled()
        torch.set_warn_always(True)                   # (torch raises this warning once per process otherwise)
        try:
            with warnings.catch_warnings(record=True) as seen:
                warnings.simplefilter("always")
                with self._on_stream():
                    saved = self.seed_dev.clone()
                    if check:
                        for p in self.model.parameters():
                            if id(p) not in known:
                                p.grad = None
                    self._fwd_bwd(batch)
                    self.seed_dev.copy_(saved)
        finally:
            torch.set_warn_always(warn_always)
        for w_ in seen:
            if "AccumulateGrad node's stream does not match" in str(w_.message):
                # An autograd graph of an EARLIER forward pass of this model is still alive (a loss tensor kept by the caller, a
                # traceback that holds one): its AccumulateGrad nodes are bound to the stream of that pass, this warm-up ran on
                # the trainer's capture stream, and the capture that follows would record a cross-stream wait on the legacy
                # stream -- hipStreamEndCapture then takes the process down (a core dump, seen in round 6 behind a failed test).
                raise RuntimeError("mobgt TrainStep: an autograd graph of an earlier forward pass of this model is still alive (a loss "
                                   "tensor or an exception traceback holding one?).  Its AccumulateGrad nodes belong to another stream and "
                                   "a hipGraph capture of the backward pass would abort the process.  Delete every reference to earlier "
                                   "losses / outputs of the model (del loss; gc.collect()) before TrainStep.prepare().")
            warnings.warn_explicit(w_.message, w_.category, w_.filename, w_.lineno)
        with self._on_stream():
            extra = [n for n, p in self.model.named_parameters() if id(p) not in known and p.grad is not None] if check else []
        self._join()
        if check and extra:
            raise RuntimeError(f"TrainStep.add_batch: this batch reaches parameters the trainer was not built for: {extra[:5]}")

    def _exchange(self, buf=None):
        """Sum of the flat gradient buffer (`buf`: the window's accumulator instead) over the ranks and the average, issued on the
        CURRENT stream (eager, or as nodes of the step graph being captured): through the bf16 exchange buffer when there is one
        (half the bytes on the wire; the widening pass applies 1 / world), else in place."""
        if buf is None:
            buf = self.flat.flat
        if self.comm_buf is not None:
            self.comm_buf.copy_(buf)
            dist.all_reduce(self.comm_buf, op=dist.ReduceOp.SUM)
            torch.mul(self.comm_buf, 1.0 / self.world, out=buf)
        elif self.world > 1 and buf is self.flat.flat:
            self.flat.all_reduce_mean()
        elif self.world > 1:
            dist.all_reduce(buf, op=dist.ReduceOp.SUM)
            buf.div_(self.world)
        else:                                  # (one forced rank: the collective itself, no division)
            dist.all_reduce(buf, op=dist.ReduceOp.SUM)

    # ---- captures: one routine per kind of entry (step_graphs.py), each returns the Entry it captured ----------------------
    def _capture_step(self, j, comm, warm=True):
        """("step", j, comm).  fused_opt: the whole step as ONE graph -- forward + backward [+ the gradient exchange on this stream:
        `comm`] + AdamW; host exchange: forward + backward; overlap: phase A, then phase B whole or in its parts."""
        batch = self.batches[j]
        if warm:
            self._warmup(j)
        g = torch.cuda.CUDAGraph()
        # private memory pool per graph: the graphs are replayed in data order, not capture order, and a shared
        # pool is only safe for capture-order replay (measured: NaNs on the second lap with a shared pool)
        if not self.overlap:
            with self._capturing(g):
                loss = self._fwd_bwd(batch, rows=j)
                if comm:
                    self._exchange()
                if self.fused_opt:
                    self._opt_step()
            return Entry((g,), loss)
        # several graphs over ONE autograd graph: phase B is captured right after phase A and replays its kernels on the
        # activations phase A's replay leaves at the same addresses (A's private pool; nothing else writes there)
        with self._capturing(g):
            loss, hand = self._phase_a(batch)
        gbs = []
        for s in range(max(1, len(self.parts))):
            gbs.append(torch.cuda.CUDAGraph())
            with self._capturing(gbs[-1]):
                hand = self._phase_b_part(hand, s) if self.parts else self._phase_b(hand)
        return Entry((g, *gbs), loss)

    def _capture_opt(self):
        g = torch.cuda.CUDAGraph()
        with self._capturing(g):
            self._opt_step()
        return Entry((g,), None)

    def prepare(self):
        """Capture every batch's step (or micro-step) and, in the forms that replay them, the optimizer / update graphs."""
        if not self.use_graph:
            return
        self.fused_opt = not self._accum and not self.overlap and (not self.ddp or self.one_graph)
        self._capture_all(first=True)
        self._prepared = True

    def _capture_all(self, first=False):
        """The eager capture loop of prepare() (`first`: with the one-off first calls) and recapture(): per batch a warm-up pass
        and ONE capture.  Single process, or the exchange captured (`one_graph`): the optimizer rides at the end of every batch's
        graph -- one graph launch per step instead of two (the boundary between two replayed graphs idles the device for
        ~8.7 us: `tools/prof_gaps.sh`); the other forms replay a stand-alone optimizer / update graph, captured behind the batches."""
        for j in range(len(self.batches)):
            self._warmup(j)
            if first and j == 0:
                self._first_calls()
            self._capture_batch(j)
        if self._accum:
            self.graphs.get(("update", self.one_graph), self._capture_update, self.one_graph)
        elif not self.fused_opt:
            self.graphs.get(("opt",), self._capture_opt)

    def _capture_batch(self, j):
        """The entry every step of batch j replays by default, behind that batch's warm-up pass."""
        if self._accum:
            return self.graphs.get(("micro", j), self._capture_micro, j, False)
        return self.graphs.get(("step", j, self.one_graph), self._capture_step, j, self.one_graph, False)

    def _first_calls(self):
        """One eager pass over the optimizer's / the update's launches and the collective on these buffers before ANY capture
        that holds them (first-launch initialisation must not happen inside a capture), made side-effect free: parameters,
        shadows, both Adam moments, the accumulator and the update counter are put back, so the first replayed update is AdamW's
        t = 1 on fresh moments, exactly like torch.optim.AdamW's first step -- on every rank alike."""
        with self._on_stream():
            with torch.no_grad():
                saved = self.flat_params.tensor.detach().clone()
                if self._accum:
                    if self.one_graph:
                        self._exchange(self._gsrc)
                    self._accumulate()
                    self._update_kernels()
                    if self.acc is not None:
                        self.acc.zero_()
                    self.upd_dev.zero_()
                else:
                    self._step_base = int(self.seed_dev.item()) - 1
                    self._opt_step()
                    if self.one_graph:
                        self._exchange()
                self.flat_params.tensor.copy_(saved)
                self.exp_avg.zero_()
                self.exp_avg_sq.zero_()
                self.flat.flat.zero_()
                self.sync_shadows()
            if not self._accum:
                # every later prologue (one per replayed step) advances the counter by one: t = counter - base = 1, 2, ...
                self._step_base = int(self.seed_dev.item())
        self._join()

    # ---- accumulation windows and global-norm clipping ----------------------------------------------------------
    # A micro-step is [prologue, forward, backward, accumulate]: ONE graph per batch whatever its position in the window (the
    # accumulator is zero at a window's start, so the first micro-step adds like every other).  The update -- [exchange],
    # [norm], finish, scaled AdamW -- is a small graph of its own, replayed after the window's last micro-step: one replay
    # boundary per window, and a flushed short window needs no second form of any batch's graph.
    def _accumulate(self):
        """Tail of a micro-step: acc += the micro-batch's gradient.  On a single rank with clipping the same launch leaves the
        per-block sums of squares of the new accumulator (after the window's last micro-step they are the update's); with an
        exchange in between, the norm pass of `_update_kernels` computes them from the exchanged bytes instead."""
        from . import _lib
        from .ops import _p, _stream
        part = self.partials if not self.ddp else None
        n = self.flat.flat.numel()
        if self.acc is not None:
            _lib.call("mobgt_grad_accumulate", _p(self.acc), _p(self.flat.flat), n, _p(part), _stream())
        elif part is not None:                       # (k = 1: nothing to add, the norm of the flat gradient buffer itself)
            _lib.call("mobgt_grad_accumulate", _p(self.flat.flat), None, n, _p(part), _stream())

    def _update_kernels(self):
        """[norm of the exchanged gradient,] finish (grad_norm, scale = coef / k, update counter + 1), AdamW on scale * acc (which
        leaves the accumulator zero)."""
        from . import _lib
        from .ops import _p, _stream
        n, g = self.flat.flat.numel(), self._gsrc
        if self.partials is not None and self.ddp:
            _lib.call("mobgt_grad_accumulate", _p(g), None, n, _p(self.partials), _stream())
        _lib.call("mobgt_grad_norm_finish", _p(self.partials), 0 if self.partials is None else self.partials.numel(),
                  1.0 / self.accumulate, self.clip_norm or 0.0, _p(self.grad_norm), _p(self.scale_dev),
                  _p(self.upd_dev), _stream())
        _lib.call("mobgt_adamw_flat_scaled", _p(self.flat_params.tensor), _p(g), _p(self.exp_avg), _p(self.exp_avg_sq),
                  _p(self.shadow_flat), n, _p(self.lr_dev), _p(self.sched_dev), _p(self.upd_dev), 0,
                  _p(self.scale_dev), 1 if self.acc is not None else 0, self.betas[0], self.betas[1],
                  self.eps, float(self.model.weight_decay), _stream())

    def _capture_micro(self, j, warm=True):
        """("micro", j)"""
        if warm:
            self._warmup(j)
        g = torch.cuda.CUDAGraph()
        with self._capturing(g):
            loss = self._fwd_bwd(self.batches[j], rows=j)
            self._accumulate()
        return Entry((g,), loss)

    def _capture_update(self, comm):
        """("update", comm): [the captured exchange,] norm, finish, AdamW.  Does not depend on a batch."""
        g = torch.cuda.CUDAGraph()
        with self._capturing(g):
            if comm:
                self._exchange(self._gsrc)
            self._update_kernels()
        return Entry((g,), None)

    def _update(self):
        """The optimizer update that ends a window (the host bookkeeping -- `self.window` -- has been done by the caller)."""
        comm = self.ddp and self.comm
        if comm:
            self.exchanges_done += 1
        captured = bool(comm and self.use_graph and self.one_graph)
        if comm and not captured:
            self._exchange(self._gsrc)                           # (issued by the host: gloo, MOBGT_DDP_HOST_EXCHANGE, eager)
        if self.use_graph:                                       # (the twin without the exchange: captured on first use)
            self.graphs.get(("update", captured), self._capture_update, captured).graphs[0].replay()
        else:
            self._update_kernels()
        self._set_lr()

    def _step_accum(self, i):
        j = i % len(self.batches)
        if self.use_graph:
            graphs, self._loss_ref = self.graphs.get(("micro", j), self._capture_micro, j, False)
            graphs[0].replay()
        else:
            self._loss_ref = self._fwd_bwd(self.batches[j])
            self._accumulate()
        if self.window.step(self.sched_state):
            self._update()
        return self.loss_out

    def flush(self):
        """End an incomplete accumulation window with an update now (its gradient is still `sum / accumulate`: Lightning divides
        every micro-loss by k whatever the window's length).  No-op on an empty window, and always without accumulation."""
        if self._accum and self.window.flush(self.sched_state):
            self._update()

    # ---- several steps per graph replay (round 6) -----------------------------------------------------------------------
    # Between two replayed step graphs the device idles (~60 us of a 0.595 ms S-FSQ step in round 5: 0.534 ms of graph wall
    # time): the replay that follows cannot start before the runtime has retired the one in front of it.  Nothing of a step
    # lives on the host -- the dropout stream, AdamW's t and the learning-rate schedule are device counters the step's own
    # kernels advance -- so k consecutive steps on pre-collated batches can be ONE graph: k x (forward, backward [, exchange],
    # AdamW), one replay, no host round trip between them.  The graph holds k steps' activations (S-FSQ: ~30 MB per step).
    def _capture_group(self, batches, comm):
        """("group", batches, comm): the steps of those batches, one behind the other, as ONE graph."""
        if not (self._prepared and self.fused_opt and self.sched_dev is not None):
            raise RuntimeError("TrainStep.step_group needs prepare(), hipGraphs, the one-graph step form and the device-side schedule")
        g = torch.cuda.CUDAGraph()
        with self._capturing(g):
            for j in batches:
                loss = self._fwd_bwd(self.batches[j])
                if comm:
                    self._exchange()
                self._opt_step()
        return Entry((g,), loss)

    def step_group(self, i, k):
        """Steps i, i + 1, ... i + k - 1 (batches taken cyclically from the pre-collated pool, like k calls of `step`) as ONE
        graph replay; -> the last step's loss tensor.  Same arithmetic, same counters, same order as k single steps."""
        if self._accum:
            raise NotImplementedError("TrainStep.step_group is not built for accumulate > 1 / clip_norm: call step() per micro-step")
        comm = self.ddp and self.comm
        key = group_key(i, int(k), len(self.batches), comm)
        graphs, self._loss_ref = self.graphs.get(key, self._capture_group, key[1], comm)
        graphs[0].replay()
        self.window.updated(self.sched_state, int(k))
        self._set_lr()
        return self.loss_out

    # ---- peer waits that gave up (csrc/chain.hip WS_FAULT, head.hip, smallgcn.hip): detection and recovery ---------------
    def recapture(self):
        """Capture every step graph again (after forms "safe_forms" changed which kernels a step launches).  Parameters,
        optimizer state and the step counter are left as they are."""
        if not (self.use_graph and self._prepared):
            return
        self.graphs.clear()          # (what is captured on first use -- the twins without exchange, groups -- comes back that way)
        self._capture_all()

    def check_faults(self, on_fault="raise"):
        """Workgroups that gave up waiting for their cluster partners / at a grid barrier since the last check ({} = none;
        synchronises the device).  The steps since then may have trained on garbage gradients: "raise" -> RuntimeError."""
        f = ops.peer_wait_faults(reset=True)
        if self.ddp:                                    # every rank must take the same decision
            t = torch.tensor([float(sum(f.values()))], device=self.device)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            if float(t.item()) > 0 and not f:
                f = {"other_rank": int(t.item())}
        if f and on_fault == "raise":
            raise RuntimeError(f"mobgt: workgroups gave up waiting for their peers {f} -- the affected steps' gradients are invalid "
                               "(co-residency lost to another stream's kernels?); use TrainStep.guarded_step or MOBGT_SAFE_FORMS=1")
        return f

    def guarded_step(self, i):
        """step(i) with the promise that no peer-wait fault goes unnoticed: state snapshot -> step -> device sync + fault check;
        on a fault the snapshot is restored, every launch switches to its form WITHOUT cross-workgroup waits
        (forms "safe_forms": one workgroup per row block, the head as three launches, the GCN layer by layer), the graphs are
        captured again and the step is re-run with the same dropout counter.  Costs three buffer copies and a host
        synchronisation per step: meant for runs that share the device with other streams' persistent kernels."""
        with torch.no_grad():
            snap = (self.flat_params.tensor.detach().clone(), self.exp_avg.clone(), self.exp_avg_sq.clone(), self.seed_dev.clone())
            # (accumulation: the open window -- accumulator, its sums of squares, the update counter -- so that the re-run
            #  micro-step is added once and counted once)
            snap_acc = [(t, t.clone()) for t in (self.acc, self.partials, self.upd_dev, self.scale_dev, self.grad_norm)
                        if t is not None]
        sched, win = dict(self.sched_state), self.window.state()
        loss = self.step(i)
        if not self.check_faults(on_fault="return"):
            return loss
        with torch.no_grad():
            self.flat_params.tensor.copy_(snap[0])
            self.exp_avg.copy_(snap[1])
            self.exp_avg_sq.copy_(snap[2])
            self.seed_dev.copy_(snap[3])
            for t, saved in snap_acc:
                t.copy_(saved)
            self.sync_shadows()
        self.sched_state = sched
        self.window.restore(win)
        self._set_lr()
        forms.set("safe_forms", True)
        ops.set_peer_wait_limit(0, 0)
        self.recapture()
        self.faults_recovered += 1
        loss = self.step(i)
        self.check_faults(on_fault="raise")
        return loss

    def add_batch(self, batch):
        """Register one more static batch (a new shape bucket of EpochLoop) and, in graph mode after `prepare()`, capture
        its step graph now (the capture's eager warm-up pass leaves the step counter and the parameters untouched)."""
        self.batches.append(batch)
        i = len(self.batches) - 1
        try:
            self._warmup(i, check=True)                 # (the capture's warm-up pass and the parameter-set check in one)
        except Exception:
            self.batches.pop()
            raise
        if self.use_graph and self._prepared:
            self._capture_batch(i)                      # (nothing else in the cache depends on the number of batches)
        return i

    def step(self, i):
        """One optimizer step on pre-collated batch i (model_fqandtoyo.py:1434-1478 + optimizer + scheduler).  With
        `accumulate` / `clip_norm`: one micro-step; the window's last one also updates.  -> this batch's loss."""
        if self._accum:
            return self._step_accum(i)
        j = i % len(self.batches)
        if self.use_graph:
            # (comm: the exchange as a node of the graph; bench.py runs the same step without it, captured on first use)
            comm = self.one_graph and self.comm
            graphs, self._loss_ref = self.graphs.get(("step", j, comm), self._capture_step, j, comm, False)
            if self.overlap:
                self._replay_overlap(graphs)
            else:
                graphs[0].replay()
        else:
            self._loss_ref = self._fwd_bwd(self.batches[j])
        if not self.fused_opt:
            if self.ddp and self.comm and not self.overlap:
                self._exchange()                                    # (issued by the host: gloo, MOBGT_DDP_HOST_EXCHANGE, eager)
            if self.use_graph:
                self.graphs.get(("opt",), self._capture_opt).graphs[0].replay()
            else:
                self._opt_step()
        self.window.updated(self.sched_state)
        self._set_lr()
        return self.loss_out

    def _replay_overlap(self, graphs):
        """Phase A, then the parts of phase B: every element range of the flat buffer is all-reduced (RCCL's stream) as soon as the
        replay that completes it has been enqueued, i.e. beside the replay of the next part."""
        na, cb = self.n_head_elems, self.comm_buf
        comm = self.ddp and self.comm
        bounds = [(0, na)] + ([(e0, e1) for _, _, _, e0, e1 in self.parts] if self.parts else [(na, self.flat.flat.numel())])
        works = []
        for g, (e0, e1) in zip(graphs, bounds):
            g.replay()
            if comm and e1 > e0:
                if cb is not None:
                    cb[e0:e1].copy_(self.flat.flat[e0:e1])
                works.append(dist.all_reduce((cb if cb is not None else self.flat.flat)[e0:e1], op=dist.ReduceOp.SUM, async_op=True))
        if comm:
            for w in works:
                w.wait()
            if cb is not None:
                torch.mul(cb, 1.0 / self.world, out=self.flat.flat)          # widen + average in one pass
            else:
                self.flat.flat.div_(self.world)


class _StagedBatches:
    """Fresh batches on the device data path, shared by EpochLoop and EvalLoop: shape buckets, pinned staging, the device collate
    on the copy stream, the host-side index checks, the hand-over of a staged batch to its bucket's static buffer and the
    one-batch-ahead pipeline."""

    def __init__(self, model, collator, dataset, batch_size, buckets, rank, world, side_collate):
        from .data import BUCKETS
        self.model, self.collator, self.dataset = model, collator, dataset
        self.batch_size = int(batch_size)
        self.buckets = tuple(buckets or BUCKETS)
        ddp = dist.is_available() and dist.is_initialized()
        self.rank = rank if rank is not None else (dist.get_rank() if ddp else 0)
        self.world = world if world is not None else (dist.get_world_size() if ddp else 1)
        self.device = next(model.parameters()).device
        self.copy_stream = torch.cuda.Stream(device=self.device)
        self.slots, self.limits = {}, None
        self.side_collate = bool(side_collate)

    # ---- buckets --------------------------------------------------------------------------------------------------------
    def _slot(self, G, N):
        from .data import BatchLayout, RawLayout
        key = (G, N)
        s = self.slots.get(key)
        if s is None:
            # `side`: the device collate of the NEXT batch runs on the copy stream, beside the current step (whose kernels
            # leave most of the chip idle); the step graph then reads a collated static batch.  Collators that need torch
            # ops (coords= + bin_edges=, S-BIG's default) keep the collate inside the step graph (batch_fn = finish); a
            # collator built with pair_bins= collates coordinate-bin universes here like any other.
            side = self.side_collate and self.collator.can_finish_into()
            lay = BatchLayout(G, N, self.collator.D) if side else RawLayout(G, N)
            buf = torch.zeros(lay.nbytes, dtype=torch.uint8, device=self.device)
            views = lay.views_torch(buf)
            s = dict(layout=lay, buf=buf, views=views, index=None, stages=[], turn=0, side=side,
                     batch=self.collator.batch_from_views(views) if side else views,
                     copy_bytes=lay.copy_bytes if side else lay.nbytes)
            for _ in range(2):
                s["stages"].append(self.collator.new_stage(lay, side))      # (pinned host buffer + device staging buffer)
            # (the zero fills above are queued on the current stream, behind whatever it still runs; the copy stream writes the
            #  staging buffers next and must not overtake them -- a fill landing after the copy left a batch of zeros)
            self.copy_stream.wait_stream(torch.cuda.current_stream())
            self.slots[key] = s
        return s

    def _check_host(self, h):
        """What nn.Embedding would raise on in the reference (IndexError), checked on the host arrays of a fresh batch --
        the captured step cannot look at values (model.validate_batch does this for pre-collated batches)."""
        m = self.model
        if self.limits is None:
            # (the model says which fields it indexes tables with -- model.index_limits(); a model without the hook is not checked)
            self.limits = m.index_limits() if hasattr(m, "index_limits") else {}
        bad = self.collator.limit_violation(h, self.limits)      # (the collator knows its host arrays: dicts or sessions)
        if bad:
            raise IndexError(f"batch.{bad[0]} has index {bad[1]}, out of range for a table of {bad[2]} rows")

    def _stage(self, ids):
        """Host half of a step's input: raw samples (trajectory dicts, or sessions with a SessionCollator) -> the bucket's
        pinned buffer -> async copy to a device staging buffer on the copy stream.  Returns (slot, stage)."""
        from .data import bucket_nodes
        trajs = [self.dataset[i] for i in ids]
        trajs = [t for t in trajs if self.collator.keeps(t)]
        G = len(trajs)
        if G == 0:
            return None                                # (every trajectory filtered out: the reference's collator skips such a batch too, collator.py:313)
        N = bucket_nodes(max(self.collator.nodes_of(t) for t in trajs), self.buckets)
        slot = self._slot(G, N)
        st = slot["stages"][slot["turn"]]
        slot["turn"] ^= 1
        if st["free"] is not None:
            st["free"].synchronize()                   # its previous device-to-device copy has been executed
        self._check_host(self.collator.stage_host(st, trajs, ids[:G] if len(ids) == G else 0, N))
        st["used"] = True
        with torch.cuda.stream(self.copy_stream):
            self.collator.upload(st)                   # (H2D; from sessions: + the kernel that builds the raw fields)
            if slot["side"]:
                st["work"] = self.collator.finish_into(st["dev_views"], st["work"])
            st["ready"].record(self.copy_stream)
        return slot, st

    def _hand_over(self, slot, st):
        """On the current stream (where the graphs replay): behind the staged batch's copy-stream work, ONE device-to-device copy
        of its [raw | derived] bytes into the bucket's static buffer; then the stage may be filled again.  -> that stream."""
        cur = torch.cuda.current_stream()
        cur.wait_event(st["ready"])
        n = slot["copy_bytes"]
        slot["buf"][:n].copy_(st["dev"][:n], non_blocking=True)
        if st["free"] is None:
            st["free"] = torch.cuda.Event()
        st["free"].record(cur)
        return cur

    def _collated(self, b):
        """Inside a step or a forward: raw views -> the collate (in-graph form); a collated static batch passes through."""
        return self.collator.finish(b) if isinstance(b, dict) else b

    def _pipeline(self, batches, launch=None):
        """One batch ahead, in this host order for every j: launch(j, slot, stage) of batch j (asynchronous: the GPU works on
        it ...), unless staging returned None for it (an empty batch: skipped, as the reference's collator does); stage batch
        j + 1 (... while the host packs the next one); only then yield (j, ids, staged, launch's result) to the caller, whose
        code may synchronise.  `launch` defaults to the loop's own _launch(slot, stage)."""
        if launch is None:
            launch = lambda j, slot, st: self._launch(slot, st)
        nxt = self._stage(batches[0]) if batches else None
        for j, ids in enumerate(batches):
            cur = nxt
            res = launch(j, *cur) if cur is not None else None
            nxt = self._stage(batches[j + 1]) if j + 1 < len(batches) else None
            yield j, ids, cur, res


class EpochLoop(_StagedBatches):
    """The fit loop over the training set (Lightning's `trainer.fit` on `train_dataloader`: entry.py:141-161,
    data.py:282-295), one process per GPU: a NEW batch every step, collated on the device.

    * sampler: `data.shard_indices` = torch's DistributedSampler (shuffle by seed + epoch, wrap-around padding, stride by
      rank); consecutive runs of `batch_size` indices form the batches (`drop_last=False`, as the reference's DataLoader);
    * shapes: a batch's padded node count is rounded up to a bucket (`data.BUCKETS`); every (G, bucket) owns ONE static
      collated batch on the device, two staging buffers and ONE step graph = forward + loss + backward + AdamW, captured
      the first time the bucket occurs;
    * a step on the host: pack the NEXT batch's raw trajectories into a pinned staging buffer and, on the copy stream, start
      its host-to-device copy and its device collate (`DeviceCollator.finish_into`: SPD / edge paths / degrees / distance
      bins) while the GPU runs the current step; then -- on the compute stream -- one device-to-device copy of the staged
      raw + derived bytes into the bucket's static batch and one graph replay.  Collators whose finish needs torch ops
      (coordinate bins by coords= + bin_edges=; pair_bins= needs none) keep the collate inside the step graph
      (`batch_fn = finish`).
    """

    def __init__(self, model, collator, dataset, batch_size=16, seed=1, use_graph=True, overlap=True, buckets=None, rank=None,
                 world=None, shuffle=True, autocast_dtype=None, side_collate=True, balance=None, balance_window=32,
                 accumulate=1, clip_norm=None):
        """`accumulate`, `clip_norm`: passed to `TrainStep` (Lightning's `accumulate_grad_batches` / `gradient_clip_val`); every
        batch is then a micro-step and `run_epoch` flushes the window after the epoch's last batch (an epoch's last batch
        always steps).  `balance`: deal every step's batches by length over the ranks (`data.balanced_batches`: neighbouring shape buckets on
        all ranks in every synchronous step, the epoch's sample set still DistributedSampler's).  Default: on when there is more
        than one rank; with one rank the order is the reference's (DistributedSampler order, consecutive batches).
        `balance_window`: the length sort runs inside windows of that many steps of the permuted epoch (default 32: a
        mega-batch of 32 x world x batch_size i.i.d. samples -- batches stay mixed over the epoch and its long graphs are spread
        over the windows; DEVIATION from the reference's i.i.d. batches, bounded by the window; None = sort the whole epoch, the
        tightest balance; balance=False = the reference's sampler order exactly)."""
        super().__init__(model, collator, dataset, batch_size, buckets, rank, world, side_collate)
        self.seed, self.shuffle = int(seed), shuffle
        self.balance = (self.world > 1) if balance is None else bool(balance)
        self.balance_window = balance_window
        self._lengths = None
        self.ts = None
        self._ts_args = dict(autocast_dtype=autocast_dtype, use_graph=use_graph, seed=seed, overlap=overlap)
        check_accum_args(accumulate, clip_norm)          # (fail at construction, not at the first batch)
        if accumulate != 1 or clip_norm is not None:
            self._ts_args.update(accumulate=accumulate, clip_norm=clip_norm)
        self.steps_done = 0
        # (round 4 measured and round 5 removed: one step graph per STAGING buffer, i.e. no device-to-device copy between two
        #  replays -- 0.734 against 0.700 ms per step on the S-FSQ pool: two graphs per bucket alternate between two sets of
        #  activation buffers, and the copy was not what the loop waited for)

    # ---- data order -----------------------------------------------------------------------------------------------------
    def batches_of_epoch(self, epoch):
        from .data import DeviceCollator, balanced_batches, shard_indices
        if self.balance:
            if self._lengths is None:
                # (the collator knows its dataset's form; a loop set up for its order alone has none: trajectory dicts)
                self._lengths = (getattr(self, "collator", None) or DeviceCollator).lengths_of(self.dataset)
            steps = balanced_batches(self._lengths, self.world, self.batch_size, epoch=epoch, seed=self.seed, shuffle=self.shuffle,
                                     buckets=self.buckets, window=self.balance_window)
            return [s[self.rank] for s in steps]
        idx = shard_indices(len(self.dataset), self.rank, self.world, epoch=epoch, seed=self.seed, shuffle=self.shuffle)
        B = self.batch_size
        return [idx[i:i + B] for i in range(0, len(idx), B)]

    def _ensure_trainer(self, slot):
        """The first batch builds the TrainStep (dry run for the trained-parameter set, flat buffers, optimizer graph)."""
        if self.ts is None:
            self.ts = TrainStep(self.model, [slot["batch"]], batch_fn=self._collated, **self._ts_args)
            self.ts.prepare()
            slot["index"] = 0
        elif slot["index"] is None:
            slot["index"] = self.ts.add_batch(slot["batch"])

    def _launch(self, slot, st):
        self._hand_over(slot, st)
        if slot["index"] is None or self.ts is None:
            self._ensure_trainer(slot)                   # (dry run / capture on the data that is now in the static buffer)
        return self.ts.step(slot["index"])

    def run_epoch(self, epoch=0, max_steps=None, on_step=None):
        """One pass over this rank's shard.  Returns dict(steps, graphs, sample_ids); `on_step(step, loss_tensor)` is called
        after each launch (reading the loss there synchronises -- do it sparingly)."""
        batches = self.batches_of_epoch(epoch)
        if max_steps is not None:
            batches = batches[:max_steps]
        seen = []
        if not batches:
            return dict(steps=0, graphs=len(self.slots), sample_ids=seen)
        steps = 0
        for _, ids, staged, loss in self._pipeline(batches):
            seen.extend(ids)
            if staged is None:
                continue
            steps += 1
            self.steps_done += 1
            if on_step is not None:
                on_step(self.steps_done, loss)
        # peer waits that gave up during the epoch (the kernels count and carry on, csrc/chain.hip WS_FAULT): raise here, once
        # per epoch, rather than train on silently (one device synchronisation; every rank takes the same decision)
        if self.ts is not None:
            self.ts.flush()                              # (accumulation: the epoch's last window updates, however short)
            self.ts.check_faults(on_fault="raise")
        return dict(steps=steps, graphs=len(self.slots), sample_ids=seen)


class _FrozenModelLoop(_StagedBatches):
    """What EvalLoop and PredictLoop share on top of the staged batches: the eval loader's order, the model held in eval mode
    with its weights refreshed once and frozen while a run lasts, and per (G, bucket, forms.on("safe_forms")) ONE captured graph
    of the loop's step -- `_step(slot, warm)`, which each loop supplies -- warmed once on the capture stream and then replayed.
    `use_graph=False` runs the step eagerly, and so do buckets whose collate needs torch ops."""

    def __init__(self, model, collator, dataset, batch_size, rank, world, use_graph, buckets, side_collate):
        super().__init__(model, collator, dataset, batch_size, buckets, rank, world, side_collate)
        self.stream = torch.cuda.Stream(device=self.device) if use_graph else None     # warm-ups and captures
        self.use_graph = bool(use_graph)
        self.graphs, self._graph_ptrs = {}, None
        self.captures = 0                                   # graphs captured so far (a replayed run captures none)

    near = property(lambda self: self.restriction.near)             # (the loop's restriction is one object; these two parts of it
    allow = property(lambda self: self.restriction.allow)           #  stay readable on the loop)

    def batches(self, max_batches=None):
        from .data import shard_indices
        idx = shard_indices(len(self.dataset), self.rank, self.world, shuffle=False)
        B = self.batch_size
        return [idx[i:i + B] for i in range(0, len(idx), B)][:max_batches]

    def _step(self, slot, warm):
        """The loop's launches on the bucket's static batch; warm: the pass before a capture, whose results count nowhere."""
        raise NotImplementedError

    def _launch(self, slot, st):
        cur = self._hand_over(slot, st)
        if not self.use_graph or not slot["side"]:
            # Buckets whose collate needs torch ops (coords= + bin_edges=: S-BIG's default collator) run eagerly.  Captured with the collate inside, the
            # replay took 130 ms per 16 x 784 batch against 13 ms eager: inside the replayed graph the SPD kernel's split form
            # (workgroups that wait for each other, csrc/spd.hip) gave up on every call and its one-workgroup-per-graph redo
            # pass ran (fw_kernel: 75 ms per call, rocprofv3).  Why it gives up only there is not known.
            self._step(slot, warm=False)
            return
        key = (slot["layout"].G, slot["layout"].N, forms.on("safe_forms"))
        g = self.graphs.get(key)
        if g is None:
            self.stream.wait_stream(cur)
            with torch.cuda.stream(self.stream):
                self._step(slot, warm=True)                                          # allocator, lazy initialisations
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=self.stream):
                self._step(slot, warm=False)
            cur.wait_stream(self.stream)
            self.graphs[key] = g
            self.captures += 1
        g.replay()

    def _weights_ptrs(self):
        """Addresses a captured eval forward reads besides its batch: parameters, bf16 shadows, MFMA packs, the dropout seed.  A
        change (a trainer built after the capture re-homes the shadows) drops the graphs."""
        ptrs = [p.data_ptr() for p in self.model.parameters()]
        for layer in getattr(self.model, "layers", []):
            for name in ("_shadows", "_packed"):
                t = getattr(layer, name, None)
                ptrs += [x.data_ptr() for x in t] if t is not None else [0]
        ptrs += [m.seed_dev.data_ptr() for m in self.model.modules() if getattr(m, "seed_dev", None) is not None]
        return tuple(ptrs)

    def _refresh_weights(self):
        """bf16 shadows and MFMA packs from the current fp32 weights, once, outside any graph (the captured forwards then skip
        the copy: layer._weights_frozen)."""
        from .model import refresh_shadows
        layers = list(getattr(self.model, "layers", []))
        for layer in layers:
            if not getattr(layer, "_shadow_external", False):
                layer._shadow_ver = None                    # (unconditional copy: see model._may_skip_shadow_copy)
            layer._packed_ver = None
        refresh_shadows(layers)
        for layer in layers:                                # (a pack is good for the forward that follows a refresh only)
            layer._packed_fresh = layer._packed_t_fresh = False

    @contextlib.contextmanager
    def _evaluating(self):
        """Eval mode under no_grad with the weights refreshed and frozen for the captured forwards; on the way out the model's
        mode, the layers' flags and the forward state the trainer's next step reads are put back, and parked work left behind
        is refused."""
        model = self.model
        layers = list(getattr(model, "layers", []))
        was_training = model.training
        frozen = [getattr(l, "_weights_frozen", False) for l in layers]
        saved = {k: model.__dict__.get(k) for k in ("_enc_out", "_bias_pack", "_cuts")}
        model.eval()
        try:
            with torch.no_grad(), STEP.keeping_carried():
                self._refresh_weights()
                for l in layers:
                    l._weights_frozen = True
                ptrs = self._weights_ptrs()
                if ptrs != self._graph_ptrs:
                    self.graphs.clear()
                    self._graph_ptrs = ptrs
                yield
        finally:
            for l, f in zip(layers, frozen):
                l._weights_frozen = f
            for k, v in saved.items():
                setattr(model, k, v)
            model.train(was_training)
        left = ops.step_state_leftovers()
        if left:
            raise RuntimeError(f"{type(self).__name__}: the evaluation left parked work behind {left}")


class EvalLoop(_FrozenModelLoop):
    """The validation / test loop (Lightning's `trainer.validate` / `trainer.test` over the reference's eval DataLoader,
    entry.py:120-161, with test_epoch_end's bookkeeping, model_fqandtoyo.py:1484-1597) on the device data path of EpochLoop.

    * order: the reference's eval loader -- no shuffle, consecutive runs of `batch_size`, drop_last=False; with `world` > 1 the
      non-shuffling DistributedSampler (data.shard_indices, wrap-around duplicates included).  Batches are never regrouped by
      length: which rows share a batch decides where get_acc's stop at the first target 0 applies;
    * shapes and staging: EpochLoop's buckets (one static batch per (G, bucket)), pinned buffers, device collate on the copy
      stream, host index checks; trajectories over `collator.max_node` are dropped;
    * per (G, bucket, forms.on("safe_forms")) ONE captured graph = eval forward + the fused classifier-ranking launches
      (Graphormer.metric_step) adding into ONE f64 accumulator; `use_graph=False` runs the same launches eagerly, and so do
      collators whose finish needs torch ops (coordinate bins by coords= + bin_edges=, S-BIG's default: see _launch; a
      collator built with pair_bins= is captured like a bin-table one);
    * `run()` reads the accumulator once (after one all-reduce of all its doubles when world > 1: every rank's samples pooled).
    The weights are read as they are when `run()` starts (bf16 shadows and MFMA packs re-derived there, outside any graph), so an
    evaluation between training epochs sees the current model; it leaves no state behind that the trainer's next step reads.

    Restricted and split evaluation (Graphormer.metric_step's restricted form, ops.rank_metrics_masked) measures the lists
    PredictLoop returns with the same restriction, kept for the loop's lifetime: exclude_visited ranks each target among the
    POIs its trajectory has not visited, candidates (POI ids in y's label space, packed once here) among those only.
    split_revisits also reports the rows whose target is a new POI and those whose target is a revisit.  run() then returns
    metrics.finalize_restricted's dict: today's keys, "n", "reachable" (targets that can be listed at all) and, with the split,
    "new" / "revisit" dicts of the same keys.  The defaults run today's launches and return today's dict.

    within_km=r ranks each target among the POIs within r km of the row's anchor (ops.near_words inside the captured graph, then
    the per-row form of ops.rank_metrics_masked); it combines with the other restrictions.  coords: [P + 1, 2] lat / lon in
    degrees, row 0 the pad POI (default: the collator's coords; neither: ValueError).  near="last": the anchor is the
    trajectory's last node, node_name[-1] -- the last history check-in for a SessionDataset and for dicts made from sessions
    (nodes ordered by last visit); a hand-made dict stores distinct POIs in the order given, where the last node need not be the
    last check-in; near="any": within r of any POI of the trajectory, which does not depend on order.  A target outside its
    row's radius is unreachable and counts in n only.

    dataset / collator: trajectory dicts with a DeviceCollator, or a data.SessionDataset with a data.SessionCollator -- the
    loops reach the input form through the collator only (nodes_of, keeps, lengths_of, new_stage, stage_host, limit_violation,
    upload), and the collate through can_finish_into, finish_into and batch_from_views on the copy stream, or finish inside
    the step.

    prior: a prior.MarkovPrior on the loop's device (mb.prior(...) of a data.MarkovBaseline fitted on the TRAIN sessions).  Its
    weighted log-counts are added to the scores inside the captured graph, one launch between the classifier and the ranking
    (the rule: prior.py's docstring), and exclude_visited, candidates, within_km and split_revisits act on the blended scores.
    The anchor of a row is its trajectory's last node, with near="last"'s caveat: the last history check-in for sessions and
    graphs made from them, not necessarily for a hand-made dict.  The graphs read the prior's weights from device memory, so
    prior.set_weights between two runs needs no new capture.  run() zeroes the prior's status word when it starts and reads it
    with the accumulator; a status that is not zero (tables that fit did not make) is a ValueError.

    prior may also be a geoprior.DistancePrior (mb.distance_prior(pair_bins): a fitted distance-decay table, the rule in
    geoprior.py's docstring, the same anchor), a ctxprior.ContextPrior (data.ContextPrior.fit(ds, train): the category-transition
    and time-of-day tables, the rule in ctxprior.py's docstring, the same anchor, its category and its slot read from batch.cat
    and batch.time), a visitprior.VisitPrior (data.VisitPrior.fit(ds, train): how often and how recently batch.user has been at
    each POI, the rule in visitprior.py's docstring, no anchor) or a prior.Stack of several priors, blended in the order given,
    one launch each.

    prior_weights: a sweep, [L, prior.n_weights] rows of prior.WEIGHTS -- (user, transition, popularity) for a MarkovPrior,
    (distance,) for a DistancePrior, (category, time) for a ContextPrior, (visits, recency) for a VisitPrior, the members' names
    concatenated for a Stack --
    1 <= L <= 16.  Every batch is encoded ONCE;
    for each row the scores are blended out of place into one scratch [batch_size, V] with that row's weights and ranked into
    an accumulator of the row's own; run() returns the list of the L dicts, each what a loop with those weights returns.  The
    prior's own weights are not used and not changed (prior.tune picks the best row and sets it)."""

    def __init__(self, model, collator, dataset, batch_size=16, rank=None, world=None, use_graph=True, buckets=None,
                 side_collate=True, exclude_visited=False, candidates=None, split_revisits=False, within_km=None, coords=None,
                 near="last", prior=None, prior_weights=None):
        from . import metrics
        if not hasattr(model, "metric_step"):
            raise TypeError("EvalLoop: the model has no metric_step (the fq model, model_fqandtoyo.Graphormer)")
        radius = Restriction.radius(collator, within_km, coords, near)
        sweep = None
        if prior_weights is not None:
            from .prior import sweep_weights
            if prior is None:
                raise ValueError("EvalLoop: prior_weights without prior= (the sweep blends a prior: prior.MarkovPrior, geoprior.DistancePrior, prior.Stack)")
            sweep = sweep_weights(prior_weights, "EvalLoop: prior_weights", prior.WEIGHTS)
        super().__init__(model, collator, dataset, batch_size, rank, world, use_graph, buckets, side_collate)
        V = model.out_proj.out_features
        self.prior = prior
        if prior is not None:
            prior.for_loop(model, self.device, self.batch_size, "EvalLoop")
        r = self.restriction = Restriction.on_device(model.label_offset, V, self.batch_size, self.device, exclude_visited,
                                                     candidates, split_revisits, radius)
        if r.active:
            new_acc = lambda: metrics.new_restricted_accumulator(self.device, r.split_revisits)
            nbytes = ops.rank_metrics_masked_work_bytes(self.batch_size, V)
        else:
            new_acc = lambda: metrics.new_accumulator(self.device)
            nbytes = ops.rank_metrics_work_bytes(self.batch_size, V)
        self.acc, self._scratch = new_acc(), new_acc()      # (warm-up passes count in the scratch one, that is nowhere)
        self.work = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self.sweep = None
        if sweep is not None:                               # [L, n_weights] weights, L accumulators, one [rows, V] buffer for the blends
            self.sweep = (torch.from_numpy(sweep).to(self.device), [new_acc() for _ in sweep],
                          torch.empty(self.batch_size, V, dtype=torch.float32, device=self.device))

    restricted = property(lambda self: self.restriction.active)

    def _step(self, slot, warm):
        if self.sweep is not None:
            return self._sweep_step(self._collated(slot["batch"]), warm)
        self.model.metric_step(self._collated(slot["batch"]), self._scratch if warm else self.acc, work=self.work,
                               restriction=self.restriction, prior=self.prior)

    def _sweep_step(self, batch, warm):
        """metric_step with the encoder run once: the scores blended with every weights row in turn, each blend ranked by
        metric_step's own ranking call into that row's accumulator."""
        model, r = self.model, self.restriction
        W, accs, blended = self.sweep
        with torch.no_grad():
            scores = model.poi_scores(model.encode(batch))
            out = blended[:scores.shape[0]]
            hist = r.hist(batch)
            allow = r.allow_for(hist) if r.active else None  # (the rows' words do not depend on the scores: built once)
            for l in range(W.shape[0]):
                acc = self._scratch if warm else accs[l]
                self.prior.blend(scores, batch, r.label_offset, out=out, weights=W[l])
                if r.active:
                    ops.rank_metrics_masked(out, batch.y, acc, target_offset=-r.label_offset, allow=allow, hist=hist,
                                            hist_offset=r.label_offset, exclude_hist=r.exclude_visited, split=r.split_revisits,
                                            work=self.work)
                else:
                    ops.rank_metrics(out, batch.y, acc, target_offset=-r.label_offset, work=self.work)

    def run(self, max_batches=None):
        """One pass over this rank's part of the split -> dict of metrics.evaluate_outputs' keys + "n" (samples counted)."""
        from . import metrics
        accs = [self.acc] if self.sweep is None else self.sweep[1]
        with self._evaluating():
            for acc in accs:
                acc.zero_()
            if self.prior is not None:
                self.prior.reset_status()
            for _ in self._pipeline(self.batches(max_batches)):
                pass
            if self.world > 1 and dist.is_available() and dist.is_initialized():
                for acc in accs:
                    if dist.get_backend() == "gloo":
                        host = acc.cpu()
                        dist.all_reduce(host)
                        acc.copy_(host)
                    else:
                        dist.all_reduce(acc)
            if self.prior is not None:
                self.prior.check("EvalLoop")                # (read with the accumulator: the pass is over)
            finalize = metrics.finalize_restricted if self.restriction.active else metrics.finalize
            if self.sweep is not None:
                return [finalize(acc) for acc in accs]
            return finalize(self.acc)                       # the one host read


class PredictLoop(_FrozenModelLoop):
    """Top-k next-POI recommendations over a whole split (Graphormer.recommend_step) on EvalLoop's device data path: the eval
    loader's order and sharding, EpochLoop's buckets and staging, one captured graph per (G, bucket, forms.on("safe_forms")) -- eager
    for collators whose finish needs torch ops (coords= + bin_edges=, S-BIG's default) -- and the weights as they are when run() starts.

    A graph writes its batch's [G, k] ids / vals into buffers of its own (fixed pointers); a device-to-device copy on the same
    stream, outside the graph, then moves them to the batch's rows of the result.  Trajectories over collator.max_node, which
    the evaluation drops, keep ids -1 and vals -inf.  Gathering the ranks' shards is left to the caller.

    A loop keeps one restriction for its lifetime: exclude_visited leaves out each trajectory's own POIs (next *new* POI lists);
    candidates, a 1-D tensor of POI ids in y's label space, limits every list to them (packed once, here, into words the graphs
    read at a fixed address).  Rows with fewer than k candidates end in ids -1 / vals -inf, as dropped trajectories do.

    within_km=r limits each list to the POIs within r km of the row's anchor, with coords and near as in EvalLoop (near="last":
    the trajectory's last node, node_name[-1]: the last history check-in when the graphs come from sessions; near="any":
    within r of any POI of the trajectory).  The rows' candidate words are built inside the captured graph (ops.near_words) from
    positions packed once here, and combine with exclude_visited and candidates.

    prior: any prior (a prior.Prior) or a prior.Stack on the loop's device, blended into the scores inside the captured graph before the lists are
    taken, as in EvalLoop (vals are the blended scores; the anchor caveat of near="last" holds).  run() zeroes the prior's status
    word when it starts and reads it after the pass -- the loop's one host read, made only with a prior; not zero: ValueError."""

    def __init__(self, model, collator, dataset, k=20, batch_size=16, rank=None, world=None, use_graph=True, buckets=None,
                 side_collate=True, exclude_visited=False, candidates=None, within_km=None, coords=None, near="last", prior=None):
        if not hasattr(model, "recommend_step"):
            raise TypeError("PredictLoop: the model has no recommend_step (the fq model, model_fqandtoyo.Graphormer)")
        radius = Restriction.radius(collator, within_km, coords, near)
        V = model.out_proj.out_features
        self.k = int(k)
        if not 1 <= self.k <= min(ops.TOPK_MAX, V):
            raise ValueError(f"PredictLoop: k = {k} outside [1, {min(ops.TOPK_MAX, V)}]")
        super().__init__(model, collator, dataset, batch_size, rank, world, use_graph, buckets, side_collate)
        self.restriction = Restriction.on_device(model.label_offset, V, self.batch_size, self.device, exclude_visited, candidates,
                                                 radius=radius)
        self.prior = prior
        if prior is not None:
            prior.for_loop(model, self.device, self.batch_size, "PredictLoop")
        self.outs = {}                                      # (G, N) -> the [G, k] buffers its graphs write
        self.work = torch.empty(ops.topk_work_bytes(self.batch_size, V, self.k), dtype=torch.uint8, device=self.device)

    def _out(self, slot):
        key = (slot["layout"].G, slot["layout"].N)
        if key not in self.outs:
            G = key[0]
            self.outs[key] = (torch.empty(G, self.k, dtype=torch.int64, device=self.device),
                              torch.empty(G, self.k, dtype=torch.float32, device=self.device))
        return self.outs[key]

    def _step(self, slot, warm):
        self.model.recommend_step(self._collated(slot["batch"]), *self._out(slot), work=self.work, restriction=self.restriction,
                                  prior=self.prior)

    def run(self, max_batches=None):
        """One pass over this rank's part of the split -> (sample_index [n] int64, ids [n, k] int64, vals [n, k] f32), device
        tensors in batch order, no host read."""
        batches = self.batches(max_batches)
        flat = [i for b in batches for i in b]
        sample_index = torch.tensor(flat, dtype=torch.int64).to(self.device)
        ids = torch.full((len(flat), self.k), -1, dtype=torch.int64, device=self.device)
        vals = torch.full((len(flat), self.k), float("-inf"), dtype=torch.float32, device=self.device)
        starts = [0, *itertools.accumulate(len(b) for b in batches)]

        def launch(j, slot, st):
            """Rank batch j, then -- enqueued before the next batch is staged -- its lists into the result's rows."""
            self._launch(slot, st)
            bi, bv = self._out(slot)
            rows = [starts[j] + i for i, t in enumerate(batches[j]) if self.collator.keeps(self.dataset[t])]
            r = 0
            while r < len(rows):                         # runs of kept rows (one run unless a trajectory was dropped)
                e = r + 1
                while e < len(rows) and rows[e] == rows[e - 1] + 1:
                    e += 1
                ids[rows[r]:rows[e - 1] + 1].copy_(bi[r:e], non_blocking=True)
                vals[rows[r]:rows[e - 1] + 1].copy_(bv[r:e], non_blocking=True)
                r = e

        with self._evaluating():
            if self.prior is not None:
                self.prior.reset_status()
            for _ in self._pipeline(batches, launch):
                pass
        if self.prior is not None:
            self.prior.check("PredictLoop")
        return sample_index, ids, vals


class PriorFitLoop(_FrozenModelLoop):
    """One pass of the priors' maximum-likelihood weight fit (priorfit.py's docstring is the rule) over a held-out split, on
    EvalLoop's device data path: the eval loader's order, EpochLoop's buckets and staging, the weights as they are when run()
    starts, and per (G, bucket, forms.on("safe_forms")) ONE captured graph of

        model.poi_scores(model.encode(batch))                      the scores, [G, V]
        prior.features(batch, label_offset, ...)                   one blend of zeros per weight, into planes of ONE [K, rows, V] buffer
                                                                   (with scale_model the scores are copied into plane 0)
        mobgt_priorfit_terms                                       n, nll, gradient, Hessian of every (weight row, sample)
        acc += terms.sum(1)                                        ONE f64 [rows, NT] accumulator

    -- eager with use_graph=False and for collators whose finish needs torch ops, as in the other loops.

    prior: any prior (a prior.Prior) or a prior.Stack on the loop's device.  scale_model: the model's scores are
    feature 0 and scaled by a weight of their own, K = 1 + prior.n_weights; else they are the base and K = prior.n_weights.
    weights: the first weight rows, [L, K] (default: one row, `start` -- the prior's current weights, after a 1 for the model's
    scale).  rows: how many weight rows every launch evaluates (default 4: a Newton pass's step lengths); the graphs always
    evaluate that many, so a pass with fewer repeats its first row and no pass needs a new capture.

    set_rows(W) overwrites the device f64 [rows, K] the graphs read; run() zeroes the accumulator and the status words, makes one
    pass and reads the accumulator once: -> f64 numpy [L, NT], the terms summed over this split's samples for each row set.
    SNONFINITE (scores or features that are not finite) and a prior's SBADINDEX are a ValueError.  A fit on several ranks or
    under a restriction is not offered: world > 1, exclude_visited, candidates and within_km are refused."""

    def __init__(self, model, collator, dataset, prior, weights=None, scale_model=True, batch_size=16, use_graph=True, rows=4,
                 rank=None, world=None, buckets=None, side_collate=True, exclude_visited=False, candidates=None, within_km=None):
        import numpy as np
        from . import _priorfit, priorfit
        if not (hasattr(model, "poi_scores") and hasattr(model, "encode")):
            raise TypeError("PriorFitLoop: the model has no encode / poi_scores (the fq model, model_fqandtoyo.Graphormer)")
        if exclude_visited or candidates is not None or within_km is not None:
            raise ValueError("PriorFitLoop: a fit under a restriction (exclude_visited, candidates, within_km) is not offered: the "
                             "likelihood is that of the unrestricted softmax")
        self.scale_model = bool(scale_model)
        self.K = prior.n_weights + self.scale_model
        if self.K > _priorfit.MAX_K:
            raise ValueError(f"PriorFitLoop: {prior.n_weights} prior weights" + " and the model's scale" * self.scale_model +
                             f" are {self.K} features, one launch takes up to {_priorfit.MAX_K} (MOBGT_PRIORFIT_MAX_K)")
        self.rows = int(rows)
        if not 1 <= self.rows <= _priorfit.MAX_L:
            raise ValueError(f"PriorFitLoop: rows = {rows} outside 1 .. {_priorfit.MAX_L} (MOBGT_PRIORFIT_MAX_L)")
        super().__init__(model, collator, dataset, batch_size, rank, world, use_graph, buckets, side_collate)
        if self.world > 1:
            raise ValueError(f"PriorFitLoop: world = {self.world}: a fit on several ranks is not offered (run it on one)")
        prior.for_loop(model, self.device, self.batch_size, "PriorFitLoop")
        self.prior = prior
        V, B, K, L = model.out_proj.out_features, self.batch_size, self.K, self.rows
        self.NT = priorfit.nt_of(K)
        dev = self.device
        self.start = np.r_[[1.0] * self.scale_model, [prior.get_weights()[k] for k in prior.WEIGHTS]].astype(np.float64)
        self.W = torch.zeros(_priorfit.MAX_L, K, dtype=torch.float64, device=dev)
        self.feats = torch.zeros(K, B, V, dtype=torch.float32, device=dev)
        self.zeros = torch.zeros(B, V, dtype=torch.float32, device=dev)
        self.terms = torch.zeros(L * B * self.NT, dtype=torch.float64, device=dev)
        self.work = torch.empty(max(priorfit.work_bytes(K, B, V, L), 8), dtype=torch.uint8, device=dev)
        self.acc, self._scratch = (torch.zeros(L, self.NT, dtype=torch.float64, device=dev) for _ in range(2))
        self.status, self._scratch_status = (torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(2))
        self.live = 0
        self.set_rows(self.start[None, :] if weights is None else weights)

    def set_rows(self, W):
        """The weight rows of the next run(): [L, K] finite numbers, 1 <= L <= rows; the rows beyond L repeat the first."""
        import numpy as np
        W = np.asarray(W.detach().cpu().numpy() if isinstance(W, torch.Tensor) else W, dtype=np.float64)
        if W.ndim != 2 or W.shape[1] != self.K or not 1 <= W.shape[0] <= self.rows or not np.isfinite(W).all():
            names = ("scale",) * self.scale_model + tuple(self.prior.WEIGHTS)
            raise ValueError(f"PriorFitLoop.set_rows: 1 .. {self.rows} finite rows of ({', '.join(names)}) weights, got shape {tuple(W.shape)}")
        full = np.concatenate([W, np.repeat(W[:1], self.rows - len(W), axis=0)])
        self.W[:self.rows].copy_(torch.from_numpy(full))
        self.live = len(W)
        return self

    def _step(self, slot, warm):
        from . import priorfit
        model, lo, s = self.model, self.model.label_offset, int(self.scale_model)
        batch = self._collated(slot["batch"])
        with torch.no_grad():
            scores = model.poi_scores(model.encode(batch))
            G, V = scores.shape
            feats = self.feats[:, :G]
            if s:
                feats[0].copy_(scores)
            self.prior.features(batch, lo, feats[s:], V, self.zeros[:G])
            terms = self.terms[:self.rows * G * self.NT].view(self.rows, G, self.NT)
            priorfit.terms(None if s else scores, feats, batch.y, -lo, self.W[:self.rows], V=V, work=self.work, out=terms,
                           status=self._scratch_status if warm else self.status)
            (self._scratch if warm else self.acc).add_(terms.sum(1))

    def run(self, max_batches=None):
        """One pass over the split with the rows last set -> f64 numpy [L, NT]: sums of (n, nll, g_k, H_kj) over the samples."""
        with self._evaluating():
            self.acc.zero_()
            self.status.zero_()
            self.prior.reset_status()
            for _ in self._pipeline(self.batches(max_batches)):
                pass
            sums = self.acc.cpu().numpy()                   # the one read of the accumulator: the pass is over
            bits = int(self.status[0])
            self.prior.check("PriorFitLoop")
        if bits:
            raise ValueError(f"PriorFitLoop: scores or features that are not finite (status {bits}): a row held NaN or +inf, a "
                             "feature that is not finite, nothing but -inf, or -inf at its target; such rows were left out")
        return sums[:self.live]
