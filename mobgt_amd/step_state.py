"""The hand-overs of one train step -- one autograd node parks a job, a later launch takes it -- as fields of `STEP`, declared
ONCE in `FIELDS`: the leftover check, the drop after a pass that raised and the save / restore around an evaluation walk that
table.  The launches stay in ops.py / fused_layer.py / model.py.  Imports nothing from the package, needs no torch (like forms.py).
`STEP` is process-wide, not thread-local: a job parked by the forward pass on the caller's thread is taken by a launch the
autograd engine issues from ITS thread, and ONE step is in flight per process."""
import contextlib
from collections import namedtuple

# scope -- parked: must be empty behind a completed forward + backward;  carried: legitimately outlives the step;  switch: a mode
PARKED, CARRIED, SWITCH = "parked", "carried", "switch"
Field = namedtuple("Field", "name scope new doc")          # new(): the empty value;  doc: who parks, who takes
_none = type(None)                                         # (_none() is None)

FIELDS = (
    Field("zero_arena", SWITCH, _none, "TrainStep._prologue sets the step's ZeroArena; ops.zeros_f32 carves from it"),
    Field("grad_sinks", CARRIED, dict, "TrainStep (ops.set_grad_sinks): parameter address -> (weak parameter, gradient view); ops.grad_sink reads"),
    Field("sink_census", SWITCH, lambda: {"on": False, "cur": {}, "max": {}}, "train.used_parameters' dry run counts ops.grad_sink requests per forward"),
    Field("bias_bwd_job", PARKED, _none, "_BuildBiasFn.forward parks; the category GCN's backward launch, the side stream or its own backward takes"),
    Field("dist_gu_job", PARKED, _none, "_DistGcnFn.forward parks (ops.park_dist_gu_job); the encoder input's burst scatter takes, or that node's own backward drops"),
    Field("front_on", SWITCH, bool, "the model's forward (ops.front_deferral) around the hop table and the node indices"),
    Field("front_hop", PARKED, _none, "_HopTableFn.forward parks; the category GCN's / stock front's forward launch or ops.flush_front takes"),
    Field("front_ni", PARKED, _none, "ops.node_index parks; the same launches take"),
    Field("token_fwd_on", SWITCH, bool, "model_fqandtoyo.node_features (ops.token_fwd_deferral)"),
    Field("token_fwd", PARKED, dict, "'gather' / 'f2' / 'f4': _GatherMultiFn / _LinearSplitKFn.forward record; _AssembleTokensFn launches them as one"),
    Field("token_fwd_fused_calls", CARRIED, int, "how often mobgt_token_fwd_chain took the three records (a counter for tests)"),
    Field("token_chain", CARRIED, _none, "ops.register_token_chain: the encoder-input chain of the forward that just ran; its backward reads it"),
    Field("token_pending", PARKED, dict, "_AssembleTokensFn.backward parks under a gradient's address (with the first layer's tail, taken from layer_tails, "
          "under 'tail'); FuseEmbeddings-4 / -2's backward re-park / launch"),
    Field("front_sgemm", PARKED, dict, "'job': ops.front_small_gemm parks, the bias assembly's launch takes; 'done': its result until ops.small_gemm asks"),
    Field("wgrad_on", SWITCH, bool, "ops.recording_wgrads around the trainer's backward"),
    Field("wgrad_items", PARKED, list, "leaf weight gradients (ops.linear_wgrad*, fused layers) for ops.flush_deferred_wgrads' grouped launch"),
    Field("wgrad_hop", PARKED, _none, "_HopTableFn.backward parks; rides in the flush's first grouped launch"),
    Field("wgrad_hop_wide", PARKED, _none, "_HopTableFn.backward past 256 edge ids; shares the flush's stock tail launch"),
    Field("wgrad_stock_tok", PARKED, _none, "_StockTokensFn.backward parks; the flush's stock tail launch takes"),
    Field("wgrad_psum", PARKED, list, "ops.defer_partial_sum: split-K partial sums for the flush's one reduction launch"),
    Field("layer_tails", PARKED, dict, "(graph task, device, address of dx1) -> a fused layer's tail; the chain launch of the layer below (first layer: "
          "the encoder input's backward) takes"),
    Field("tail_check_task", PARKED, _none, "graph task whose end-of-backward check (fused_layer._pending_check) is queued"),
    Field("weight_pack", PARKED, list, "model.pack_layer_weights(defer=True) parks; the category GCN's / stock front's forward launch takes"),
    Field("gcn_prelaunched", PARKED, dict, "modelGNN.prelaunch_small_gcn: id(module) -> (key, result); that module's forward adopts it"),
)


class StepState:
    def __init__(self):
        for f in FIELDS:
            setattr(self, f.name, f.new())

    def leftovers(self):
        """{field: what it still holds} over the parked fields -- {} when a forward + backward consumed everything it parked."""
        held = {f.name: getattr(self, f.name) for f in FIELDS if f.scope == PARKED}
        return {k: sorted(map(str, v)) if isinstance(v, dict) else len(v) if isinstance(v, list) else type(v).__name__
                for k, v in held.items() if v is not None and v != [] and v != {}}

    def drop_stale_tails(self, task_id):
        """Tails parked by a backward pass that is not the running one: that pass died before its end-of-backward callback ran (an
        exception in a backward function: the engine then skips the callbacks).  Their buffers belong to a dead graph: drop them,
        never feed them to a kernel.  (An entry holds views of its buffers, so while it is parked no other tensor can be allocated
        at its address: a key of the RUNNING task always names the tensor it was parked under.)"""
        if self.tail_check_task != task_id:
            self.tail_check_task = None
        for k in [k for k in self.layer_tails if k[0] != task_id]:
            del self.layer_tails[k]

    def drop_parked(self, task_id=-1):
        """After a pass that raised: forget everything parked -- its buffers belong to a dead graph.  Layer tails of the graph
        task that is running (`task_id`, -1 outside a backward pass) stay: they are that task's to finish."""
        self.drop_stale_tails(task_id)
        for f in FIELDS:
            if f.scope == PARKED and f.name not in ("layer_tails", "tail_check_task"):
                setattr(self, f.name, f.new())

    @contextlib.contextmanager
    def keeping_carried(self):
        """Put the carried fields back on the way out (an evaluation between two train steps)."""
        saved = {f.name: getattr(self, f.name) for f in FIELDS if f.scope == CARRIED}
        try:
            yield
        finally:
            for k, v in saved.items():
                setattr(self, k, v)


STEP = StepState()
