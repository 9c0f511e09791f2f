"""What a fused encoder layer launches, configuration by configuration, as an ordered list per configuration: every native
entry point that goes through `_lib.lib()` with its Python int / float / bool arguments (pointers and ctypes arrays as 0 = null /
1 = non-null) and, interleaved, every aten op that launches a kernel (views and `empty` do not).  Two commits whose lists are
equal choose the same kernel forms with the same arguments in the same order: tests/test_gpu_layer_trace.py compares against
tests/golden/layer_launch_traces.json, which this tool wrote at the commit before fused_layer.py was split into plan + executors.

    python tools/layer_launch_trace.py OUT.json          (needs the GPU; ~15 s)

It uses nothing of fused_layer.py itself: the two EncoderLayer classes, model.refresh_shadows, forms.using, the `_lib.lib` spy of
the GPU tests (tests/test_host_native.py: test_call_of_lib_goes_through_the_modules_lib) and a TorchDispatchMode.
The SECOND pass of a configuration is the recorded one (the first allocates workspaces and probes torch for `out_dtype`)."""
import ctypes
import json
import os
import sys

import torch
from torch.utils._python_dispatch import TorchDispatchMode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from mobgt_amd import _lib, forms  # noqa: E402

DEV = "cuda"
SHAPES = ((3, 11), (16, 38), (6, 785))                  # 33, 608 and 4 710 rows (the last: past the 4 096-row switch)
STACKS = (("fq", 192), ("fq", 256), ("stock", 128), ("stock", 192))
FLIPS = ("chain", "chain_bwd", "chain_big", "ln_gemm", "ln_gemm_bwd", "own_gemm", "tail", "defer_tail", "wgrad_big", "stock_ln_qkv",
         "safe_forms")
# aten ops that launch nothing: views are recognised by their schema, these by name
_NO_KERNEL = {"empty", "empty_like", "empty_strided", "new_empty", "new_empty_strided", "detach", "alias", "lift_fresh",
              "_local_scalar_dense", "is_pinned", "record_stream", "set_", "resize_", "_pin_memory", "_has_compatible_shallow_copy_type"}


def flip_matters(name, variant, bf16, R):
    """A flip that cannot change what a configuration launches is skipped: f32 activations take none of the forms; the others by
    the variant and the row count they are read under."""
    if not bf16 or (variant == "stock" and R > 4096):     # (pre-LN past 4 096 rows: the library's GEMMs whatever the forms say)
        return False
    return {"chain_big": variant == "fq" and R > 4096, "wgrad_big": variant == "fq" and R > 4096, "tail": variant == "fq",
            "stock_ln_qkv": variant == "stock"}.get(name, True)


class Recorder(TorchDispatchMode):
    """`with Recorder() as rec:` -> rec.entries, the ordered list."""

    def __init__(self):
        super().__init__()
        self.entries = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        name = func._schema.name.split("::")[-1]
        if not (func.is_view or name in _NO_KERNEL):
            self.entries.append(name)
        return func(*args, **(kwargs or {}))

    def _native(self, name, fn):
        kinds = _lib.SIGNATURES[name][1]

        def call(*args):
            self.entries.append(name + "(" + ",".join(_show(a, k is ctypes.c_void_p) for a, k in zip(args, kinds)) + ")")
            return fn(*args)
        return call

    def __enter__(self):
        rec, self._real = self, _lib.lib
        real = _lib.lib()

        class _Spy:
            def __getattr__(self, name):
                return rec._native(name, getattr(real, name))
        _lib.lib = lambda: _Spy()
        return super().__enter__()

    def __exit__(self, *exc):
        _lib.lib = self._real
        return super().__exit__(*exc)


def _show(a, pointer):
    """`pointer`: the header declares the parameter as one (some callers pass an address as a plain int)."""
    if pointer and isinstance(a, int):
        return "1" if a else "0"
    if isinstance(a, (bool, int)):
        return str(int(a))
    if isinstance(a, float):
        return repr(a)
    if a is None:
        return "0"
    if isinstance(a, ctypes.c_void_p):
        return "1" if a.value else "0"
    if isinstance(a, (ctypes.Array, ctypes._Pointer)):
        return "1"
    raise TypeError(f"an argument of type {type(a).__name__} in a native call")


def _stack(variant, C):
    from mobgt_amd.model import EncoderLayer as StockLayer
    from mobgt_amd.model_fqandtoyo import EncoderLayer as FqLayer
    torch.manual_seed(5)
    cls = FqLayer if variant == "fq" else StockLayer
    layers = torch.nn.ModuleList([cls(C, 1024, 0.1, 0.1, 8) for _ in range(3)]).to(DEV)
    for li, l in enumerate(layers):
        l.self_attention.set_layer_index(li + 1)
        l.self_attention.seed_dev = torch.tensor([11], dtype=torch.int64, device=DEV)
    return layers.train()


def _run_stack(layers, x0, bias, gy, rec=None):
    from mobgt_amd.model import refresh_shadows
    for q in layers.parameters():
        q.grad = None
    x = x0.clone().requires_grad_(gy is not None)
    refresh_shadows(layers, rows=x0.shape[0] * x0.shape[1])
    torch.cuda.synchronize()
    if rec is not None:
        rec.__enter__()
    try:
        y = x
        for li, l in enumerate(layers):
            y = l(y, bias, next_layer=layers[li + 1] if li + 1 < len(layers) else None)
        if gy is not None:
            y.backward(gy)
    finally:
        if rec is not None:
            rec.__exit__(None, None, None)
    torch.cuda.synchronize()


def _second_pass(layers, x0, bias, gy, **flipped):
    with forms.using(**flipped):
        _run_stack(layers, x0, bias, gy)
        rec = Recorder()
        _run_stack(layers, x0, bias, gy, rec)
    return rec.entries


def layer_traces():
    """{configuration name: entries} of the 3-layer stacks called with `next_layer=` (training mode, p = 0.1)."""
    out = {}
    for variant, C in STACKS:
        layers = _stack(variant, C)
        for G, T in SHAPES:
            torch.manual_seed(7)
            x0, gy = torch.randn(G, T, C, device=DEV), torch.randn(G, T, C, device=DEV)
            bias = torch.randn(G, 8, T, T, device=DEV) * 0.3
            for dt in (torch.float32, torch.bfloat16):
                bf16 = dt == torch.bfloat16
                for l in layers:
                    l.act_dtype = dt
                base = f"{variant} C={C} {'bf16' if bf16 else 'f32'} G={G} T={T}"
                out[base + " default"] = _second_pass(layers, x0, bias, gy)
                for name in FLIPS:
                    if flip_matters(name, variant, bf16, G * T):
                        out[f"{base} {name}={int(not forms.on(name))}"] = _second_pass(layers, x0, bias, gy, **{name: not forms.on(name)})
                if bf16 and (G, T) == (16, 38) and C == 192 - 64 * (variant == "stock"):
                    with torch.no_grad():                  # the `need_bwd` false branch (pre-LN chain without its backward packs)
                        out[base + " no_grad"] = _second_pass(layers, x0, bias, None)
    return out


def train_step_traces():
    """One eager train step per variant on the suite's smallest synthetic workload: the sink-dependent branches (small_sink, the
    deferred tail, the step's grouped weight gradients)."""
    from mobgt_amd import workloads
    from mobgt_amd.train import TrainStep
    out = {}
    for variant in ("fq", "stock"):
        uni, model, coll = workloads.build("fsq", DEV, seed=1, variant=variant, model_overrides=dict(n_layers=2))
        batches = [coll(t) for t in workloads.make_pool("fsq", 1, 16, uni)]
        ts = TrainStep(model, batches, use_graph=False, seed=1)
        ts.prepare()
        ts.step(0)
        torch.cuda.synchronize()
        with Recorder() as rec:
            ts.step(1)
        torch.cuda.synchronize()
        out[f"train step {variant} eager"] = rec.entries
    return out


def traces():
    out = layer_traces()
    out.update(train_step_traces())
    return out


def dump(tr, path):
    """One line per configuration: indices into the table of distinct entries."""
    table = sorted({e for v in tr.values() for e in v})
    at = {e: i for i, e in enumerate(table)}
    with open(path, "w") as f:
        f.write('{"entries": [\n' + ",\n".join(json.dumps(e) for e in table) + '\n],\n"traces": {\n')
        f.write(",\n".join(json.dumps(k) + ": " + json.dumps([at[e] for e in v], separators=(",", ":")) for k, v in tr.items()))
        f.write("\n}}\n")


def load(path):
    with open(path) as f:
        d = json.load(f)
    return {k: [d["entries"][i] for i in v] for k, v in d["traces"].items()}


if __name__ == "__main__":
    tr = traces()
    dump(tr, sys.argv[1])
    print(f"{len(tr)} configurations, {sum(map(len, tr.values()))} entries -> {sys.argv[1]}")
