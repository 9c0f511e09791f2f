"""Host side of gradient accumulation and global-norm clipping (`TrainStep(accumulate=, clip_norm=)`): the new C-ABI entry
points are declared, bound with the declared arity and exported; the window bookkeeping (`mobgt_amd.accum.UpdateWindow`) says
which calls update and what the counters and the schedule read afterwards.  No GPU."""
import math
import os
import re

import pytest

from mobgt_amd import _lib
from mobgt_amd.lr import polynomial_decay_lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mobgt_grad_norm_block", "mobgt_grad_accumulate", "mobgt_grad_norm_finish", "mobgt_adamw_flat_scaled")


def _declared_arity(hdr, name):
    m = re.search(r"\b(?:int|int64_t)\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
    assert m, f"{name} is not declared in include/mobgt_hip.h"
    args = m.group(1).strip()
    return 0 if args in ("", "void") else args.count(",") + 1


def test_new_exports_are_declared_bound_and_built():
    hdr = open(os.path.join(ROOT, "include", "mobgt_hip.h")).read()
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == _declared_arity(hdr, name), name
    # the scaled AdamW is the plain one + (scale_dev, zero_grads)
    assert len(_lib.SIGNATURES["mobgt_adamw_flat_scaled"][1]) == len(_lib.SIGNATURES["mobgt_adamw_flat"][1]) + 2
    assert re.search(r"#define\s+MOBGT_ABI_VERSION\s+3\b", hdr) and _lib.ABI_VERSION == 3
    _lib.build()
    handle = _lib.lib()
    for name in NEW:
        assert hasattr(handle, name), name
    blk = int(handle.mobgt_grad_norm_block())
    assert blk >= 1024 and blk % 1024 == 0          # whole 16-byte passes of a 256-thread workgroup


SCHED = dict(warmup=4, tot=40, lr=1e-3, end_lr=1e-9, power=1.0)


@pytest.mark.parametrize("k", [1, 3, 8])
def test_window_bookkeeping(k):
    """A sequence of step / flush calls: which of them update, and updates_done / window_pos / step_count after each; the
    learning rate update u runs at (the schedule read right before the call that updates) is the schedule at u, however many
    micro-steps the windows had."""
    from mobgt_amd.accum import UpdateWindow, scheduled_lr
    sched = dict(SCHED, step_count=1)
    w = UpdateWindow(k)
    calls = ["s"] * (2 * k + 1) + ["f", "f"] + ["s"] * k + ["f"] + ["s"] * max(1, k - 1) + ["f"]
    pos = upd = 0
    for c in calls:
        lr_of_next_update = scheduled_lr(sched)
        if c == "s":
            want = pos + 1 == k
            pos = 0 if want else pos + 1
            got = w.step(sched)
        else:
            want = pos > 0                       # a flush updates from a short window and is a no-op on an empty one
            pos = 0
            got = w.flush(sched)
        upd += int(want)
        assert got == want, (k, c)
        assert (w.window_pos, w.updates_done, sched["step_count"]) == (pos, upd, 1 + upd)
        if want:
            assert lr_of_next_update == polynomial_decay_lr(upd, SCHED["warmup"], SCHED["tot"], SCHED["lr"], SCHED["end_lr"], 1.0)
        else:
            assert scheduled_lr(sched) == lr_of_next_update          # a micro-step inside a window leaves the schedule alone
    n_steps = calls.count("s")
    assert upd >= math.ceil(n_steps / k)
    # k = 1: every step updates and no flush ever does
    if k == 1:
        assert upd == n_steps


def test_window_state_round_trip():
    """guarded_step's snapshot: a restored window counts a re-run micro-step once."""
    from mobgt_amd.accum import UpdateWindow
    sched = dict(SCHED, step_count=1)
    w = UpdateWindow(2)
    w.step(sched)
    snap, snap_sched = w.state(), dict(sched)
    assert w.step(sched) and w.updates_done == 1 and sched["step_count"] == 2
    w.restore(snap)
    sched = snap_sched
    assert (w.window_pos, w.updates_done, sched["step_count"]) == (1, 0, 1)
    assert w.step(sched) and w.updates_done == 1 and sched["step_count"] == 2


@pytest.mark.parametrize("bad", [dict(accumulate=0), dict(accumulate=-2), dict(accumulate=1.5), dict(clip_norm=0), dict(clip_norm=-1.0),
                                 dict(clip_norm=float("nan")), dict(clip_norm=float("inf"))])
def test_bad_arguments_are_refused(bad):
    from mobgt_amd.accum import check_accum_args
    with pytest.raises(ValueError):
        check_accum_args(**dict(dict(accumulate=1, clip_norm=None), **bad))
    assert check_accum_args(4, 0.5) == (4, 0.5) and check_accum_args(1, None) == (1, None)
