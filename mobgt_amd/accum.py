"""Host bookkeeping of gradient accumulation (`train.TrainStep(accumulate=k, clip_norm=c)`): which call of `step` / `flush`
ends a window with an optimizer update, and what the counters read afterwards.  Pure Python, no device: the device side
(accumulator, norm, scaled AdamW) is csrc/layer.hip, driven by train.TrainStep from the decisions made here.

Lightning's rules (`Trainer(accumulate_grad_batches=k, gradient_clip_val=c)`): the k-th micro-step of a window updates; an epoch's
last batch always updates (`flush`); every micro-loss is divided by k whatever the window's length, so the update's gradient
is `sum / k` also for a flushed short window; the scheduler steps once per UPDATE.
"""
from .lr import polynomial_decay_lr


def check_accum_args(accumulate, clip_norm):
    """-> (k, c): validated `accumulate` (integer >= 1) and `clip_norm` (None, or a float > 0)."""
    if isinstance(accumulate, bool) or int(accumulate) != accumulate or int(accumulate) < 1:
        raise ValueError(f"accumulate must be an integer >= 1, got {accumulate!r}")
    if clip_norm is not None:
        if isinstance(clip_norm, bool) or not float(clip_norm) > 0.0 or float(clip_norm) == float("inf"):
            raise ValueError(f"clip_norm must be None or a finite number > 0, got {clip_norm!r}")
        clip_norm = float(clip_norm)
    return int(accumulate), clip_norm


def scheduled_lr(sched):
    """Learning rate of the NEXT update: the schedule (TrainStep.sched_state: step_count, warmup, tot, lr, end_lr, power) at its
    current step count."""
    return polynomial_decay_lr(sched["step_count"], sched["warmup"], sched["tot"], sched["lr"], sched["end_lr"], sched["power"])


class UpdateWindow:
    """Window position and update count.  The schedule's dict is passed per call (its one owner is the trainer): an update steps
    `sched["step_count"]` once."""

    def __init__(self, accumulate=1):
        self.accumulate, _ = check_accum_args(accumulate, None)
        self.window_pos = 0            # micro-steps in the open window
        self.updates_done = 0

    def updated(self, sched=None, n=1):
        """n optimizer updates have been issued: counts them and steps the schedule once per update."""
        if sched is not None:
            sched["step_count"] += n
        self.updates_done += n

    def step(self, sched=None):
        """One micro-step enters the window.  -> True when it is the window's last: the caller must update now."""
        self.window_pos += 1
        if self.window_pos < self.accumulate:
            return False
        self.window_pos = 0
        self.updated(sched)
        return True

    def flush(self, sched=None):
        """End an incomplete window.  -> True when there is something to update from (no-op on an empty window)."""
        if self.window_pos == 0:
            return False
        self.window_pos = 0
        self.updated(sched)
        return True

    def state(self):
        return (self.window_pos, self.updates_done)

    def restore(self, state):
        """Back to a `state()` (guarded_step's re-run)."""
        self.window_pos, self.updates_done = state
