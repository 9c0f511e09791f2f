"""What the fused encoder layer launches, against the lists recorded before fused_layer.py was split into a plan
(layer_plan.py) and executors: tests/golden/layer_launch_traces.json, written by tools/layer_launch_trace.py at that commit.
Equal lists = the same kernel forms, in the same order, with the same scalar arguments and the same null / non-null pointers, for
every configuration of the tool's grid (3-layer fq / stock stacks, f32 / bf16, 33 / 608 / 4 710 rows, each form flipped alone, a
forward without gradients, one eager train step per variant).  A difference means the layer's behaviour moved: fix the code, the
fixture is only ever re-recorded on purpose."""
import functools
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "layer_launch_traces.json")
with open(GOLDEN) as _f:
    NAMES = list(json.load(_f)["traces"])


@functools.lru_cache(maxsize=None)
def _tool():
    spec = importlib.util.spec_from_file_location("layer_launch_trace", os.path.join(ROOT, "tools", "layer_launch_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def _both():
    """(recorded, produced now): produced once for all cases, read only."""
    return _tool().load(GOLDEN), _tool().traces()


@pytest.mark.gpu
def test_the_grid_is_the_recorded_one():
    want, got = _both()
    assert list(got) == list(want) and len(want) >= 100


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_launches_are_the_recorded_ones(name):
    want, got = _both()
    want, got = want[name], got[name]
    first = next((i for i, (a, b) in enumerate(zip(want, got)) if a != b), min(len(want), len(got)))
    assert want == got, (f"{name}: entry {first} of {len(got)} (recorded: {len(want)}) differs\n  recorded: "
                         f"{want[first] if first < len(want) else '<end>'}\n  now:      {got[first] if first < len(got) else '<end>'}")
