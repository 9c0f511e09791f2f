"""mobgt_amd/step_graphs.py on the host: the cache of a TrainStep's captured graphs and the key of a group of steps.  Stub graphs
that count their replays stand in for hipGraphs."""
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load():
    """step_graphs.py by path: it must import without the package (and so without torch or a GPU)."""
    spec = importlib.util.spec_from_file_location("_step_graphs_alone", os.path.join(ROOT, "mobgt_amd", "step_graphs.py"))
    mod = importlib.util.module_from_spec(spec)
    before = set(sys.modules)
    spec.loader.exec_module(mod)
    assert not {m for m in set(sys.modules) - before if m.split(".")[0] in ("torch", "mobgt_amd")}
    return mod


sg = _load()


class StubGraph:
    def __init__(self):
        self.replays = 0

    def replay(self):
        self.replays += 1


def _capturer(log):
    def capture(*args):
        log.append(args)
        return sg.Entry((StubGraph(),), object())
    return capture


def test_get_captures_once_per_key_and_hands_back_the_same_entry():
    cache, log = sg.StepGraphs(), []
    cap = _capturer(log)
    keys = [("step", 0, False), ("step", 1, False), ("step", 0, True), ("micro", 0), ("update", True), ("opt",),
            sg.group_key(0, 2, 2, False)]
    first = [cache.get(k, cap, k) for k in keys]
    for lap in range(3):
        for k, e in zip(keys, first):
            got = cache.get(k, cap, k)
            assert got is e
            for g in got.graphs:
                g.replay()
    assert log == [(k,) for k in keys]                      # one capture per key, with the arguments given, in first-use order
    assert all(e.graphs[0].replays == 3 for e in first)
    assert len({id(e) for e in first}) == len(keys) and len({id(e.loss) for e in first}) == len(keys)


def test_group_key_names_the_batches_it_runs():
    assert sg.group_key(3, 2, 4, False) == ("group", (3, 0), False)
    assert sg.group_key(3, 2, 5, False) == ("group", (3, 4), False)
    assert sg.group_key(3, 2, 4, False) != sg.group_key(3, 2, 5, False)
    assert sg.group_key(7, 2, 4, False) == sg.group_key(3, 2, 4, False)          # (steps are taken cyclically from the pool)
    assert sg.group_key(0, 5, 2, True) == ("group", (0, 1, 0, 1, 0), True)
    assert sg.group_key(1, 1, 3, 0) == ("group", (1,), False)


def test_with_and_without_the_exchange_are_distinct_entries():
    assert sg.group_key(3, 2, 4, True) != sg.group_key(3, 2, 4, False)
    cache, log = sg.StepGraphs(), []
    cap = _capturer(log)
    a = cache.get(sg.group_key(3, 2, 4, True), cap, "comm")
    b = cache.get(sg.group_key(3, 2, 4, False), cap, "nocomm")
    c = cache.get(("step", 1, True), cap, "step comm")
    d = cache.get(("step", 1, False), cap, "step nocomm")
    assert a is not b and c is not d and a.loss is not b.loss and c.loss is not d.loss
    assert [x[0] for x in log] == ["comm", "nocomm", "step comm", "step nocomm"]
    assert set(cache.of("group")) == {("group", (3, 0), True), ("group", (3, 0), False)}
    assert set(cache.of("step")) == {("step", 1, True), ("step", 1, False)}


def test_clear_leaves_nothing_listed_and_the_next_get_captures_again():
    cache, log = sg.StepGraphs(), []
    cap = _capturer(log)
    keys = [("step", 0, False), ("micro", 1), ("update", False), ("opt",), sg.group_key(1, 3, 2, True)]
    old = [cache.get(k, cap) for k in keys]
    kinds = ("step", "micro", "update", "opt", "group")
    assert all(len(cache.of(kind)) == 1 for kind in kinds)
    cache.clear()
    assert all(cache.of(kind) == {} for kind in kinds)
    new = [cache.get(k, cap) for k in keys]
    assert len(log) == 2 * len(keys) and all(n is not o for n, o in zip(new, old))
