"""mobgt_amd/step_state.py: the declaration table of the train step's hand-overs and what follows from it (no torch, no GPU)."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mobgt_amd")


def _load():
    # by path: the module imports nothing from the package, and importing the package's ops would pull in torch
    spec = importlib.util.spec_from_file_location("_step_state_under_test", os.path.join(PKG, "step_state.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ss = _load()
PARKED = [f.name for f in ss.FIELDS if f.scope == ss.PARKED]
CARRIED = [f.name for f in ss.FIELDS if f.scope == ss.CARRIED]
SWITCHES = [f.name for f in ss.FIELDS if f.scope == ss.SWITCH]
OLD_NAMES = ("_ARENA", "_GRAD_SINKS", "_SINK_CENSUS", "_BIAS_BWD_JOB", "_FRONT_DEFER", "_TOKEN_FWD", "_TOKEN_CHAIN", "_TOKEN_PENDING",
             "_FRONT_SGEMM", "_WGRAD_DEFER", "_PENDING_TAIL", "_PENDING_CB", "_PENDING_PACK", "_prelaunched")


def _dummy(st, name, key=(7, 0, 0x1000)):
    """Put one dummy object into the field the way its owner would: into the container, or in place of None."""
    cur = getattr(st, name)
    if isinstance(cur, dict):
        cur[key] = object()
    elif isinstance(cur, list):
        cur.append(object())
    else:
        setattr(st, name, object())


def test_the_table_declares_every_field_once_with_a_scope_and_a_description():
    names = [f.name for f in ss.FIELDS]
    assert len(names) == len(set(names)) and len(OLD_NAMES) == 14
    for f in ss.FIELDS:
        assert f.scope in (ss.PARKED, ss.CARRIED, ss.SWITCH) and f.doc.strip(), f
    # what the trainer's leftover check has to see: the jobs, the four weight-gradient slots, the three it used to skip
    assert {"bias_bwd_job", "front_hop", "front_ni", "token_fwd", "token_pending", "front_sgemm", "wgrad_items", "wgrad_hop",
            "wgrad_hop_wide", "wgrad_stock_tok", "wgrad_psum", "layer_tails", "weight_pack", "gcn_prelaunched"} <= set(PARKED)
    assert {"token_chain", "grad_sinks", "token_fwd_fused_calls"} <= set(CARRIED)
    assert {"wgrad_on", "front_on", "token_fwd_on", "zero_arena", "sink_census"} <= set(SWITCHES)
    assert isinstance(ss.STEP, ss.StepState) and not hasattr(ss, "threading")


def test_a_fresh_state_has_no_leftovers():
    assert ss.StepState().leftovers() == {}
    assert ss.STEP.leftovers() == {}


@pytest.mark.parametrize("name", PARKED)
def test_a_parked_job_is_named_by_the_leftover_check(name):
    st = ss.StepState()
    _dummy(st, name)
    assert list(st.leftovers()) == [name]


@pytest.mark.parametrize("name", CARRIED + SWITCHES)
def test_carried_fields_and_switches_are_no_leftovers(name):
    st = ss.StepState()
    _dummy(st, name)
    assert st.leftovers() == {}


def test_drop_parked_empties_every_parked_field_and_nothing_else():
    st = ss.StepState()
    for name in PARKED + CARRIED + SWITCHES:
        _dummy(st, name)
    kept = {name: getattr(st, name) for name in CARRIED + SWITCHES}
    assert sorted(st.leftovers()) == sorted(PARKED)
    st.drop_parked()
    assert st.leftovers() == {}
    fresh = ss.StepState()
    for name in PARKED:
        assert getattr(st, name) == getattr(fresh, name), name
    for name, v in kept.items():
        assert getattr(st, name) is v and v not in (None, {}, [], 0, False), name


def test_layer_tails_are_dropped_by_graph_task_never_wholesale():
    st = ss.StepState()
    st.layer_tails[(7, 0, 0x1000)] = "running task's"
    st.layer_tails[(3, 0, 0x2000)] = "a dead task's"
    st.tail_check_task = 7
    st.bias_bwd_job = object()
    st.drop_parked(task_id=7)                      # (from inside task 7's backward pass)
    assert st.layer_tails == {(7, 0, 0x1000): "running task's"} and st.tail_check_task == 7 and st.bias_bwd_job is None
    st.drop_stale_tails(8)                         # (the next backward pass meets what task 7 left when it died)
    assert st.layer_tails == {} and st.tail_check_task is None


def test_keeping_carried_puts_the_carried_fields_back():
    st = ss.StepState()
    st.token_chain, st.grad_sinks, st.token_fwd_fused_calls = "train forward's chain", {1: "sink"}, 5
    before = {name: getattr(st, name) for name in CARRIED}
    with st.keeping_carried():
        st.token_chain, st.grad_sinks, st.token_fwd_fused_calls = None, {}, 9
    assert {name: getattr(st, name) for name in CARRIED} == before

    class Boom(Exception):
        pass
    with pytest.raises(Boom):
        with st.keeping_carried():
            for name in CARRIED:
                setattr(st, name, object())
            raise Boom
    assert {name: getattr(st, name) for name in CARRIED} == before and st.token_chain is before["token_chain"]


def test_the_old_registries_are_gone_and_no_module_reaches_into_ops_privates():
    for fn in ("ops.py", "fused_layer.py", "model.py", "modelGNN.py", "model_fqandtoyo.py"):
        src = open(os.path.join(PKG, fn)).read()
        for old in OLD_NAMES:
            assert not re.search(r"(?<![A-Za-z0-9_])" + re.escape(old) + r"(?![A-Za-z0-9_])", src), (fn, old)
    for dirpath, _, files in os.walk(PKG):
        for fn in files:
            if fn.endswith((".py", ".h", ".hip", ".md", ".txt")) or "." not in fn:
                src = open(os.path.join(dirpath, fn), errors="replace").read()
                assert not re.search(r"ops\._[A-Z]", src), os.path.join(dirpath, fn)
