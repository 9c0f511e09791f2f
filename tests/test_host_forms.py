"""`mobgt_amd.forms`: the one parse of the switch variables, overrides, and the guard that the registry, the README's table and
the package's sources name the same switches.  No GPU."""
import os
import re
import subprocess
import sys

import pytest

from mobgt_amd import forms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# MOBGT_ variables that are not boolean form choices and stay where they are read
LEFT_OUT = {"MOBGT_DDP_PARTS", "MOBGT_ALGOS_BACKEND", "MOBGT_HIP_LIB", "MOBGT_NO_LIVE_PMC", "MOBGT_TEST_SHARED_GPU",
            "MOBGT_BENCH_NO_GROUPED"}


def test_one_parse_for_every_variable(monkeypatch):
    for row in forms.table():
        if row.env is None:
            continue
        for value in (None, "", "0"):
            if value is None:
                monkeypatch.delenv(row.env, raising=False)
            else:
                monkeypatch.setenv(row.env, value)
            assert forms.on(row.name) is row.default, (row.env, value)
        monkeypatch.setenv(row.env, "1")
        assert forms.on(row.name) is (not row.default), row.env
        for value in ("true", "2", " 1", "no"):
            monkeypatch.setenv(row.env, value)
            with pytest.raises(ValueError, match=row.env):
                forms.on(row.name)
        monkeypatch.delenv(row.env)


def test_polarity_follows_the_variable_name():
    """MOBGT_NO_X=1 turns the form `x` off; the forms without a variable are on."""
    for row in forms.table():
        if row.env is None:
            assert row.default is True, row.name
        elif row.env.startswith("MOBGT_NO_"):
            assert row.name == row.env[len("MOBGT_NO_"):].lower() and row.default is True, row
        assert row.doc
    names = [row.name for row in forms.table()]
    assert len(names) == len(set(names))
    assert {"ln_gemm", "own_gemm", "tail", "chain_bwd", "wgrad_big", "bias_bwd_beside", "sp_gather"} == \
        {row.name for row in forms.table() if row.env is None}


def test_the_variable_is_read_at_call_time(monkeypatch):
    monkeypatch.delenv("MOBGT_SAFE_FORMS", raising=False)
    assert not forms.on("safe_forms")
    monkeypatch.setenv("MOBGT_SAFE_FORMS", "1")
    assert forms.on("safe_forms")


def test_an_override_beats_the_environment(monkeypatch):
    monkeypatch.setenv("MOBGT_NO_CHAIN", "1")
    assert not forms.on("chain")
    forms.set("chain", True)
    try:
        assert forms.on("chain")
        monkeypatch.setenv("MOBGT_NO_CHAIN", "junk")          # (not even parsed while an override is present)
        assert forms.on("chain")
    finally:
        forms.set("chain", None)
    monkeypatch.setenv("MOBGT_NO_CHAIN", "1")
    assert not forms.on("chain")


def test_unknown_names_raise():
    for call in (lambda: forms.on("no_such_form"), lambda: forms.set("no_such_form", True)):
        with pytest.raises(KeyError):
            call()
    with pytest.raises(KeyError):
        with forms.using(no_such_form=True):
            pass


def test_using_restores_on_exit_and_on_an_exception(monkeypatch):
    monkeypatch.delenv("MOBGT_NO_CHAIN", raising=False)
    forms.set("tail", False)
    try:
        with forms.using(chain=False, tail=True, sp_gather=False):
            assert not forms.on("chain") and forms.on("tail") and not forms.on("sp_gather")
            with forms.using(chain=None):                      # (None: back to the variable / the default for the body)
                assert forms.on("chain")
            assert not forms.on("chain")
        assert forms.on("chain") and not forms.on("tail") and forms.on("sp_gather")
        with pytest.raises(RuntimeError, match="boom"):
            with forms.using(chain=False, tail=True):
                raise RuntimeError("boom")
        assert forms.on("chain") and not forms.on("tail")
    finally:
        forms.set("tail", None)
    assert forms.on("tail")


def test_forms_needs_neither_torch_nor_the_rest_of_the_package():
    code = ("import sys; import mobgt_amd.forms; "
            "bad = [m for m in sys.modules if m == 'torch' or (m.startswith('mobgt_amd.') and m != 'mobgt_amd.forms')]; "
            "assert not bad, bad")
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)


def _readme_table_names():
    lines = open(os.path.join(ROOT, "README.md")).read().split("## Environment switches", 1)[1].splitlines()
    return set(re.findall(r"MOBGT_[A-Z0-9_]+", "\n".join(l for l in lines if l.startswith("|"))))


def test_readme_table_and_registry_name_the_same_switches():
    in_readme = _readme_table_names()
    in_registry = {row.env for row in forms.table() if row.env is not None}
    assert in_registry <= in_readme, sorted(in_registry - in_readme)
    assert in_readme <= in_registry | LEFT_OUT, sorted(in_readme - in_registry - LEFT_OUT)
    text = open(os.path.join(ROOT, "README.md")).read()
    for row in forms.table():
        if row.env is None:
            assert "`%s`" % row.name in text, row.name


def test_no_other_module_reads_a_switch_variable():
    """`environ` beside `MOBGT_` only in forms.py, the fork-safe host half (algos.py), the library path (_lib.py) and the integer
    MOBGT_DDP_PARTS of train.py."""
    pkg = os.path.join(ROOT, "mobgt_amd")
    found = []
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if not f.endswith(".py") or (dirpath == pkg and f in ("forms.py", "algos.py", "_lib.py")):
                continue
            for no, line in enumerate(open(os.path.join(dirpath, f), encoding="utf-8"), 1):
                if "environ" in line and "MOBGT_" in line and not (f == "train.py" and "MOBGT_DDP_PARTS" in line):
                    found.append("%s:%d: %s" % (f, no, line.strip()))
    assert not found, found
