"""`bench.py`'s switches on the host: a plain run is the headline alone, `--full` turns the other legs on, and the secondary
workloads that a --full S-FSQ run starts as child processes are --full runs themselves (their lines carry parity, rooflines
and the Gowalla tail)."""
import argparse
import shutil
import sys
import types

import bench


def test_full_is_off_unless_asked(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert bench.parse().full is False
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5", "--full"])
    assert bench.parse().full is True


def test_secondary_workloads_are_full_runs(monkeypatch):
    calls = []

    def fake_run(cmd, **kw):
        calls.append(cmd)
        return types.SimpleNamespace(returncode=1, stdout="", stderr="not run")
    monkeypatch.setattr(bench.subprocess, "run", fake_run)
    monkeypatch.setattr(shutil, "which", lambda name: None)        # (no profiler pass)
    res = bench.run_sub_workloads(argparse.Namespace(seed=1, sub_steps=100))
    assert sorted(res) == ["big", "gow", "stock"] and all("error" in v for v in res.values())
    assert len(calls) == 3
    for cmd in calls:
        assert "--full" in cmd and "--no-sub" in cmd and cmd[cmd.index("--gpus") + 1] == "1"
