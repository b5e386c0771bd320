"""The move sweep in the health policy and its plumbing (none uses a GPU). With
the sweep off everything is called and judged exactly as before it existed.
"""
import json
import sys

import pytest

from elastic_gpu_agent_amd.cli import egpuctl
from elastic_gpu_agent_amd.isolation import health, probes
from elastic_gpu_agent_amd.isolation.health import HealthMonitor, get_health, report_failures

from helpers import Harness
from test_health import PASS, good_report
from test_health_matrix import good_matrix

MOVE_PASS = {"outcome": "report", "report": good_report(move=good_matrix(rounds=4))}
MOVE_MISCOMPARE = {"outcome": "report", "report": good_report(move=good_matrix(
    rounds=4, bad_waves=4, bad_kinds=16 | 32, bad_kind_names=["tr8", "tr6"], n_bad_cus=1,
    bad_cus=[0x10023]))}
BASE = [sys.executable, "-m", "elastic_gpu_agent_amd.isolation.health", "--probe", "3"]


@pytest.fixture
def h(tmp_path):
    harness = Harness(str(tmp_path), gpus=2)
    try:
        yield harness
    finally:
        harness.close()


def test_move_miscompare_is_suspect_then_unhealthy(h):
    calls = []

    def runner(index, timeout, **kw):
        calls.append((index, kw))
        return MOVE_MISCOMPARE if index == 0 else MOVE_PASS

    m = HealthMonitor(h.storage, h.operator, runner, 3600.0, move=True)
    out = m.run_once()
    assert out[0]["state"] == "suspect" and out[1]["state"] == "ok"
    out = m.run_once()
    rec = get_health(h.storage, 0)
    assert rec["state"] == "unhealthy" and out[0]["became_unhealthy"]
    assert rec["reason"] == "move: 4 bad wave(s) [tr8,tr6] on 1 CU(s)"
    assert rec["report"]["move"]["bad_kind_names"] == ["tr8", "tr6"]
    assert calls[:2] == [(0, {"move": True}), (1, {"move": True})]


def test_reasons_with_and_without_the_sub_report():
    bad = good_report(bad_waves=4, bad_kind_names=["mfma"], n_bad_cus=1)
    assert report_failures(good_report()) == []
    assert report_failures(bad) == ["4 bad wave(s) [mfma] on 1 CU(s)"]
    assert report_failures(MOVE_PASS["report"]) == []
    assert report_failures(good_report(move=good_matrix(waves_run=28))) == [
        "move: 28 of 32 waves reported"]
    both = dict(bad, matrix=good_matrix(bad_waves=1, bad_kind_names=["i8"], n_bad_cus=1),
                move=MOVE_MISCOMPARE["report"]["move"])
    assert report_failures(both) == ["4 bad wave(s) [mfma] on 1 CU(s)",
                                     "matrix: 1 bad wave(s) [i8] on 1 CU(s)",
                                     "move: 4 bad wave(s) [tr8,tr6] on 1 CU(s)"]


@pytest.mark.parametrize("kw, tail", [
    ({}, []), ({"move": False}, []), ({"move": True}, ["--move"]),
    ({"matrix": True, "move": True}, ["--matrix", "--move"]),
])
@pytest.mark.parametrize("full", [False, True])
def test_probe_argv_ends_in_move_only_when_on(full, kw, tail):
    assert health._probe_argv(3, full, **kw) == BASE + (["--full"] if full else []) + tail


def test_monitor_with_move_off_calls_a_two_argument_runner(h):
    calls = []

    def old_runner(index, timeout):  # as written before the sweeps existed
        calls.append((index, timeout))
        return PASS

    m = HealthMonitor(h.storage, h.operator, old_runner, 3600.0, timeout=7.0)
    assert m.move is False
    assert all(rec["passed"] for rec in m.run_once().values())
    assert calls == [(0, 7.0), (1, 7.0)]
    assert "move" not in get_health(h.storage, 0)["report"]


def test_egpuctl_agent_and_manager_options(h, monkeypatch):
    from elastic_gpu_agent_amd import manager as manager_mod
    from elastic_gpu_agent_amd.cli import agent

    calls = []

    def fake_runner(index, timeout, **kw):
        calls.append(kw)
        return MOVE_MISCOMPARE if kw.get("move") else PASS

    monkeypatch.setattr(health, "subprocess_runner", fake_runner)
    db = h.storage.path
    assert egpuctl.main(["--db", db, "health", "0", "--run"]) == 0
    assert egpuctl.main(["--db", db, "health", "0", "--run", "--move"]) == 1
    assert egpuctl.main(["--db", db, "health", "1", "--run", "--full", "--matrix", "--move"]) == 1
    assert calls == [{"full": False}, {"full": False, "move": True},
                     {"full": True, "matrix": True, "move": True}]

    opts = manager_mod.ManagerOptions
    assert opts().selftest_move is False
    assert opts.from_json(opts(selftest_move=True).to_json()).selftest_move is True
    seen = []
    monkeypatch.setattr(manager_mod, "GPUManager", lambda o: seen.append(o) or sys.exit(0))
    for extra in ([], ["--gpu-selftest-move"]):
        with pytest.raises(SystemExit):
            agent.main(["--backend", "fake", "--gpu-selftest-seconds", "600"] + extra)
    assert [o.selftest_move for o in seen] == [False, True]


def test_child_routes_the_injection_by_kind_name(monkeypatch, capsys):
    calls = []
    monkeypatch.setattr(probes, "selftest",
                        lambda d, seed=0, _inject=None, **kw: calls.append(("probe", _inject))
                        or good_report())
    monkeypatch.setattr(probes, "move_selftest",
                        lambda d, seed=0, _inject=None, **kw: calls.append(("move", _inject, kw))
                        or good_matrix())
    monkeypatch.setenv(health.INJECT_ENV, "tr16:2")
    assert health._probe_main(["--probe", "0"]) == 0  # no sweep: the name does nothing
    assert "move" not in json.loads(capsys.readouterr().out)
    assert health._probe_main(["--probe", "0", "--move"]) == 0
    assert json.loads(capsys.readouterr().out)["move"]["blocks"] == 1024
    assert health._probe_main(["--probe", "0", "--full", "--move"]) == 0
    assert calls == [("probe", None), ("probe", None), ("move", ("tr16", 2), health.PERIODIC_MOVE),
                     ("probe", None), ("move", ("tr16", 2), health.FULL_MOVE)]
    assert "move" in health._REPORT_KEYS
    assert health.FULL_MOVE["rounds"] <= probes.MOVE_MAX_ROUNDS
