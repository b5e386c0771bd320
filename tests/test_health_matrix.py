"""The matrix sweep in the health policy and its plumbing (none uses a GPU):
report_failures, the probe argv, the monitor's runner call, egpuctl, the
manager option and the agent flag. With the sweep off everything is called and
judged exactly as before it existed.
"""
from __future__ import annotations

import json
import sys

import pytest

from elastic_gpu_agent_amd.cli import egpuctl
from elastic_gpu_agent_amd.isolation import health, probes
from elastic_gpu_agent_amd.isolation.health import HealthMonitor, get_health, report_failures

from helpers import Harness
from test_health import PASS, good_report


def good_matrix(**over):
    rep = {
        "version": 1, "blocks": 8, "rounds": 8, "waves_run": 32, "cus_seen": 8, "bad_waves": 0,
        "bad_kinds": 0, "bad_kind_names": [], "n_bad_cus": 0, "bad_cus": [], "kernel_ms": 0.1,
    }
    rep.update(over)
    return rep


MATRIX_PASS = {"outcome": "report", "report": good_report(matrix=good_matrix())}
MATRIX_MISCOMPARE = {"outcome": "report", "report": good_report(matrix=good_matrix(
    bad_waves=4, bad_kinds=128 | 256, bad_kind_names=["mxfp4", "mxmix"], n_bad_cus=1,
    bad_cus=[0x10023]))}


@pytest.fixture
def h(tmp_path):
    harness = Harness(str(tmp_path), gpus=2)
    try:
        yield harness
    finally:
        harness.close()


def test_report_without_matrix_is_judged_as_before():
    assert report_failures(good_report()) == []
    bad = good_report(bad_waves=4, bad_kind_names=["mfma"], n_bad_cus=1)
    assert report_failures(bad) == ["4 bad wave(s) [mfma] on 1 CU(s)"]
    assert report_failures(good_report(matrix=good_matrix())) == []
    # a sweep's verdict is added to the probe's, it does not replace it
    both = dict(bad, matrix=MATRIX_MISCOMPARE["report"]["matrix"])
    assert report_failures(both) == ["4 bad wave(s) [mfma] on 1 CU(s)",
                                     "matrix: 4 bad wave(s) [mxfp4,mxmix] on 1 CU(s)"]


def test_matrix_miscompare_is_suspect_then_unhealthy(h):
    calls = []

    def runner(index, timeout, full=False, matrix=False):
        calls.append((index, matrix))
        return MATRIX_MISCOMPARE if index == 0 else MATRIX_PASS

    m = HealthMonitor(h.storage, h.operator, runner, 3600.0, matrix=True)
    out = m.run_once()
    assert out[0]["state"] == "suspect" and not out[0]["passed"]
    assert out[1]["state"] == "ok" and out[1]["passed"]
    out = m.run_once()
    rec = get_health(h.storage, 0)
    assert rec["state"] == "unhealthy" and out[0]["became_unhealthy"]
    assert rec["reason"] == "matrix: 4 bad wave(s) [mxfp4,mxmix] on 1 CU(s)"
    # the stored report keeps the sweep's sub-report
    assert rec["report"]["matrix"]["bad_kind_names"] == ["mxfp4", "mxmix"]
    assert get_health(h.storage, 1)["report"]["matrix"]["bad_waves"] == 0
    assert calls[:2] == [(0, True), (1, True)]


def test_missing_matrix_waves_fail():
    rep = good_report(matrix=good_matrix(waves_run=28))
    assert report_failures(rep) == ["matrix: 28 of 32 waves reported"]
    rep = good_report(matrix=good_matrix(waves_run=0))
    assert report_failures(rep) == ["matrix: 0 of 32 waves reported"]


def test_probe_argv_appends_matrix_last():
    base = [sys.executable, "-m", "elastic_gpu_agent_amd.isolation.health", "--probe", "3"]
    assert health._probe_argv(3, False) == base
    assert health._probe_argv(3, False, matrix=False) == base
    assert health._probe_argv(3, True) == base + ["--full"]
    assert health._probe_argv(3, False, matrix=True) == base + ["--matrix"]
    assert health._probe_argv(3, True, matrix=True) == base + ["--full", "--matrix"]


def test_runner_passes_matrix_to_the_child(monkeypatch):
    seen = []

    class Done(Exception):
        pass

    def fake_popen(argv, **kw):
        seen.append(argv)
        raise Done

    monkeypatch.setattr(health.subprocess, "Popen", fake_popen)
    for kw in ({}, {"matrix": True}, {"full": True, "matrix": True}):
        with pytest.raises(Done):
            health.subprocess_runner(0, 1.0, **kw)
    assert [a[5:] for a in seen] == [[], ["--matrix"], ["--full", "--matrix"]]


def test_monitor_with_matrix_off_calls_a_two_argument_runner(h):
    calls = []

    def old_runner(index, timeout):  # as written before the sweep existed
        calls.append((index, timeout))
        return PASS

    m = HealthMonitor(h.storage, h.operator, old_runner, 3600.0, timeout=7.0)
    assert m.matrix is False
    out = m.run_once()
    assert calls == [(0, 7.0), (1, 7.0)]
    assert all(rec["passed"] for rec in out.values())
    assert "matrix" not in get_health(h.storage, 0)["report"]


def test_monitor_with_matrix_on_passes_the_keyword(h):
    calls = []

    def runner(index, timeout, **kw):
        calls.append((index, kw))
        return MATRIX_PASS

    HealthMonitor(h.storage, h.operator, runner, 3600.0, matrix=True).run_once()
    assert calls == [(0, {"matrix": True}), (1, {"matrix": True})]


def test_egpuctl_matrix_is_passed_through(h, capsys, monkeypatch):
    calls = []

    def fake_runner(index, timeout, **kw):
        calls.append((index, kw))
        return MATRIX_MISCOMPARE if kw.get("matrix") else PASS

    monkeypatch.setattr(health, "subprocess_runner", fake_runner)
    db = h.storage.path
    assert egpuctl.main(["--db", db, "health", "0", "--run"]) == 0
    capsys.readouterr()
    assert egpuctl.main(["--db", db, "health", "0", "--run", "--matrix"]) == 1
    out = json.loads(capsys.readouterr().out)
    assert out["state"] == "suspect" and "mxfp4" in out["reason"]
    assert egpuctl.main(["--db", db, "health", "1", "--run", "--full", "--matrix"]) == 1
    # the keyword only when the flag is given
    assert calls == [(0, {"full": False}), (0, {"full": False, "matrix": True}),
                     (1, {"full": True, "matrix": True})]


def test_manager_options_roundtrip_and_default():
    from elastic_gpu_agent_amd.manager import ManagerOptions

    assert ManagerOptions().selftest_matrix is False
    o = ManagerOptions(backend="fake", selftest_seconds=900.0, selftest_matrix=True)
    back = ManagerOptions.from_json(o.to_json())
    assert back == o and back.selftest_matrix is True
    assert ManagerOptions.from_json(ManagerOptions().to_json()).selftest_matrix is False


def test_agent_flag_defaults_off_and_reaches_the_options(monkeypatch):
    from elastic_gpu_agent_amd import manager as manager_mod
    from elastic_gpu_agent_amd.cli import agent

    seen = {}

    class StopHere(Exception):
        pass

    def fake_manager(opts):
        seen["opts"] = opts
        raise StopHere

    monkeypatch.setattr(manager_mod, "GPUManager", fake_manager)
    with pytest.raises(StopHere):
        agent.main(["--backend", "fake", "--gpu-selftest-seconds", "600"])
    assert seen["opts"].selftest_matrix is False
    with pytest.raises(StopHere):
        agent.main(["--backend", "fake", "--gpu-selftest-seconds", "600",
                    "--gpu-selftest-matrix"])
    assert seen["opts"].selftest_matrix is True and seen["opts"].selftest_seconds == 600.0


def test_manager_hands_the_option_to_the_monitor(tmp_path):
    from test_health import _manager

    GPUManager, opts, sitter, locators = _manager(
        tmp_path, selftest_seconds=3600.0, selftest_matrix=True)
    mgr = GPUManager(opts, sitter=sitter, locators=locators,
                     selftest_runner=lambda index, timeout, **kw: MATRIX_PASS)
    mgr.run(wait_sync_timeout=5.0)
    try:
        assert mgr.health_monitor is not None and mgr.health_monitor.matrix is True
    finally:
        mgr.stop()


def test_probe_sizes_and_report_key():
    assert health.PERIODIC_MATRIX == {"blocks": 1024, "rounds": 8}
    assert health.FULL_MATRIX == {"blocks": 1024, "rounds": 64}
    assert health.FULL_MATRIX["rounds"] <= probes.MX_MAX_ROUNDS
    assert "matrix" in health._REPORT_KEYS


def test_child_routes_the_injection_by_kind_name(monkeypatch, capsys):
    """EGPU_SELFTEST_INJECT=<matrix kind> goes to the sweep, any other name to
    the probe before it; without --matrix the child's output has no sweep."""
    calls = []

    def fake_selftest(device, seed=0, _inject=None, **sizes):
        calls.append(("probe", _inject))
        return good_report()

    def fake_mx(device, seed=0, _inject=None, **sizes):
        calls.append(("matrix", _inject, sizes))
        return good_matrix()

    monkeypatch.setattr(probes, "selftest", fake_selftest)
    monkeypatch.setattr(probes, "mx_selftest", fake_mx)
    monkeypatch.delenv(health.INJECT_ENV, raising=False)
    assert health._probe_main(["--probe", "0"]) == 0
    assert "matrix" not in json.loads(capsys.readouterr().out)
    assert calls == [("probe", None)]

    del calls[:]
    monkeypatch.setenv(health.INJECT_ENV, "mxfp4:3")
    assert health._probe_main(["--probe", "0", "--matrix"]) == 0
    out = json.loads(capsys.readouterr().out)
    assert out["matrix"]["blocks"] == 1024 and out["matrix"]["rounds"] == 8
    assert calls == [("probe", None), ("matrix", ("mxfp4", 3), health.PERIODIC_MATRIX)]

    del calls[:]
    monkeypatch.setenv(health.INJECT_ENV, "mfma")
    assert health._probe_main(["--probe", "0", "--full", "--matrix"]) == 0
    assert json.loads(capsys.readouterr().out)["matrix"]["rounds"] == 64
    assert calls == [("probe", ("mfma", 0)), ("matrix", None, health.FULL_MATRIX)]
