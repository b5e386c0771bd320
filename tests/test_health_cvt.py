"""The conversion sweep in the health policy and its plumbing (none uses a GPU).
With the sweep off everything is called and judged exactly as before it existed.
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

CVT_PASS = {"outcome": "report", "report": good_report(cvt=good_matrix(rounds=4))}
CVT_MISCOMPARE = {"outcome": "report", "report": good_report(cvt=good_matrix(
    rounds=4, bad_waves=4, bad_kinds=16 | 1024, bad_kind_names=["enc_fp4", "x16"], n_bad_cus=1,
    bad_cus=[0x10023]))}
BASE = [sys.executable, "-m", "elastic_gpu_agent_amd.isolation.health", "--probe", "3"]


@pytest.fixture
def h(tmp_path):
    harness = Harness(str(tmp_path), gpus=2)
    try:
        yield harness
    finally:
        harness.close()


def test_cvt_miscompare_is_suspect_then_unhealthy(h):
    calls = []

    def runner(index, timeout, **kw):
        calls.append((index, kw))
        return CVT_MISCOMPARE if index == 0 else CVT_PASS

    m = HealthMonitor(h.storage, h.operator, runner, 3600.0, cvt=True)
    out = m.run_once()
    assert out[0]["state"] == "suspect" and out[1]["state"] == "ok"
    out = m.run_once()
    rec = get_health(h.storage, 0)
    assert rec["state"] == "unhealthy" and out[0]["became_unhealthy"]
    assert rec["reason"] == "cvt: 4 bad wave(s) [enc_fp4,x16] on 1 CU(s)"
    assert rec["report"]["cvt"]["bad_kind_names"] == ["enc_fp4", "x16"]
    assert calls[:2] == [(0, {"cvt": True}), (1, {"cvt": True})]


def test_reasons_missing_waves_and_all_three_sweeps():
    assert report_failures(CVT_PASS["report"]) == []
    assert report_failures(good_report(cvt=good_matrix(waves_run=28))) == [
        "cvt: 28 of 32 waves reported"]
    bad = good_report(bad_waves=4, bad_kind_names=["mfma"], n_bad_cus=1)
    every = dict(bad, matrix=good_matrix(bad_waves=1, bad_kind_names=["i8"], n_bad_cus=1),
                 move=good_matrix(bad_waves=2, bad_kind_names=["tr8"], n_bad_cus=1),
                 cvt=CVT_MISCOMPARE["report"]["cvt"])
    assert report_failures(every) == ["4 bad wave(s) [mfma] on 1 CU(s)",
                                      "matrix: 1 bad wave(s) [i8] on 1 CU(s)",
                                      "move: 2 bad wave(s) [tr8] on 1 CU(s)",
                                      "cvt: 4 bad wave(s) [enc_fp4,x16] on 1 CU(s)"]


@pytest.mark.parametrize("kw, tail", [
    ({}, []), ({"cvt": False}, []), ({"cvt": True}, ["--cvt"]), ({"move": True}, ["--move"]),
    ({"matrix": True, "move": True, "cvt": True}, ["--matrix", "--move", "--cvt"]),
])
@pytest.mark.parametrize("full", [False, True])
def test_probe_argv_ends_in_cvt_only_when_on(full, kw, tail):
    assert health._probe_argv(3, full, **kw) == BASE + (["--full"] if full else []) + tail


def test_monitor_with_cvt_off_calls_a_two_argument_runner_and_stores_the_same_record(h):
    calls = []

    def old_runner(index, timeout):  # as written before the sweeps existed
        calls.append((index, timeout))
        return PASS

    m = HealthMonitor(h.storage, h.operator, old_runner, 3600.0, timeout=7.0)
    assert m.cvt is False
    assert all(rec["passed"] for rec in m.run_once().values())
    assert calls == [(0, 7.0), (1, 7.0)]
    assert get_health(h.storage, 0)["report"] == {
        k: v for k, v in PASS["report"].items() if k in health._REPORT_KEYS}


def test_egpuctl_agent_and_manager_options(h, monkeypatch):
    from elastic_gpu_agent_amd import manager as manager_mod
    from elastic_gpu_agent_amd.cli import agent

    calls = []

    def fake_runner(index, timeout, **kw):
        calls.append(kw)
        return CVT_MISCOMPARE if kw.get("cvt") else PASS

    monkeypatch.setattr(health, "subprocess_runner", fake_runner)
    db = h.storage.path
    assert egpuctl.main(["--db", db, "health", "0", "--run"]) == 0
    assert egpuctl.main(["--db", db, "health", "0", "--run", "--cvt"]) == 1
    assert egpuctl.main(["--db", db, "health", "1", "--run", "--full", "--matrix", "--move",
                         "--cvt"]) == 1
    assert calls == [{"full": False}, {"full": False, "cvt": True},
                     {"full": True, "matrix": True, "move": True, "cvt": True}]

    opts = manager_mod.ManagerOptions
    assert opts().selftest_cvt is False
    assert opts.from_json(opts(selftest_cvt=True).to_json()).selftest_cvt is True
    seen = []
    monkeypatch.setattr(manager_mod, "GPUManager", lambda o: seen.append(o) or sys.exit(0))
    for extra in ([], ["--gpu-selftest-cvt"]):
        with pytest.raises(SystemExit):
            agent.main(["--backend", "fake", "--gpu-selftest-seconds", "600"] + extra)
    assert [o.selftest_cvt for o in seen] == [False, True]


def test_child_routes_the_injection_by_kind_name_and_runs_the_sweep_last(monkeypatch, capsys):
    calls = []

    def fake(name):
        return lambda d, seed=0, _inject=None, **kw: calls.append((name, _inject, kw)) or good_matrix()

    monkeypatch.setattr(probes, "selftest",
                        lambda d, seed=0, _inject=None, **kw: calls.append(("probe", _inject))
                        or good_report())
    monkeypatch.setattr(probes, "move_selftest", fake("move"))
    monkeypatch.setattr(probes, "cvt_selftest", fake("cvt"))
    monkeypatch.setenv(health.INJECT_ENV, "enc_fp4:2")
    assert health._probe_main(["--probe", "0"]) == 0  # no sweep: the name does nothing
    assert "cvt" not in json.loads(capsys.readouterr().out)
    assert health._probe_main(["--probe", "0", "--cvt"]) == 0
    assert json.loads(capsys.readouterr().out)["cvt"]["blocks"] == 1024
    assert health._probe_main(["--probe", "0", "--full", "--move", "--cvt"]) == 0
    assert calls == [("probe", None), ("probe", None), ("cvt", ("enc_fp4", 2), health.PERIODIC_CVT),
                     ("probe", None), ("move", None, health.FULL_MOVE),
                     ("cvt", ("enc_fp4", 2), health.FULL_CVT)]
    assert "cvt" in health._REPORT_KEYS
    assert health.FULL_CVT["rounds"] <= probes.CVT_MAX_ROUNDS
