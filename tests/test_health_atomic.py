"""The atomic sweep in the health policy and its plumbing (none uses a GPU).
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

AT_PASS = {"outcome": "report", "report": good_report(atomic=good_matrix(rounds=4, grid_bad_cells=0))}
AT_MISCOMPARE = {"outcome": "report", "report": good_report(atomic=good_matrix(
    rounds=4, bad_waves=4, bad_kinds=16 | 512, bad_kind_names=["l_fadd", "g_fadd"], n_bad_cus=1,
    bad_cus=[0x10023], grid_bad_cells=0))}
AT_GRID = good_matrix(rounds=4, bad_kinds=1024, bad_kind_names=["g_grid"], grid_bad_cells=3)
BASE = [sys.executable, "-m", "elastic_gpu_agent_amd.isolation.health", "--probe", "3"]


@pytest.fixture
def h(tmp_path):
    harness = Harness(str(tmp_path), gpus=2)
    try:
        yield harness
    finally:
        harness.close()


def test_atomic_miscompare_is_suspect_then_unhealthy(h):
    calls = []

    def runner(index, timeout, **kw):
        calls.append((index, kw))
        return AT_MISCOMPARE if index == 0 else AT_PASS

    m = HealthMonitor(h.storage, h.operator, runner, 3600.0, atomic=True)
    out = m.run_once()
    assert out[0]["state"] == "suspect" and out[1]["state"] == "ok"
    out = m.run_once()
    rec = get_health(h.storage, 0)
    assert rec["state"] == "unhealthy" and out[0]["became_unhealthy"]
    assert rec["reason"] == "atomic: 4 bad wave(s) [l_fadd,g_fadd] on 1 CU(s)"
    assert rec["report"]["atomic"]["bad_kind_names"] == ["l_fadd", "g_fadd"]
    assert calls[:2] == [(0, {"atomic": True}), (1, {"atomic": True})]


def test_both_forms_of_the_reason_and_missing_waves():
    assert report_failures(AT_PASS["report"]) == []
    assert report_failures(good_report(atomic=AT_GRID)) == [
        "atomic: 0 bad wave(s) [g_grid] on 0 CU(s); 3 bad grid cell(s)"]
    both = dict(AT_MISCOMPARE["report"]["atomic"], bad_kind_names=["l_fadd", "g_grid"],
                grid_bad_cells=1)
    assert report_failures(good_report(cvt=good_matrix(bad_waves=1, bad_kind_names=["x16"], n_bad_cus=1),
                                       atomic=both)) == [
        "cvt: 1 bad wave(s) [x16] on 1 CU(s)",
        "atomic: 4 bad wave(s) [l_fadd,g_grid] on 1 CU(s); 1 bad grid cell(s)"]
    assert report_failures(good_report(atomic=good_matrix(waves_run=28))) == [
        "atomic: 28 of 32 waves reported"]


@pytest.mark.parametrize("kw, tail", [
    ({}, []), ({"atomic": False}, []), ({"atomic": True}, ["--atomic"]), ({"cvt": True}, ["--cvt"]),
    ({"matrix": True, "move": True, "cvt": True, "atomic": True},
     ["--matrix", "--move", "--cvt", "--atomic"]),
])
@pytest.mark.parametrize("full", [False, True])
def test_probe_argv_ends_in_atomic_only_when_on(full, kw, tail):
    assert health._probe_argv(3, full, **kw) == BASE + (["--full"] if full else []) + tail


def test_monitor_with_atomic_off_calls_a_two_argument_runner_and_stores_the_same_record(h):
    calls = []

    def old_runner(index, timeout):  # as written before the sweeps existed
        calls.append((index, timeout))
        return PASS

    m = HealthMonitor(h.storage, h.operator, old_runner, 3600.0, timeout=7.0)
    assert m.atomic is False
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
        return AT_MISCOMPARE if kw.get("atomic") else PASS

    monkeypatch.setattr(health, "subprocess_runner", fake_runner)
    db = h.storage.path
    assert egpuctl.main(["--db", db, "health", "0", "--run"]) == 0
    assert egpuctl.main(["--db", db, "health", "0", "--run", "--atomic"]) == 1
    assert egpuctl.main(["--db", db, "health", "1", "--run", "--full", "--matrix", "--move",
                         "--cvt", "--atomic"]) == 1
    assert calls == [{"full": False}, {"full": False, "atomic": True},
                     {"full": True, "matrix": True, "move": True, "cvt": True, "atomic": True}]

    opts = manager_mod.ManagerOptions
    assert opts().selftest_atomic is False
    assert opts.from_json(opts(selftest_atomic=True).to_json()).selftest_atomic is True
    seen = []
    monkeypatch.setattr(manager_mod, "GPUManager", lambda o: seen.append(o) or sys.exit(0))
    for extra in ([], ["--gpu-selftest-atomic"]):
        with pytest.raises(SystemExit):
            agent.main(["--backend", "fake", "--gpu-selftest-seconds", "600"] + extra)
    assert [o.selftest_atomic for o in seen] == [False, True]


def test_child_routes_the_injection_by_kind_name_and_runs_the_sweep_last(monkeypatch, capsys):
    calls = []

    def fake(name):
        return lambda d, seed=0, _inject=None, **kw: calls.append((name, _inject, kw)) or good_matrix()

    monkeypatch.setattr(probes, "selftest",
                        lambda d, seed=0, _inject=None, **kw: calls.append(("probe", _inject))
                        or good_report())
    monkeypatch.setattr(probes, "cvt_selftest", fake("cvt"))
    monkeypatch.setattr(probes, "atomic_selftest", fake("atomic"))
    monkeypatch.setenv(health.INJECT_ENV, "g_grid:2")
    assert health._probe_main(["--probe", "0"]) == 0  # no sweep: the name does nothing
    assert "atomic" not in json.loads(capsys.readouterr().out)
    assert health._probe_main(["--probe", "0", "--atomic"]) == 0
    assert json.loads(capsys.readouterr().out)["atomic"]["blocks"] == 1024
    assert health._probe_main(["--probe", "0", "--full", "--cvt", "--atomic"]) == 0
    assert calls == [("probe", None), ("probe", None), ("atomic", ("g_grid", 2), health.PERIODIC_ATOMIC),
                     ("probe", None), ("cvt", None, health.FULL_CVT),
                     ("atomic", ("g_grid", 2), health.FULL_ATOMIC)]
    assert "atomic" in health._REPORT_KEYS
    for sizes in (health.PERIODIC_ATOMIC, health.FULL_ATOMIC):
        assert sizes["rounds"] <= probes.ATOMIC_MAX_ROUNDS and sizes["rounds"] % 2 == 0
        assert sizes["blocks"] * sizes["rounds"] <= probes.ATOMIC_GRID_MAX_WORK


@pytest.mark.parametrize("kw, why", [
    ({"blocks": 0}, "blocks 0 outside"), ({"blocks": 65537}, "blocks 65537 outside"),
    ({"rounds": 0}, "rounds 0 outside"), ({"rounds": 65}, "rounds 65 outside"),
    ({"blocks": 4, "_inject": ("l_add", 4)}, "inject_block 4 is not a workgroup"),
    ({"blocks": 4, "_inject": ("g_grid", -1)}, "inject_block -1 is not a workgroup"),
    ({"blocks": 65536, "rounds": 16}, "blocks x rounds = 1048576 is over 699050"),
])
def test_bad_arguments_are_refused_without_a_gpu(kw, why):
    with pytest.raises(probes.ProbeError, match=why):
        probes.atomic_selftest(0, **kw)
    with pytest.raises(ValueError, match="unknown atomic kind"):
        probes.atomic_selftest(0, _inject=("enc_fp4", 0))
    with pytest.raises(probes.ProbeError, match="unknown kind"):
        probes.atomic_selftest_ops("nope")
    with pytest.raises(probes.ProbeError, match="group 4 outside"):
        probes.atomic_selftest_cells(0, "l_add", group=4)
    with pytest.raises(probes.ProbeError, match="rounds 0 outside"):
        probes.atomic_selftest_expected(0, 0)
