"""Active GPU health (isolation/health.py): policy with a scripted runner,
per-GPU Unhealthy advertisement, the subprocess runner against stub children
(none uses a GPU), egpuctl, and the agent / manager wiring.
"""
from __future__ import annotations

import json
import sys
import threading

import pytest

from elastic_gpu_agent_amd import consts
from elastic_gpu_agent_amd.cli import egpuctl
from elastic_gpu_agent_amd.drain import clear_drain, set_drain
from elastic_gpu_agent_amd.isolation import health
from elastic_gpu_agent_amd.isolation.health import (
    HealthMonitor,
    apply_result,
    clear_health,
    get_health,
    list_health,
    subprocess_runner,
    unhealthy_indexes,
)
from elastic_gpu_agent_amd.protos import deviceplugin as dp
from elastic_gpu_agent_amd.protos import fastpath
from elastic_gpu_agent_amd.storage import Storage
from elastic_gpu_agent_amd.types import Device, PodContainer

from helpers import Harness


def good_report(**over):
    rep = {
        "blocks": 8, "waves_run": 32, "cus_seen": 8, "bad_waves": 0, "bad_kinds": 0,
        "bad_kind_names": [], "n_bad_cus": 0, "bad_cus": [], "lds_bytes": 32768,
        "hbm_status": "ok", "hbm_bytes_checked": 1 << 20, "hbm_miscompares": 0,
        "hbm_first_bad_offset": 0, "kernel_ms": 0.1, "hbm_ms": 0.1,
    }
    rep.update(over)
    return rep


PASS = {"outcome": "report", "report": good_report()}
MISCOMPARE = {"outcome": "report", "report": good_report(
    bad_waves=4, bad_kinds=4, bad_kind_names=["mfma"], n_bad_cus=1, bad_cus=[0x10023])}
HBM_MISCOMPARE = {"outcome": "report", "report": good_report(
    hbm_status="failed", hbm_miscompares=1, hbm_first_bad_offset=4096)}
HBM_SKIPPED = {"outcome": "report", "report": good_report(
    hbm_status="skipped", hbm_bytes_checked=0)}
TIMEOUT = {"outcome": "timeout", "reason": "no report within 1 s", "report": None}


class ScriptedRunner:
    """runner(index, timeout) answering from a per-GPU script; the last
    entry repeats. Records every call."""

    def __init__(self, script):
        self.script = {k: list(v) for k, v in script.items()}
        self.calls = []

    def __call__(self, index, timeout, full=False):
        self.calls.append(index)
        q = self.script.get(index, [PASS])
        return q.pop(0) if len(q) > 1 else q[0]


def monitor(h, runner, **kw):
    return HealthMonitor(h.storage, h.operator, runner, 3600.0, **kw)


def _health_by_gpu(devices):
    out = {}
    for d in devices:
        out.setdefault(int(d["ID"].split("-")[0]), set()).add(d["health"])
    return out


@pytest.fixture
def h(tmp_path):
    harness = Harness(str(tmp_path), gpus=2)
    yield harness
    harness.close()


# ---------------------------------------------------------------- policy

def test_no_records_leaves_advertisement_untouched(h):
    before_list = h.plugin.core.list_devices(True)
    before_groups = h.plugin.memory.device_groups(True)
    assert list_health(h.storage) == {} and unhealthy_indexes(h.storage) == set()
    assert h.plugin.core.list_devices(True) == before_list
    assert h.plugin.memory.device_groups(True) == before_groups
    assert {d["health"] for d in before_list} == {consts.HEALTHY}


def test_pass_writes_ok(h):
    r = ScriptedRunner({})
    out = monitor(h, r).run_once()
    assert r.calls == [0, 1]  # one after another, enumeration order
    assert set(out) == {0, 1}
    for idx in (0, 1):
        rec = get_health(h.storage, idx)
        assert rec["state"] == "ok" and rec["consecutive_failures"] == 0
        assert rec["reason"] == "" and rec["last_run"] >= rec["since"] > 0
        assert rec["report"]["waves_run"] == 32
    assert unhealthy_indexes(h.storage) == set()


def test_one_miscompare_is_suspect_and_stays_healthy(h):
    m = monitor(h, ScriptedRunner({0: [MISCOMPARE]}))
    m.run_once()
    rec = get_health(h.storage, 0)
    assert rec["state"] == "suspect" and rec["consecutive_failures"] == 1
    assert "mfma" in rec["reason"]
    for plugin in (h.plugin.core, h.plugin.memory):
        assert _health_by_gpu(plugin.list_devices(True)) == {
            0: {consts.HEALTHY}, 1: {consts.HEALTHY}}


def test_pass_after_suspect_resets(h):
    m = monitor(h, ScriptedRunner({0: [MISCOMPARE, PASS]}))
    m.run_once()
    m.run_once()
    rec = get_health(h.storage, 0)
    assert rec["state"] == "ok" and rec["consecutive_failures"] == 0


def test_second_miscompare_is_unhealthy_and_readvertised(h):
    changes = []
    h.plugin.cfg.options.health_refresh_seconds = 30.0

    def on_change():
        changes.append(1)
        h.plugin.core.trigger_refresh()
        h.plugin.memory.trigger_refresh()

    m = monitor(h, ScriptedRunner({0: [MISCOMPARE]}), on_change=on_change)
    watch = h.plugin.core.list_and_watch(None)
    first = next(watch)
    assert _health_by_gpu(first["devices"]) == {0: {consts.HEALTHY}, 1: {consts.HEALTHY}}
    m.run_once()
    assert changes == []
    m.run_once()
    assert changes == [1]
    assert get_health(h.storage, 0)["state"] == "unhealthy"
    assert get_health(h.storage, 0)["consecutive_failures"] == 2
    assert unhealthy_indexes(h.storage) == {0}
    # the refresh event is set: the generator yields at once, not in 30 s
    second = next(watch)
    assert second != first
    assert _health_by_gpu(second["devices"]) == {0: {consts.UNHEALTHY}, 1: {consts.HEALTHY}}
    mem = _health_by_gpu(h.plugin.memory.list_devices(True))
    assert mem == {0: {consts.UNHEALTHY}, 1: {consts.HEALTHY}}
    # every fake id of GPU 0, on both resources
    for plugin in (h.plugin.core, h.plugin.memory):
        devs = plugin.list_devices(True)
        ids0 = [d for d in devs if d["ID"].startswith("0-")]
        assert len(ids0) == len(plugin.fake_device_ids_for_gpu(h.operator.devices()[0]))
        assert all(d["health"] == consts.UNHEALTHY for d in ids0)
    watch.close()


def test_encoded_snapshot_equals_fastpath_encoding(h):
    apply_result(h.storage, 1, TIMEOUT)
    for plugin in (h.plugin.core, h.plugin.memory):
        raw = next(plugin.list_and_watch_encoded(None))
        assert raw == fastpath.encode_list_and_watch(plugin.device_groups(True))
        snap = dp.ListAndWatchResponse.decode(raw)
        assert snap["devices"] == plugin.list_devices(True)
        assert _health_by_gpu(snap["devices"]) == {
            0: {consts.HEALTHY}, 1: {consts.UNHEALTHY}}


def test_schedsim_stops_placing_on_unhealthy_gpu(h):
    from elastic_gpu_agent_amd.schedsim import SimScheduler

    sim = SimScheduler(devices=h.operator.devices(), mem_unit_mib=1024)
    m = monitor(h, ScriptedRunner({0: [MISCOMPARE]}))
    m.run_once()
    m.run_once()
    sim.sync_health(h.plugin.core, h.plugin.memory)
    for i in range(3):
        placed = sim.place(f"c{i}", core_units=30)
        assert placed is not None and placed["gpu_indexes"] == [1], placed
    assert sim.place("cx", core_units=30) is None
    clear_health(h.storage, 0)
    sim.sync_health(h.plugin.core, h.plugin.memory)
    placed = sim.place("cy", core_units=30)
    assert placed is not None and placed["gpu_indexes"] == [0]


def test_unhealthy_is_sticky_and_not_probed_again(h):
    r = ScriptedRunner({0: [MISCOMPARE, MISCOMPARE, PASS]})
    m = monitor(h, r)
    m.run_once()
    m.run_once()
    assert r.calls == [0, 1, 0, 1]
    out = m.run_once()
    assert r.calls == [0, 1, 0, 1, 1]  # GPU 0 skipped
    assert 0 not in out
    assert get_health(h.storage, 0)["state"] == "unhealthy"
    # even a pass handed to the policy directly does not heal it
    rec = apply_result(h.storage, 0, PASS)
    assert rec["state"] == "unhealthy" and not rec["became_unhealthy"]
    assert unhealthy_indexes(h.storage) == {0}


def test_state_survives_reopening_storage(tmp_path):
    h1 = Harness(str(tmp_path), gpus=2)
    try:
        apply_result(h1.storage, 0, TIMEOUT)
    finally:
        h1.close()
    h2 = Harness(str(tmp_path), gpus=2)
    try:
        assert unhealthy_indexes(h2.storage) == {0}
        r = ScriptedRunner({})
        monitor(h2, r).run_once()
        assert r.calls == [1]
        assert _health_by_gpu(h2.plugin.core.list_devices(True)) == {
            0: {consts.UNHEALTHY}, 1: {consts.HEALTHY}}
    finally:
        h2.close()


def test_clear_health_restores_healthy(h):
    before = h.plugin.core.list_devices(True)
    apply_result(h.storage, 0, TIMEOUT)
    assert h.plugin.core.list_devices(True) != before
    clear_health(h.storage, 0)
    assert h.plugin.core.list_devices(True) == before
    assert get_health(h.storage, 0) is None
    r = ScriptedRunner({})
    monitor(h, r).run_once()
    assert r.calls == [0, 1]  # probed again


@pytest.mark.parametrize("outcome", ["timeout", "crash", "unparsable"])
def test_failed_probe_is_unhealthy_at_once(h, outcome):
    changes = []
    m = monitor(h, ScriptedRunner({1: [{"outcome": outcome, "reason": "x", "report": None}]}),
                on_change=lambda: changes.append(1))
    m.run_once()
    rec = get_health(h.storage, 1)
    assert rec["state"] == "unhealthy" and outcome in rec["reason"]
    assert changes == [1]
    assert get_health(h.storage, 0)["state"] == "ok"


def test_runner_exception_counts_as_crash(h):
    def boom(index, timeout, full=False):
        raise OSError("cannot fork")

    monitor(h, boom).run_once()
    assert unhealthy_indexes(h.storage) == {0, 1}


def test_hbm_skipped_is_a_pass_and_hbm_miscompare_is_not(h):
    m = monitor(h, ScriptedRunner({0: [HBM_SKIPPED], 1: [HBM_MISCOMPARE]}))
    m.run_once()
    assert get_health(h.storage, 0)["state"] == "ok"
    assert get_health(h.storage, 0)["report"]["hbm_status"] == "skipped"
    rec = get_health(h.storage, 1)
    assert rec["state"] == "suspect" and "4096" in rec["reason"]


def test_missing_waves_count_as_failure(h):
    short = {"outcome": "report", "report": good_report(waves_run=28)}
    assert apply_result(h.storage, 0, short)["state"] == "suspect"


def test_fail_threshold_is_configurable(h):
    m = monitor(h, ScriptedRunner({0: [MISCOMPARE]}), fail_threshold=3)
    m.run_once()
    m.run_once()
    assert get_health(h.storage, 0)["state"] == "suspect"
    m.run_once()
    assert get_health(h.storage, 0)["state"] == "unhealthy"


def test_drained_and_unhealthy_compose(h):
    set_drain(h.storage, 0)
    apply_result(h.storage, 1, TIMEOUT)
    assert _health_by_gpu(h.plugin.core.list_devices(True)) == {
        0: {consts.UNHEALTHY}, 1: {consts.UNHEALTHY}}
    clear_drain(h.storage, 0)
    assert _health_by_gpu(h.plugin.core.list_devices(True)) == {
        0: {consts.HEALTHY}, 1: {consts.UNHEALTHY}}
    set_drain(h.storage, 1)
    clear_health(h.storage, 1)  # still drained
    assert _health_by_gpu(h.plugin.memory.list_devices(True)) == {
        0: {consts.HEALTHY}, 1: {consts.UNHEALTHY}}


def _bind_fractional(h, ns, name, container, gpu_index, percent):
    ids = [f"{gpu_index}-{s:02d}" for s in range(percent)]
    device = Device.new(ids, consts.RESOURCE_GPU_CORE)
    h.core_locator.assign(device.hash, PodContainer(ns, name, container))
    h.add_assumed_pod(ns, name, container, str(gpu_index))
    h.plugin.core.allocate({"container_requests": [{"devicesIDs": ids}]}, None)
    h.plugin.core.pre_start_container({"devicesIDs": ids}, None)
    return device


def test_one_event_per_live_allocation_on_the_sick_gpu(h):
    _bind_fractional(h, "ns", "a", "c", 0, 25)
    _bind_fractional(h, "ns", "b", "c", 0, 100 - 25)
    _bind_fractional(h, "ns", "other", "c", 1, 50)
    events = []
    m = monitor(h, ScriptedRunner({0: [MISCOMPARE]}),
                event_sink=lambda ns, pod, reason, msg: events.append((ns, pod, reason, msg)),
                limits=h.plugin.cfg.limits)
    m.run_once()
    assert events == []  # suspect: nobody is told yet
    m.run_once()
    assert sorted(e[:3] for e in events) == [
        ("ns", "a", "GPUSelfTestFailed"), ("ns", "b", "GPUSelfTestFailed")]
    assert all("GPU 0" in e[3] for e in events)
    m.run_once()
    assert len(events) == 2  # once per transition, not per pass


def test_broken_event_sink_does_not_stop_the_pass(h):
    _bind_fractional(h, "ns", "a", "c", 0, 25)

    def sink(*a):
        raise RuntimeError("events down")

    m = monitor(h, ScriptedRunner({0: [TIMEOUT]}), event_sink=sink,
                limits=h.plugin.cfg.limits)
    out = m.run_once()
    assert out[0]["state"] == "unhealthy" and out[1]["state"] == "ok"


def test_probe_wall_time_is_recorded(h):
    from elastic_gpu_agent_amd.metrics import GLOBAL_METRICS, GPU_SELFTEST

    before = GLOBAL_METRICS.recorder(GPU_SELFTEST).count
    monitor(h, ScriptedRunner({})).run_once()
    assert GLOBAL_METRICS.recorder(GPU_SELFTEST).count == before + 2
    assert GPU_SELFTEST == "gpu_selftest"


def test_start_stop_runs_passes_on_a_thread(h):
    seen = threading.Event()

    def runner(index, timeout, full=False):
        seen.set()
        return PASS

    m = HealthMonitor(h.storage, h.operator, runner, 0.01)
    m.start()
    assert seen.wait(5.0)
    assert m.running
    m.stop()
    assert not m.running


# ---------------------------------------------------------------- runner

def _stub(code):
    return [sys.executable, "-c", code]


def test_runner_good_json():
    r = subprocess_runner(0, 20, _argv=_stub(
        "import json; print('noise'); print(json.dumps({'bad_waves': 0, 'waves_run': 4}))"))
    assert r["outcome"] == "report"
    assert r["report"] == {"bad_waves": 0, "waves_run": 4}
    assert r["wall_s"] > 0


def test_runner_garbage_output():
    r = subprocess_runner(0, 20, _argv=_stub("print('Segmentation fault?'); print('[1, 2]')"))
    assert r["outcome"] == "unparsable" and r["report"] is None
    r = subprocess_runner(0, 20, _argv=_stub("pass"))
    assert r["outcome"] == "unparsable"


def test_runner_exit_status_1():
    r = subprocess_runner(0, 20, _argv=_stub(
        "import sys; print('{}'); print('hipErrorNoDevice', file=sys.stderr); sys.exit(1)"))
    assert r["outcome"] == "crash"
    assert "exit status 1" in r["reason"] and "hipErrorNoDevice" in r["reason"]


def test_runner_timeout_kills_the_child(tmp_path):
    pidfile = tmp_path / "pid"
    r = subprocess_runner(0, 1.0, _argv=_stub(
        f"import os, time; open({str(pidfile)!r}, 'w').write(str(os.getpid())); "
        "time.sleep(60)"))
    assert r["outcome"] == "timeout"
    assert 1.0 <= r["wall_s"] < 10.0
    pid = int(pidfile.read_text())
    import os

    with pytest.raises(ProcessLookupError):  # killed and reaped
        os.kill(pid, 0)


def test_runner_child_ended_by_signal():
    r = subprocess_runner(0, 20, _argv=_stub(
        "import os, signal; os.kill(os.getpid(), signal.SIGKILL)"))
    assert r["outcome"] == "crash" and "signal 9" in r["reason"]


def test_runner_drops_hsa_tools_lib(monkeypatch):
    monkeypatch.setenv("HSA_TOOLS_LIB", "/opt/egpu/libegpu_shim.so")
    monkeypatch.setenv("EGPU_SELFTEST_INJECT", "mfma:5")
    r = subprocess_runner(0, 20, _argv=_stub(
        "import json, os; print(json.dumps({'hsa': 'HSA_TOOLS_LIB' in os.environ, "
        "'inject': os.environ.get('EGPU_SELFTEST_INJECT'), "
        "'importable': __import__('elastic_gpu_agent_amd').__name__}))"))
    assert r["outcome"] == "report"
    assert r["report"] == {"hsa": False, "inject": "mfma:5",
                           "importable": "elastic_gpu_agent_amd"}


def test_runner_default_command_is_a_fresh_python_child():
    argv = health._probe_argv(3, full=True)
    assert argv[:3] == [sys.executable, "-m", "elastic_gpu_agent_amd.isolation.health"]
    assert argv[3:] == ["--probe", "3", "--full"]
    assert health._probe_argv(0, full=False)[3:] == ["--probe", "0"]


def test_every_runner_outcome_feeds_the_policy(tmp_path):
    st = Storage(str(tmp_path / "meta.db"))
    try:
        crash = subprocess_runner(0, 20, _argv=_stub("raise SystemExit(1)"))
        assert apply_result(st, 0, crash)["state"] == "unhealthy"
        good = subprocess_runner(1, 20, _argv=_stub(
            f"print({json.dumps(json.dumps(good_report()))})"))
        assert apply_result(st, 1, good)["state"] == "ok"
    finally:
        st.close()


def test_probe_sizes():
    p, f = health.PERIODIC_PROBE, health.FULL_PROBE
    assert p["lds_bytes"] == 32 * 1024 and 16 << 20 <= p["hbm_bytes"] <= 64 << 20
    assert f["lds_bytes"] == 163840 and f["hbm_bytes"] == 1 << 30
    assert health._parse_inject("mfma") == ("mfma", 0)
    assert health._parse_inject("hbm:4096") == ("hbm", 4096)


# ---------------------------------------------------------------- egpuctl

def test_egpuctl_health_lists_and_clears(h, capsys):
    db = h.storage.path
    assert egpuctl.main(["--db", db, "health"]) == 0
    assert json.loads(capsys.readouterr().out) == {}
    apply_result(h.storage, 1, TIMEOUT)
    apply_result(h.storage, 0, PASS)
    assert egpuctl.main(["--db", db, "health"]) == 0
    out = json.loads(capsys.readouterr().out)
    assert out["1"]["state"] == "unhealthy" and out["0"]["state"] == "ok"
    assert egpuctl.main(["--db", db, "health", "1"]) == 0
    assert json.loads(capsys.readouterr().out)["1"]["state"] == "unhealthy"
    assert egpuctl.main(["--db", db, "health", "1", "--clear"]) == 0
    capsys.readouterr()
    assert unhealthy_indexes(h.storage) == set()
    assert get_health(h.storage, 1) is None
    assert _health_by_gpu(h.plugin.core.list_devices(True))[1] == {consts.HEALTHY}
    assert egpuctl.main(["--db", db, "health", "--clear"]) == 2


def test_egpuctl_health_run_records_under_the_same_policy(h, capsys, monkeypatch):
    calls = []

    def fake_runner(index, timeout, full=False):
        calls.append((index, full))
        return MISCOMPARE

    monkeypatch.setattr(health, "subprocess_runner", fake_runner)
    db = h.storage.path
    assert egpuctl.main(["--db", db, "health", "0", "--run"]) == 1
    assert json.loads(capsys.readouterr().out)["state"] == "suspect"
    assert egpuctl.main(["--db", db, "health", "0", "--run", "--full"]) == 1
    assert json.loads(capsys.readouterr().out)["state"] == "unhealthy"
    assert calls == [(0, False), (0, True)]
    assert unhealthy_indexes(h.storage) == {0}
    monkeypatch.setattr(health, "subprocess_runner", lambda i, t, full=False: PASS)
    assert egpuctl.main(["--db", db, "health", "1", "--run"]) == 0


# ---------------------------------------------------------------- agent / manager

def test_manager_options_roundtrip_and_defaults():
    from elastic_gpu_agent_amd.manager import ManagerOptions

    d = ManagerOptions()
    assert d.selftest_seconds == 0.0 and d.selftest_timeout == health.DEFAULT_TIMEOUT_SECONDS
    o = ManagerOptions(backend="fake", selftest_seconds=900.0, selftest_timeout=25.0)
    back = ManagerOptions.from_json(o.to_json())
    assert back == o
    assert back.selftest_seconds == 900.0 and back.selftest_timeout == 25.0


def test_agent_flags_default_off(monkeypatch):
    """The parser's defaults reach ManagerOptions with the monitor off."""
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
        agent.main(["--backend", "fake"])
    assert seen["opts"].selftest_seconds == 0.0
    assert seen["opts"].selftest_timeout == health.DEFAULT_TIMEOUT_SECONDS
    with pytest.raises(StopHere):
        agent.main(["--backend", "fake", "--gpu-selftest-seconds", "600",
                    "--gpu-selftest-timeout", "30"])
    assert seen["opts"].selftest_seconds == 600.0
    assert seen["opts"].selftest_timeout == 30.0


def _manager(tmp_path, **opt_kw):
    from elastic_gpu_agent_amd.kube.locator import FakeDeviceLocator
    from elastic_gpu_agent_amd.kube.sitter import FakeSitter
    from elastic_gpu_agent_amd.manager import GPUManager, ManagerOptions
    from elastic_gpu_agent_amd.plugins.config import AgentPaths

    plugin_dir = str(tmp_path / "dp")
    (tmp_path / "dp").mkdir()
    paths = AgentPaths(
        dev_root=str(tmp_path / "dev"), plugin_dir=plugin_dir,
        kubelet_socket=str(tmp_path / "dp" / "kubelet.sock"),
        limits_dir=str(tmp_path / "limits"), limits_dir_host=None,
        state_dir=str(tmp_path), shim_host_path=None,
    )
    opts = ManagerOptions(backend="fake", db_path=str(tmp_path / "meta.db"), paths=paths,
                          **opt_kw)
    return GPUManager, opts, FakeSitter(), (FakeDeviceLocator(), FakeDeviceLocator())


def test_manager_starts_and_stops_the_monitor(tmp_path):
    seen = threading.Event()

    def runner(index, timeout, full=False):
        assert timeout == 7.0
        seen.set()
        return TIMEOUT if index == 0 else PASS

    GPUManager, opts, sitter, locators = _manager(
        tmp_path, selftest_seconds=0.01, selftest_timeout=7.0)
    mgr = GPUManager(opts, sitter=sitter, locators=locators, selftest_runner=runner)
    assert mgr.health_monitor is None  # not before run()
    mgr.run(wait_sync_timeout=5.0)
    try:
        assert mgr.health_monitor is not None and mgr.health_monitor.running
        assert seen.wait(5.0)
    finally:
        monitor_ = mgr.health_monitor
        mgr.stop()
    assert not monitor_.running


def test_manager_leaves_the_monitor_off_by_default(tmp_path):
    GPUManager, opts, sitter, locators = _manager(tmp_path)
    mgr = GPUManager(opts, sitter=sitter, locators=locators)
    mgr.run(wait_sync_timeout=5.0)
    try:
        assert mgr.health_monitor is None
    finally:
        mgr.stop()
