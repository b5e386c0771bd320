"""Active GPU health: periodic self-test, policy, and per-GPU Unhealthy state.

The agent's passive health signal is "amdsmi enumeration did not throw". This
module adds an active one: a child process runs the self-test kernels of
libegpu_kernels.so (``probes.selftest``) on one GPU and prints a report; the
policy below turns reports into a per-GPU record under the aux key
``health/<gpu>`` of the shared state DB. Both resource servers advertise every
fake device of an ``unhealthy`` GPU Unhealthy (plugins/gpushare.py), the same
way they treat an operator drain, so pre-forked workers agree without a new
channel.

Policy:

- a pass resets the record to ``ok``;
- a miscompare of any kind increments ``consecutive_failures``: ``suspect``
  below ``fail_threshold``, ``unhealthy`` once it is reached;
- a probe that times out, crashes or prints something unparsable makes the
  GPU ``unhealthy`` at once;
- ``unhealthy`` is sticky: it survives agent restarts and the GPU is not
  probed again until an operator clears the record (``egpuctl health IDX
  --clear``). No work is launched on a card that just hung or faulted, and a
  marginal card does not flap;
- ``hbm_status = skipped`` (the scratch allocation failed because tenants own
  the memory) is not a failure;
- with ``matrix`` on (off by default) the child also runs the matrix sweep
  (``probes.mx_selftest``: FP8, FP6, FP4, INT8, F16 and 16x16 MFMA paths) and
  its miscompares count like any other.

The agent process itself never initialises HIP: every probe is a fresh child
started with ``subprocess``, without ``HSA_TOOLS_LIB`` in its environment, and
killed on timeout.
"""
from __future__ import annotations

import json
import logging
import os
import subprocess
import sys
import threading
import time
from typing import Callable, Dict, List, Optional, Set

log = logging.getLogger(__name__)

AUX_HEALTH_PREFIX = "health/"

OK = "ok"
SUSPECT = "suspect"
UNHEALTHY = "unhealthy"

EVENT_REASON = "GPUSelfTestFailed"

# runner outcomes: the child produced a report, or one of the three ways it
# can fail to
OUTCOME_REPORT = "report"
OUTCOME_TIMEOUT = "timeout"
OUTCOME_CRASH = "crash"
OUTCOME_UNPARSABLE = "unparsable"

# Derived in profiles/selftest.md: worst child wall time seen x 10, rounded up
# to whole seconds, at least 10 s.
DEFAULT_TIMEOUT_SECONDS = 10.0

# Periodic probe: small, because tenants are running. 4 workgroups (16 waves)
# per CU of a 256-CU part, a quarter of one workgroup's LDS share, and a
# scratch buffer far below the Infinity Cache.
PERIODIC_PROBE = {"blocks": 1024, "rounds": 64, "lds_bytes": 32768, "hbm_bytes": 32 << 20}
# Full probe, for drained or idle GPUs: one workgroup owns the CU's whole LDS
# and the scratch buffer is four times the Infinity Cache.
FULL_PROBE = {"blocks": 1024, "rounds": 256, "lds_bytes": 163840, "hbm_bytes": 1 << 30}
# Matrix sweep (probes.mx_selftest), run after the probe above when the child
# gets --matrix. Its host reference costs 16 patterns x rounds x 3.2e5
# multiply-adds, so rounds is small (profiles/selftest.md).
PERIODIC_MATRIX = {"blocks": 1024, "rounds": 8}
FULL_MATRIX = {"blocks": 1024, "rounds": 64}

# test-only: EGPU_SELFTEST_INJECT=<kind>[:arg] in the CHILD's environment
# simulates a miscompare (kind int|fma|mfma|lds with a workgroup index, or hbm
# with a byte offset; or one of probes.MX_KINDS with a workgroup index, which
# corrupts that kind of the matrix sweep)
INJECT_ENV = "EGPU_SELFTEST_INJECT"

_REPORT_KEYS = (
    "waves_run", "cus_seen", "bad_waves", "bad_kind_names", "n_bad_cus", "bad_cus",
    "lds_bytes", "hbm_status", "hbm_bytes_checked", "hbm_miscompares",
    "hbm_first_bad_offset", "kernel_ms", "hbm_ms", "matrix",
)


# ---------------------------------------------------------------- state

def _key(gpu_index: int) -> str:
    return AUX_HEALTH_PREFIX + str(gpu_index)


def list_health(storage) -> Dict[int, dict]:
    out: Dict[int, dict] = {}
    for key, val in storage.aux_items(AUX_HEALTH_PREFIX):
        try:
            out[int(key[len(AUX_HEALTH_PREFIX):])] = json.loads(val)
        except ValueError:
            continue
    return out


def get_health(storage, gpu_index: int) -> Optional[dict]:
    raw = storage.aux_get(_key(gpu_index))
    if raw is None:
        return None
    try:
        return json.loads(raw)
    except ValueError:
        return None


def unhealthy_indexes(storage) -> Set[int]:
    return {idx for idx, rec in list_health(storage).items()
            if isinstance(rec, dict) and rec.get("state") == UNHEALTHY}


def clear_health(storage, gpu_index: int) -> None:
    storage.aux_delete(_key(gpu_index))


# ---------------------------------------------------------------- policy

def report_failures(report: dict) -> List[str]:
    """Why a report counts as a miscompare ([] = pass)."""
    why: List[str] = []
    if report.get("bad_waves", 0):
        kinds = ",".join(report.get("bad_kind_names") or []) or "?"
        why.append(f"{report['bad_waves']} bad wave(s) [{kinds}] on "
                   f"{report.get('n_bad_cus', '?')} CU(s)")
    blocks = report.get("blocks")
    if blocks is not None and report.get("waves_run") != 4 * blocks:
        why.append(f"{report.get('waves_run')} of {4 * blocks} waves reported")
    # hbm_status 'skipped' (no memory to test) and 'off' are not failures
    if report.get("hbm_miscompares", 0) or report.get("hbm_status") == "failed":
        why.append(f"{report.get('hbm_miscompares')} memory miscompare(s), first at byte "
                   f"{report.get('hbm_first_bad_offset')}")
    matrix = report.get("matrix")
    if isinstance(matrix, dict):
        if matrix.get("bad_waves", 0):
            kinds = ",".join(matrix.get("bad_kind_names") or []) or "?"
            why.append(f"matrix: {matrix['bad_waves']} bad wave(s) [{kinds}] on "
                       f"{matrix.get('n_bad_cus', '?')} CU(s)")
        blocks = matrix.get("blocks")
        if blocks is not None and matrix.get("waves_run") != 4 * blocks:
            why.append(f"matrix: {matrix.get('waves_run')} of {4 * blocks} waves reported")
    return why


def apply_result(storage, gpu_index: int, result: dict, fail_threshold: int = 2,
                 now: Optional[float] = None) -> dict:
    """Fold one runner result into the stored record. Returns the new record
    with two extra keys that are not stored: ``passed`` and ``became_unhealthy``."""
    now = int(time.time() if now is None else now)
    prev = get_health(storage, gpu_index) or {}
    prev_state = prev.get("state", OK)
    outcome = result.get("outcome")
    report = result.get("report") if isinstance(result.get("report"), dict) else None

    if outcome == OUTCOME_REPORT and report is not None:
        failures = report_failures(report)
        fatal = False
    else:
        failures = [f"probe {outcome or 'failed'}: {result.get('reason', '')}".rstrip(": ")]
        fatal = True

    if prev_state == UNHEALTHY:
        # sticky: a later pass does not heal; only an operator's clear does
        state, count, reason = UNHEALTHY, prev.get("consecutive_failures", 0), prev.get("reason", "")
    elif not failures:
        state, count, reason = OK, 0, ""
    else:
        count = int(prev.get("consecutive_failures", 0)) + 1
        reason = "; ".join(failures)
        state = UNHEALTHY if fatal or count >= fail_threshold else SUSPECT
    rec = {
        "state": state,
        "consecutive_failures": count,
        "reason": reason,
        "since": prev.get("since", now) if state == prev.get("state") else now,
        "last_run": now,
        "report": {k: report[k] for k in _REPORT_KEYS if k in report} if report else None,
    }
    storage.aux_set(_key(gpu_index), json.dumps(rec))
    return dict(rec, passed=not failures,
                became_unhealthy=state == UNHEALTHY and prev_state != UNHEALTHY)


# ---------------------------------------------------------------- runner

def _probe_argv(index: int, full: bool, matrix: bool = False) -> List[str]:
    argv = [sys.executable, "-m", "elastic_gpu_agent_amd.isolation.health",
            "--probe", str(index)]
    if full:
        argv.append("--full")
    if matrix:
        argv.append("--matrix")
    return argv


def subprocess_runner(index: int, timeout: float, full: bool = False,
                      _argv: Optional[List[str]] = None, matrix: bool = False) -> dict:
    """Runs the probe of GPU ``index`` in a fresh child and maps what happened
    to a result: {"outcome", "reason", "report", "wall_s"}. The last line of
    the child's stdout must be one JSON object."""
    env = {k: v for k, v in os.environ.items() if k != "HSA_TOOLS_LIB"}
    # the child must find this package wherever the agent was started from
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    env["PYTHONPATH"] = os.pathsep.join(p for p in (root, env.get("PYTHONPATH")) if p)
    t0 = time.monotonic()
    proc = subprocess.Popen(_argv or _probe_argv(index, full, matrix), env=env,
                            stdin=subprocess.DEVNULL, stdout=subprocess.PIPE,
                            stderr=subprocess.PIPE, text=True)

    def result(outcome, reason="", report=None):
        return {"outcome": outcome, "reason": reason, "report": report,
                "wall_s": time.monotonic() - t0}

    try:
        out, err = proc.communicate(timeout=timeout)
    except subprocess.TimeoutExpired:
        proc.kill()
        try:  # a child stuck in the driver may not die; do not wait for ever
            proc.communicate(timeout=5)
        except subprocess.TimeoutExpired:
            pass
        return result(OUTCOME_TIMEOUT, f"no report within {timeout:g} s")
    if proc.returncode != 0:
        how = (f"signal {-proc.returncode}" if proc.returncode < 0
               else f"exit status {proc.returncode}")
        tail = (err or "").strip().splitlines()[-1:] or [""]
        return result(OUTCOME_CRASH, f"{how} {tail[0][:200]}".strip())
    lines = (out or "").strip().splitlines()
    try:
        report = json.loads(lines[-1]) if lines else None
    except ValueError:
        report = None
    if not isinstance(report, dict):
        return result(OUTCOME_UNPARSABLE, f"output {(lines[-1] if lines else '')[:80]!r}")
    return result(OUTCOME_REPORT, "", report)


# ---------------------------------------------------------------- monitor

class HealthMonitor:
    """Probes every enumerated GPU, one after another, every ``interval``
    seconds and keeps the ``health/<gpu>`` records."""

    def __init__(self, storage, operator, runner: Callable = subprocess_runner,
                 interval: float = 600.0, fail_threshold: int = 2,
                 on_change: Optional[Callable[[], None]] = None, event_sink=None,
                 limits=None, timeout: float = DEFAULT_TIMEOUT_SECONDS,
                 matrix: bool = False):
        self.storage = storage
        self.operator = operator
        self.runner = runner
        self.interval = interval
        self.fail_threshold = fail_threshold
        self.on_change = on_change
        self.event_sink = event_sink
        self.limits = limits
        self.timeout = timeout
        self.matrix = matrix
        self._stop = threading.Event()
        self._probe_lock = threading.Lock()  # never two probes at once
        self._thread: Optional[threading.Thread] = None

    def run_once(self) -> Dict[int, dict]:
        """One pass over the GPUs; returns {gpu index: new record} for the
        GPUs that were probed (unhealthy ones are skipped)."""
        from ..metrics import GLOBAL_METRICS, GPU_SELFTEST

        out: Dict[int, dict] = {}
        with self._probe_lock:
            for gpu in self.operator.devices():
                if self._stop.is_set():
                    break
                idx = gpu.index
                if (get_health(self.storage, idx) or {}).get("state") == UNHEALTHY:
                    continue
                t0 = time.perf_counter()
                try:
                    # the keyword only when set: a runner written before the
                    # matrix sweep takes two arguments
                    result = (self.runner(idx, self.timeout, matrix=True) if self.matrix
                              else self.runner(idx, self.timeout))
                except Exception as e:  # a runner that cannot start a child
                    result = {"outcome": OUTCOME_CRASH, "reason": f"runner: {e}"}
                GLOBAL_METRICS.recorder(GPU_SELFTEST).observe(time.perf_counter() - t0)
                rec = apply_result(self.storage, idx, result, self.fail_threshold)
                out[idx] = rec
                if not rec["passed"]:
                    log.warning("gpu %d self-test: %s (%s)", idx, rec["state"], rec["reason"])
                if rec["became_unhealthy"]:
                    self._on_unhealthy(idx, rec)
        return out

    def _on_unhealthy(self, idx: int, rec: dict) -> None:
        if self.on_change is not None:
            try:
                self.on_change()
            except Exception as e:
                log.error("health on_change failed: %s", e)
        if self.event_sink is None:
            return
        from ..drain import live_allocations_on

        try:
            rows = live_allocations_on(self.storage, idx, self.limits)
        except Exception as e:
            log.error("health: cannot list allocations on gpu %d: %s", idx, e)
            return
        for row in rows:
            ns, _, name = row["pod"].partition("/")
            try:  # events are best-effort
                self.event_sink(ns, name, EVENT_REASON,
                                f"GPU {idx} failed its self-test and takes no new pods "
                                f"({rec['reason']}); container {row['container']} is still "
                                "bound to it")
            except Exception as e:
                log.debug("event emission failed: %s", e)

    def _loop(self) -> None:
        while not self._stop.wait(self.interval):
            try:
                self.run_once()
            except Exception as e:
                log.error("health pass failed: %s", e)

    def start(self) -> None:
        if self._thread is not None:
            return
        self._stop.clear()
        self._thread = threading.Thread(target=self._loop, name="gpu-selftest", daemon=True)
        self._thread.start()

    def stop(self) -> None:
        self._stop.set()
        t, self._thread = self._thread, None
        if t is not None:
            t.join(timeout=self.timeout + 10)

    @property
    def running(self) -> bool:
        return self._thread is not None and self._thread.is_alive()


# ---------------------------------------------------------------- child

def _parse_inject(raw: str):
    kind, _, arg = raw.partition(":")
    return (kind, int(arg) if arg else 0)


def _probe_main(argv: List[str]) -> int:
    import argparse

    p = argparse.ArgumentParser(prog="egpu-selftest-probe")
    p.add_argument("--probe", type=int, required=True, metavar="GPU")
    p.add_argument("--full", action="store_true")
    p.add_argument("--matrix", action="store_true")
    args = p.parse_args(argv)
    from . import probes

    sizes = dict(FULL_PROBE if args.full else PERIODIC_PROBE)
    inject = os.environ.get(INJECT_ENV)
    inject = _parse_inject(inject) if inject else None
    # a matrix kind's name selects the sweep, any other name the probe above
    # (without --matrix there is no sweep to corrupt and it does nothing)
    mx_inject = inject if inject and inject[0] in probes.MX_KINDS else None
    seed = int(time.time()) & 0xFFFFFFFF
    report = probes.selftest(args.probe, seed=seed,
                             _inject=None if mx_inject else inject, **sizes)
    report.update(gpu=args.probe, blocks=sizes["blocks"], rounds=sizes["rounds"], seed=seed)
    if args.matrix:
        mx_sizes = dict(FULL_MATRIX if args.full else PERIODIC_MATRIX)
        report["matrix"] = dict(
            probes.mx_selftest(args.probe, seed=seed, _inject=mx_inject, **mx_sizes), **mx_sizes)
    print(json.dumps(report), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(_probe_main(sys.argv[1:]))
