"""GPU manager: wires clients, storage, sitter, isolation and the plugin.

Role of the reference's GPUManager (ref: pkg/manager/manager.go:17-156),
with Run/GC/Restore all actually implemented (the reference declares GC and
Restore on the interface but never defines them — SURVEY §1.C).
"""
from __future__ import annotations

import logging
import os
import queue
import threading
from dataclasses import dataclass, field
from typing import Optional

from . import consts
from .isolation import CUMaskAllocator, LimitsWriter
from .kube.locator import KubeletDeviceLocator
from .kube.sitter import FakeSitter, PodSitter
from .operator import GPUOperator
from .operator.fake import FakeBackend
from .plugins.aggregate import GPUSharePlugin
from .plugins.config import AgentPaths, GPUPluginConfig, PluginOptions

log = logging.getLogger(__name__)


@dataclass
class ManagerOptions:
    node_name: str = ""
    db_path: str = "/host/var/lib/egpu/meta.db"
    kubeconf: Optional[str] = None
    gpu_plugin_name: str = "gpushare"
    backend: str = "amdsmi"  # "amdsmi" | "fake"
    paths: AgentPaths = field(default_factory=AgentPaths)
    plugin_options: PluginOptions = field(default_factory=PluginOptions)
    metrics_port: int = 0
    # pre-forked data plane: N worker processes accept on the plugin
    # sockets (kernel load-balancing); 0 = serve in-process. The parent
    # keeps registration, fsnotify watching, GC, Restore and drains.
    workers: int = 0
    # active GPU self-test (isolation/health.py): seconds between passes over
    # the GPUs, 0 = off; and the time limit of one probe child
    selftest_seconds: float = 0.0
    selftest_timeout: float = 10.0
    # each probe also runs the matrix sweep (probes.mx_selftest)
    selftest_matrix: bool = False
    # how the store's rows hold a large consecutive device set: "runs"
    # (ID runs) or "list" (the reference-format record; the way back for a
    # rollback to a build that cannot read runs)
    record_format: str = "runs"
    # entry cap of the native Allocate -> PreStart hash memo (0 = off); each
    # process, pre-forked workers included, keeps its own
    hash_memo_entries: int = 256

    def to_json(self) -> str:
        import dataclasses
        import json

        return json.dumps(dataclasses.asdict(self))

    @staticmethod
    def from_json(raw: str) -> "ManagerOptions":
        import json

        obj = json.loads(raw)
        paths = AgentPaths(**obj.pop("paths"))
        popts = PluginOptions(**obj.pop("plugin_options"))
        return ManagerOptions(paths=paths, plugin_options=popts, **obj)


class GPUManager:
    def __init__(self, opts: ManagerOptions, sitter=None, locators=None, storage=None,
                 selftest_runner=None):
        if opts.gpu_plugin_name != "gpushare":
            raise ValueError(f"unsupported plugin {opts.gpu_plugin_name!r} (only 'gpushare')")
        self.opts = opts

        from .protos import fastpath
        from .storage import new_storage

        fastpath.hash_memo_configure(opts.hash_memo_entries)

        self.storage = storage or new_storage(opts.db_path, opts.record_format)

        if opts.backend == "fake":
            backend = FakeBackend()
        elif opts.backend == "amdsmi":
            from .operator.amdsmi import AmdSmiBackend

            backend = AmdSmiBackend()
        else:
            raise ValueError(f"unknown backend {opts.backend!r}")
        self.operator = GPUOperator(backend, dev_root=opts.paths.dev_root)

        self.gc_events: "queue.Queue" = queue.Queue()
        if sitter is not None:
            self.sitter = sitter
            if isinstance(sitter, FakeSitter):
                sitter.set_delete_hook(self._on_pod_delete)
        else:
            from .kube.client import K8sClient

            client = K8sClient(kubeconf=opts.kubeconf)
            self.sitter = PodSitter(client, opts.node_name, delete_hook=self._on_pod_delete)
            self._event_client = client

        if locators is not None:
            core_loc, mem_loc = locators
        else:
            core_loc = KubeletDeviceLocator(
                consts.RESOURCE_GPU_CORE, opts.paths.podresources_socket
            )
            mem_loc = KubeletDeviceLocator(
                consts.RESOURCE_GPU_MEMORY, opts.paths.podresources_socket
            )

        limits = LimitsWriter(opts.paths.limits_dir)
        # on_remask: when QoS preemption shrinks (or later re-expands) a live
        # allocation's CU mask, rewrite its limits file in place — the shim's
        # watcher inside the victim container re-applies the mask to live
        # queues within its poll interval
        _remask = lambda h, mask, n: limits.update_in_place(  # noqa: E731
            h, cu_mask=mask, cu_count=n)
        if opts.workers > 0:
            # pre-forked data plane: mask state must be coherent across the
            # worker processes AND this parent's GC — coordinate through the
            # shared state DB (flock'd transactions)
            from .isolation import DbCUMaskAllocator

            cumask = DbCUMaskAllocator(
                opts.db_path, self.operator.devices(), on_remask=_remask)
        else:
            cumask = CUMaskAllocator(
                self.storage, self.operator.devices(), on_remask=_remask)

        event_sink = None
        client = getattr(self, "_event_client", None)
        if client is not None:
            def event_sink(ns, pod, reason, message, _c=client):
                try:
                    p = self.sitter.get_pod(ns, pod)
                    uid = p.uid
                except Exception:
                    uid = ""
                _c.create_event(ns, pod, uid, reason, message)

        self.config = GPUPluginConfig(
            operator=self.operator,
            storage=self.storage,
            sitter=self.sitter,
            core_locator=core_loc,
            memory_locator=mem_loc,
            paths=opts.paths,
            options=opts.plugin_options,
            limits=limits,
            cumask=cumask,
            event_sink=event_sink,
        )
        self.plugin = GPUSharePlugin(self.config)
        self._gc_thread: Optional[threading.Thread] = None
        self._selftest_runner = selftest_runner
        self.health_monitor = None

    def _on_pod_delete(self, pod) -> None:
        # only pods the scheduler assumed can hold allocations
        # (timer-driven GC still covers everything — ref: base.go:245-247)
        self.gc_events.put(pod)

    def run(self, wait_sync_timeout: float = 60.0) -> None:
        self.sitter.start()
        import time

        deadline = time.time() + wait_sync_timeout
        while not self.sitter.has_synced():
            if time.time() > deadline:
                raise TimeoutError("pod informer did not sync")
            time.sleep(0.1)
        restored = self.plugin.restore()
        if restored:
            log.info("restored %d device links from persisted state", restored)
        if self.opts.workers > 0:
            self._spawn_workers()
        self.plugin.run()
        self._gc_thread = threading.Thread(
            target=self.plugin.gc_loop, args=(self.gc_events,), name="gc", daemon=True
        )
        self._gc_thread.start()
        if self.opts.metrics_port:
            from .metrics import GLOBAL_METRICS

            GLOBAL_METRICS.serve_prometheus(self.opts.metrics_port)
        if self.opts.selftest_seconds > 0:
            self._start_health_monitor()

    def _start_health_monitor(self) -> None:
        """Parent only (agent workers never call run()): one monitor per
        node, its verdicts reach the workers through the shared state DB."""
        from .isolation.health import HealthMonitor, subprocess_runner

        def refresh():
            self.plugin.core.trigger_refresh()
            self.plugin.memory.trigger_refresh()

        self.health_monitor = HealthMonitor(
            self.storage, self.operator,
            self._selftest_runner or subprocess_runner,
            self.opts.selftest_seconds,
            on_change=refresh,
            event_sink=self.config.event_sink,
            limits=self.config.limits,
            timeout=self.opts.selftest_timeout,
            matrix=self.opts.selftest_matrix,
        )
        self.health_monitor.start()

    def _spawn_one_worker(self, core_fd: int, mem_fd: int):
        import subprocess
        import sys as _sys

        return subprocess.Popen(
            [_sys.executable, "-m", "elastic_gpu_agent_amd.cli.agent_worker",
             str(core_fd), str(mem_fd)],
            env={**os.environ, "EGPU_WORKER_OPTS": self.opts.to_json()},
            pass_fds=(core_fd, mem_fd),
        )

    def _spawn_workers(self) -> None:
        """Pre-forked data plane: bind both plugin sockets here (the parent
        keeps registration/watching), then launch opts.workers agent-worker
        processes that accept on the inherited fds. A supervisor thread
        respawns any worker that dies (a crashed worker must not silently
        shrink — or, at workers=1, eliminate — the data plane)."""
        core_fd = self.plugin.core_server.bind_listener()
        mem_fd = self.plugin.memory_server.bind_listener()
        self._worker_procs = [self._spawn_one_worker(core_fd, mem_fd)
                              for _ in range(self.opts.workers)]
        self._worker_stop = threading.Event()

        def supervise():
            import time as _time

            while not self._worker_stop.is_set():
                _time.sleep(1.0)
                for i, p in enumerate(self._worker_procs):
                    rc = p.poll()
                    if rc is not None and not self._worker_stop.is_set():
                        log.error("data-plane worker %d died rc=%s; respawning",
                                  i, rc)
                        self._worker_procs[i] = self._spawn_one_worker(
                            core_fd, mem_fd)

        threading.Thread(target=supervise, name="worker-supervisor",
                         daemon=True).start()
        log.info("spawned %d data-plane workers", len(self._worker_procs))

    def gc(self) -> int:
        return self.plugin.gc_once()

    def restore(self) -> int:
        return self.plugin.restore()

    def stop(self) -> None:
        if self.health_monitor is not None:
            self.health_monitor.stop()
        ws = getattr(self, "_worker_stop", None)
        if ws is not None:
            ws.set()
        for p in getattr(self, "_worker_procs", []):
            p.terminate()
        for p in getattr(self, "_worker_procs", []):
            try:
                p.wait(timeout=10)
            except Exception:
                p.kill()
        self.plugin.stop()
        self.sitter.stop()
        self.storage.close()
