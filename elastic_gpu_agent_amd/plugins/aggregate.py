"""GPUShare plugin aggregate: both resource servers + GC + Restore.

Role of the reference's GPUSharePlugin (ref: pkg/plugins/base.go:203-306)
with two additions: GC also reclaims CU masks and limits files, and
Restore() — declared but never implemented in the reference
(pkg/manager/manager.go:20) — re-creates per-allocation device links from
the persisted state after a node reboot wiped /host/dev.
"""
from __future__ import annotations

import logging
import queue
import threading
from typing import List

from .. import consts
from ..kube.client import NotFound
from ..operator import unlink_many
from ..types import PodInfo
from .base import DevicePluginServer
from .config import GPUPluginConfig
from .gpushare import GPUShareCorePlugin, GPUShareMemoryPlugin

log = logging.getLogger(__name__)

GC_PERIOD_SECONDS = 60.0


def _malloc_trim() -> None:
    """Return glibc's freed-but-retained heap pages to the kernel.

    Under sustained RPC churn across threads, glibc keeps freed chunks
    resident (bins/fragmentation; MALLOC_ARENA_MAX-insensitive) — measured
    ~0.3-1 KB per pod cycle of RSS creep, fully reclaimed by malloc_trim
    (soak plateaus flat with this in the GC cadence; see docs/TESTING.md)."""
    try:
        import ctypes

        ctypes.CDLL("libc.so.6").malloc_trim(0)
    except Exception:  # non-glibc platforms: harmless to skip
        pass


class GPUSharePlugin:
    def __init__(self, config: GPUPluginConfig):
        self.cfg = config
        self.core = GPUShareCorePlugin(config)
        self.memory = GPUShareMemoryPlugin(config)
        self.core_server = DevicePluginServer(
            self.core,
            consts.RESOURCE_GPU_CORE,
            consts.CORE_SOCK_NAME,
            plugin_dir=config.paths.plugin_dir,
            kubelet_socket=config.paths.kubelet_socket,
        )
        self.memory_server = DevicePluginServer(
            self.memory,
            consts.RESOURCE_GPU_MEMORY,
            consts.MEMORY_SOCK_NAME,
            plugin_dir=config.paths.plugin_dir,
            kubelet_socket=config.paths.kubelet_socket,
        )
        self._stop = threading.Event()

    # ---- lifecycle ----
    def run(self) -> None:
        self.core_server.start()
        self.memory_server.start()

    def stop(self) -> None:
        self._stop.set()
        self.core_server.stop()
        self.memory_server.stop()
        # wake any ListAndWatch watcher generators blocked on the refresh
        # event so their threads exit now rather than at the next interval
        self.core.trigger_refresh()
        self.memory.trigger_refresh()

    # ---- GC ----
    def gc_once(self) -> int:
        """Reconcile storage against live pods; returns records reclaimed.

        Runs off the pod-summary rows (hash/count/resource per container),
        never parsing full records — at the 1-MiB contract unit a loaded
        node's records total tens of MB and a full-parse GC pass would stall
        concurrent PreStarts on the storage lock."""
        doomed: List[tuple] = []  # (ns, name, summary)
        cache_missing: List[tuple] = []

        def visit(ns: str, name: str, summary: dict):
            try:
                self.cfg.sitter.get_pod(ns, name)
            except NotFound:
                cache_missing.append((ns, name, summary))

        self.cfg.storage.for_each_summary(visit)
        if cache_missing:
            # ONE bulk LIST confirms every candidate (per-record API GETs
            # thundering-herd the API server during mass deletions); any API
            # failure keeps all records — reclaim only on confirmed absence
            api_keys = None
            try:
                api_keys = self.cfg.sitter.api_pod_keys()
            except NotImplementedError:
                api_keys = None
            except Exception as e:
                log.warning("GC: bulk API list failed, keeping %d records: %s",
                            len(cache_missing), e)
                cache_missing = []
            if api_keys is not None:
                doomed = [(ns, name, s) for ns, name, s in cache_missing
                          if f"{ns}/{name}" not in api_keys]
            else:
                # sitter without bulk support: per-record fallback
                for ns, name, summary in cache_missing:
                    try:
                        self.cfg.sitter.get_pod_from_api_server(ns, name)
                    except NotFound:
                        doomed.append((ns, name, summary))
                    except Exception as e:
                        log.warning("GC: API check failed for %s/%s: %s",
                                    ns, name, e)
        import os

        aux_keys = []
        # the links, limits files and pid files of the whole pass go in one
        # unlink_many call instead of one Python try/unlink each
        must_go: List[str] = []  # an error other than ENOENT fails the pass
        pid_files: List[str] = []  # best effort
        for ns, name, summary in doomed:
            for container, dev in summary.items():
                dhash, n_ids, resource = dev["h"], dev["n"], dev["r"]
                links = (
                    GPUShareCorePlugin.links_for(n_ids)
                    if resource == consts.RESOURCE_GPU_CORE
                    else 1
                )
                for i in range(links):
                    must_go.extend(self.cfg.operator.link_paths(f"{dhash}-{i}"))
                if self.cfg.cumask:
                    aux_keys.append("mask/" + dhash)
                if self.cfg.limits:
                    must_go.append(self.cfg.limits.host_path(dhash))
                # hook-recorded pid file (occupancy attribution)
                pid_files.append(
                    os.path.join(self.cfg.paths.state_dir, "pids", dhash))
        try:
            unlink_many(must_go + pid_files)
        except OSError as e:
            # as before the batch: a link or limits file that will not go
            # stops the pass, a pid file does not (those come last, so an
            # error on one means nothing before it failed)
            if e.filename not in pid_files:
                raise
        # storage work batched: one transaction per GC pass, not per pod
        # (per-pod autocommit deletes fall behind at high churn)
        if self.cfg.cumask:
            self.cfg.cumask.release_many(k[len("mask/"):] for k in aux_keys)
        else:
            self.cfg.storage.aux_delete_many(aux_keys)
        self.cfg.storage.delete_many(f"{ns}/{name}" for ns, name, _ in doomed)
        # WAL checkpoint here (not on the binding hot path): autocheckpoint
        # is raised so a 700 KB/record workload doesn't rewrite the DB
        # mid-PreStart; the GC cadence folds the WAL back instead
        checkpoint = getattr(self.cfg.storage, "checkpoint", None)
        if checkpoint is not None:
            checkpoint()
        for ns, name, _ in doomed:
            log.info("GC reclaimed %s/%s", ns, name)
        return len(doomed)

    def gc_loop(self, gc_events: "queue.Queue", period: float = GC_PERIOD_SECONDS) -> None:
        """Event-driven + periodic reconciliation (ref: pkg/plugins/base.go:241-306)."""
        while not self._stop.is_set():
            try:
                gc_events.get(timeout=period)
                while True:  # coalesce bursts of delete events into one pass
                    try:
                        gc_events.get_nowait()
                    except queue.Empty:
                        break
            except queue.Empty:
                pass
            try:
                self.gc_once()
            except Exception as e:
                log.error("GC pass failed: %s", e)
            _malloc_trim()

    # ---- Restore ----
    def restore(self) -> int:
        """Re-create device links for pods that still exist (node reboot path).
        Returns number of allocations restored."""
        restored = 0
        records: List[PodInfo] = []
        self.cfg.storage.for_each(records.append)
        for pi in records:
            try:
                pod = self.cfg.sitter.get_pod(pi.namespace, pi.name)
            except NotFound:
                try:
                    pod = self.cfg.sitter.get_pod_from_api_server(pi.namespace, pi.name)
                except Exception:
                    continue  # GC will reclaim
            for container, device in pi.container_device_map.items():
                raw = pod.container_gpu_indexes(container)
                if raw is None:
                    continue
                try:
                    indexes = [int(x) for x in raw.split(",") if x != ""]
                except ValueError:
                    continue
                links = (
                    GPUShareCorePlugin.links_for(device.n_ids)
                    if device.resource_name == consts.RESOURCE_GPU_CORE
                    else 1
                )
                for i, idx in enumerate(indexes[:links]):
                    alloc_id = f"{device.hash}-{i}"
                    if not self.cfg.operator.check(idx, alloc_id):
                        self.cfg.operator.create(idx, alloc_id)
                        restored += 1
        return restored
