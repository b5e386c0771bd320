"""GPUShare device plugins: `elasticgpu.io/gpu-core` and `gpu-memory`.

Re-design of the reference's two gRPC servers (ref: pkg/plugins/gpushare.go)
with the MI355X-native differences:

- fake devices carry kubelet TopologyInfo (NUMA node of the GPU);
- Allocate answers **per container** (the reference merged all containers
  into one response — SURVEY §3.3 quirk, not copied);
- Allocate's DeviceSpecs grant /dev/kfd plus the per-allocation symlink
  (whose resolution by the container runtime whitelists the underlying
  /dev/dri/renderD* major:minor in the device cgroup);
- fractional core allocations mount the HSA shim + a limits file and set
  HSA_TOOLS_LIB so CU masks / HBM quotas are enforced in-container;
- GetPreferredAllocation is implemented (xGMI/NUMA-aware packing) where the
  reference stubs it (pkg/plugins/base.go:94-96).
"""
from __future__ import annotations

import logging
import math
import threading
from typing import List

from .. import consts, topology
from ..kube.client import NotFound
from ..types import Device
from .config import GPUPluginConfig

log = logging.getLogger(__name__)


class GPUSharePluginBase:
    """Handlers shared by the core and memory resource servers."""

    resource_name: str = ""

    def __init__(self, config: GPUPluginConfig):
        self.cfg = config
        self._devices_lock = threading.Lock()
        self._refresh = threading.Event()

    # ---- device advertisement ----
    def fake_device_ids_for_gpu(self, gpu) -> List[str]:
        raise NotImplementedError

    def _drained(self) -> set:
        """GPUs under an operator drain (egpuctl drain): advertised Unhealthy
        so kubelet stops placing pods while existing ones finish."""
        if self.cfg.storage is None:
            return set()
        from ..drain import drained_indexes

        try:
            return drained_indexes(self.cfg.storage)
        except Exception as e:  # a broken flag read must not kill ListAndWatch
            log.error("drain flags unreadable: %s", e)
            return set()

    def _unschedulable(self) -> set:
        """GPUs advertised Unhealthy one by one: operator drains, and GPUs
        whose self-test record is `unhealthy` (isolation/health.py)."""
        out = self._drained()
        if self.cfg.storage is None:
            return out
        from ..isolation.health import unhealthy_indexes

        try:
            return out | unhealthy_indexes(self.cfg.storage)
        except Exception as e:  # as with drains: never kill ListAndWatch
            log.error("health records unreadable: %s", e)
            return out

    def list_devices(self, healthy: bool = True) -> List[dict]:
        drained = self._unschedulable()
        out = []
        for gpu in self.cfg.operator.devices():
            health = (
                consts.HEALTHY
                if healthy and gpu.index not in drained
                else consts.UNHEALTHY
            )
            topo = {"nodes": [{"ID": gpu.numa_node}]}
            for did in self.fake_device_ids_for_gpu(gpu):
                out.append({"ID": did, "health": health, "topology": topo})
        return out

    def device_groups(self, healthy: bool = True) -> List[tuple]:
        """[(ids, encoded Device suffix)] per GPU — the fast-encode shape."""
        from ..protos import fastpath

        drained = self._unschedulable()
        groups = []
        for gpu in self.cfg.operator.devices():
            health = (
                consts.HEALTHY
                if healthy and gpu.index not in drained
                else consts.UNHEALTHY
            )
            suffix = fastpath.device_suffix(health, gpu.numa_node)
            groups.append((self.fake_device_ids_for_gpu(gpu), suffix))
        return groups

    # ---- gRPC handlers ----
    def get_device_plugin_options(self, request, context) -> dict:
        return {"pre_start_required": True, "get_preferred_allocation_available": True}

    UNHEALTHY_AFTER_FAILURES = 3

    def _watch_snapshots(self, context, snap_fn):
        """Initial snapshot + re-advertisement when enumeration changes.

        Unlike the reference (single static send, devices never re-checked —
        SURVEY §3.2), the backend is re-enumerated periodically: a GPU
        falling off the bus shrinks the advertised list, and when enumeration
        itself keeps failing (driver wedged, amdsmi gone) every device is
        re-advertised Unhealthy so kubelet stops placing pods here."""
        current = snap_fn(True)
        yield current
        interval = self.cfg.options.health_refresh_seconds
        failures = 0
        while context is None or context.is_active():
            triggered = self._refresh.wait(timeout=interval)
            self._refresh.clear()
            if context is not None and not context.is_active():
                return
            try:
                self.cfg.operator.devices(refresh=True)
                recovered = failures >= self.UNHEALTHY_AFTER_FAILURES
                failures = 0
            except Exception as e:
                failures += 1
                log.error("device re-enumeration failed (%d): %s", failures, e)
                if failures == self.UNHEALTHY_AFTER_FAILURES:
                    current = snap_fn(False)
                    yield current
                continue
            fresh = snap_fn(True)
            if fresh != current or recovered:
                current = fresh
                yield current
            elif triggered:
                yield current

    def list_and_watch(self, context):
        yield from self._watch_snapshots(
            context, lambda healthy: {"devices": self.list_devices(healthy)}
        )

    def list_and_watch_encoded(self, context):
        """Server path: pre-encoded ListAndWatchResponse bytes (cached until
        enumeration changes; at 1-MiB memory units a snapshot is ~7 MB per
        GPU and must not be re-encoded per send)."""
        from ..protos import fastpath

        yield from self._watch_snapshots(
            context,
            lambda healthy: fastpath.encode_list_and_watch(self.device_groups(healthy)),
        )

    def trigger_refresh(self) -> None:
        self._refresh.set()

    def get_preferred_allocation(self, request, context) -> dict:
        devices = self.cfg.operator.devices()
        responses = []
        for cr in request.get("container_requests", []):
            size = cr.get("allocation_size", 0)
            # memory allocations and fractional core requests bind to exactly
            # one physical GPU at PreStart — never prefer a spanning set
            single = (
                self.resource_name == consts.RESOURCE_GPU_MEMORY
                or size <= consts.GPU_PERCENT_EACH_CARD
            )
            counts = cr.get("counts")
            if counts is not None and single and not cr.get("must_include_deviceIDs"):
                # digest fast path: choose the GPU from per-GPU counts alone
                # (same ranking as prefer_allocation's single-GPU branch:
                # most-loaded GPU that fits, tie-broken by index), then have
                # C++ extract that GPU's first `size` IDs as pre-encoded
                # response bytes — the ~295k-ID pool at 1-MiB memory units
                # is never materialized in Python.
                from ..protos import fastpath

                pick = None
                for g in sorted((g for g in counts if g >= 0),
                                key=lambda g: (counts[g], g)):
                    if counts[g] >= size:
                        pick = g
                        break
                if pick is None:
                    responses.append({"deviceIDs": []})
                else:
                    responses.append({
                        "raw": fastpath.extract_preferred(
                            cr["_raw"], cr["_index"], pick, size)
                    })
                continue
            avail = cr.get("available_deviceIDs")
            if avail is None and "_raw" in cr:
                # digest-decoded request but the generic policy is needed
                # (must_include present, or a multi-GPU core request)
                from ..protos import deviceplugin as dp

                full = dp.PreferredAllocationRequest.decode(cr["_raw"])
                avail = full["container_requests"][cr["_index"]].get(
                    "available_deviceIDs", [])
            picked = topology.prefer_allocation(
                avail or [],
                cr.get("must_include_deviceIDs", []),
                size,
                devices,
                single_gpu=single,
            )
            responses.append({"deviceIDs": picked})
        return {"container_responses": responses}

    def allocate(self, request, context) -> dict:
        responses = []
        for cr in request.get("container_requests", []):
            # server fast path supplies (hash, count) straight off the wire
            # (fastpath.decode_allocate_request_digest); explicit ID lists
            # (tests, in-process callers) are hashed here instead
            digest = cr.get("digest")
            if digest is None:
                ids = cr.get("devicesIDs", [])
                digest = (Device.new(ids, self.resource_name).hash, len(ids))
            responses.append(self._allocate_one(digest[0], digest[1]))
        return {"container_responses": responses}

    def _allocate_one(self, alloc_hash: str, n_units: int) -> dict:
        raise NotImplementedError

    def _isolation_payload(self, alloc_hash: str, kind: str) -> dict:
        """Common shim env + mounts for a fractional allocation."""
        paths = self.cfg.paths
        resp: dict = {"envs": {}, "mounts": []}
        if not (self.cfg.options.isolation and self.cfg.limits and paths.shim_host_path):
            return resp
        # NOTE: the limits file itself is written at PreStart (before the
        # container is created); Allocate only declares the mount — with the
        # HOST-view path (kubelet resolves host_path on the host, not through
        # the agent's /host mount). Keeps the Allocate hot path free of disk
        # I/O (p50 latency is the headline).
        import os as _os

        limits_host = paths.limits_host_view(
            _os.path.basename(self.cfg.limits.host_path(alloc_hash)))
        resp["mounts"] = [
            {
                "container_path": paths.shim_container_path,
                "host_path": paths.shim_host_path,
                "read_only": True,
            },
            {
                "container_path": self.cfg.limits.container_path(kind),
                "host_path": limits_host,
                "read_only": True,
            },
        ]
        resp["envs"] = {"HSA_TOOLS_LIB": paths.shim_container_path}
        return resp

    def pre_start_container(self, request, context) -> dict:
        ids = request.get("devicesIDs", [])
        h8 = request.get("device_hash")
        if h8 is not None and "list_runs" in request:
            # digest3: a large consecutive set as ID runs; its literal list
            # is never built on the hot path
            device = Device.from_runs(h8, request["device_count"],
                                      request["list_runs"], self.resource_name)
        elif h8 is not None and "list_json" in request:
            # digest2: hash + count + pre-serialized sorted list (no Python
            # string materialization on the hot path)
            device = Device.from_digest(h8, request["device_count"],
                                        request["list_json"], self.resource_name)
        elif h8 is not None:  # digest deserializer: ids pre-sorted, hash ready
            device = Device(hash=h8, list=tuple(ids), resource_name=self.resource_name)
        else:
            device = Device.new(ids, self.resource_name)
        from .. import egrpc

        try:
            pc = self._locator().locate(device)
        except (KeyError, egrpc.EgrpcError) as e:
            # unknown device set, or podresources outage (clean failure —
            # kubelet will retry the container start)
            return self._fail(context, f"locate {device.hash}: {e}")
        try:
            pod = self.cfg.sitter.get_pod(pc.namespace, pc.name)
        except NotFound:
            try:
                pod = self.cfg.sitter.get_pod_from_api_server(pc.namespace, pc.name)
            except NotFound:
                return self._fail(context, f"pod {pc.pod()} not found")
        if not pod.is_assumed():
            return self._fail(
                context, f"pod {pc.pod()} lacks {consts.ELASTIC_GPU_ASSUMED_ANNOTATION}=true"
            )
        raw = pod.container_gpu_indexes(pc.container)
        if raw is None:
            return self._fail(
                context,
                f"pod {pc.pod()} lacks annotation for container {pc.container}",
            )
        try:
            indexes = [int(x) for x in raw.split(",") if x != ""]
        except ValueError:
            return self._fail(context, f"bad GPU index annotation {raw!r}")
        created: List[str] = []
        try:
            self._bind(device, indexes, created, pod)
            # persistence is part of the same atomic contract: a record-less
            # binding would leave symlinks/masks GC can never reclaim (GC
            # reconciles FROM storage), so a failed save rolls the whole
            # binding back and kubelet's retry starts clean
            pi = self.cfg.storage.load_or_create(pc.namespace, pc.name)
            pi.container_device_map[pc.container] = device
            self.cfg.storage.save(pi)
        except Exception as e:
            for alloc_id in created:  # rollback partial symlinks
                self.cfg.operator.delete(-1, alloc_id)
            if self.cfg.cumask is not None:
                try:
                    self.cfg.cumask.release(device.hash)
                except Exception:
                    pass
            if self.cfg.limits is not None:
                self.cfg.limits.delete(device.hash)
            self._emit_event(pc, "EgpuBindFailed", f"bind {device.hash}: {e}")
            return self._fail(context, f"bind {device.hash}: {e}")
        return {}

    def _bind(self, device: Device, indexes: List[int], created: List[str],
              pod=None):
        raise NotImplementedError

    def _locator(self):
        raise NotImplementedError

    def _emit_event(self, pc, reason, message):
        sink = self.cfg.event_sink
        if sink is None:
            return
        try:
            sink(pc.namespace, pc.name, reason, message)
        except Exception as e:  # events are best-effort
            log.debug("event emission failed: %s", e)

    @staticmethod
    def _fail(context, msg):
        log.error("%s", msg)
        if context is not None:
            from .. import egrpc

            context.abort(egrpc.INVALID_ARGUMENT, msg)
        raise RuntimeError(msg)


class GPUShareCorePlugin(GPUSharePluginBase):
    """100 percent-unit fake devices per GPU; fractional pods get CU masks."""

    resource_name = consts.RESOURCE_GPU_CORE

    def fake_device_ids_for_gpu(self, gpu) -> List[str]:
        return [f"{gpu.index}-{slot:02d}" for slot in range(consts.GPU_PERCENT_EACH_CARD)]

    @staticmethod
    def links_for(ids_count: int) -> int:
        """Number of per-allocation GPU links: one per started 100 units."""
        return max(1, math.ceil(ids_count / consts.GPU_PERCENT_EACH_CARD))

    def _allocate_one(self, alloc_hash: str, n_units: int) -> dict:
        n_links = self.links_for(n_units)
        devices_spec = [
            {"container_path": consts.KFD_PATH, "host_path": consts.KFD_PATH,
             "permissions": "rw"}
        ]
        for i in range(n_links):
            host = f"/dev/{consts.ELASTIC_GPU_LINK_FMT % (alloc_hash + '-' + str(i))}"
            devices_spec.append(
                {
                    "container_path": f"/dev/egpu/gpu{i}",
                    "host_path": host,
                    "permissions": "rw",
                }
            )
        resp = {
            "envs": {consts.GPU_ENV_KEY: alloc_hash},
            "devices": devices_spec,
        }
        fractional = n_units < consts.GPU_PERCENT_EACH_CARD
        if fractional:
            iso = self._isolation_payload(alloc_hash, "core")
            resp["envs"].update(iso["envs"])
            resp["mounts"] = iso["mounts"]
        return resp

    def _bind(self, device: Device, indexes: List[int], created: List[str],
              pod=None):
        n_links = self.links_for(device.n_ids)
        if len(indexes) != n_links:
            raise ValueError(
                f"annotation has {len(indexes)} GPU indexes, expected {n_links}"
            )
        for i, idx in enumerate(indexes):
            alloc_id = f"{device.hash}-{i}"
            self.cfg.operator.create(idx, alloc_id)
            created.append(alloc_id)
        percent = device.n_ids
        priority = pod.qos_class() if pod is not None else None
        if percent < consts.GPU_PERCENT_EACH_CARD and self.cfg.cumask and self.cfg.limits:
            mask_hex, n_cus = self.cfg.cumask.allocate(
                device.hash, indexes[0], percent, priority=priority)
            self.cfg.limits.finalize(
                device.hash,
                gpu_indexes=indexes,
                devices=self.cfg.operator.devices(),
                cu_mask=mask_hex,
                cu_count=n_cus,
                priority=priority,
            )
        elif self.cfg.limits:
            self.cfg.limits.finalize(
                device.hash, gpu_indexes=indexes, devices=self.cfg.operator.devices(),
                priority=priority,
            )

    def _locator(self):
        return self.cfg.core_locator


class GPUShareMemoryPlugin(GPUSharePluginBase):
    """One fake device per mem_unit_mib MiB of HBM3E (288 GiB per MI355X).

    The unit defaults to 1 MiB (reference contract). On 288 GB parts that is
    294,912 device IDs per GPU; deployments that hit kubelet scaling limits
    can set --mem-unit-mib=1024 (documented deviation, same resource name)."""

    resource_name = consts.RESOURCE_GPU_MEMORY

    def fake_device_ids_for_gpu(self, gpu) -> List[str]:
        unit = self.cfg.options.mem_unit_mib
        count = gpu.memory_mib // unit
        return [f"{gpu.index}-{slot:06d}" for slot in range(count)]

    def _allocate_one(self, alloc_hash: str, n_units: int) -> dict:
        host = f"/dev/{consts.ELASTIC_GPU_LINK_FMT % (alloc_hash + '-0')}"
        resp = {
            "envs": {consts.GPU_ENV_KEY: alloc_hash},
            "devices": [
                {"container_path": consts.KFD_PATH, "host_path": consts.KFD_PATH,
                 "permissions": "rw"},
                {"container_path": "/dev/egpu/gpu0", "host_path": host, "permissions": "rw"},
            ],
        }
        iso = self._isolation_payload(alloc_hash, "mem")
        resp["envs"].update(iso["envs"])
        if iso["mounts"]:
            resp["mounts"] = iso["mounts"]
        return resp

    def _bind(self, device: Device, indexes: List[int], created: List[str],
              pod=None):
        if len(indexes) != 1:
            raise ValueError(f"memory binding expects exactly 1 GPU index, got {indexes}")
        alloc_id = f"{device.hash}-0"
        self.cfg.operator.create(indexes[0], alloc_id)
        created.append(alloc_id)
        if self.cfg.limits:
            mem_bytes = device.n_ids * self.cfg.options.mem_unit_mib * 1024 * 1024
            self.cfg.limits.finalize(
                device.hash,
                gpu_indexes=indexes,
                devices=self.cfg.operator.devices(),
                mem_limit_bytes=mem_bytes,
                priority=pod.qos_class() if pod is not None else None,
            )

    def _locator(self):
        return self.cfg.memory_locator
