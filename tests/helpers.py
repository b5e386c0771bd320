"""Test harness: an in-process agent wired to fakes + gRPC client helpers."""
from __future__ import annotations

import os
import threading
from concurrent import futures
from dataclasses import dataclass, field
from typing import List, Optional

import grpc

from elastic_gpu_agent_amd import consts
from elastic_gpu_agent_amd.isolation import CUMaskAllocator, LimitsWriter
from elastic_gpu_agent_amd.kube.locator import FakeDeviceLocator
from elastic_gpu_agent_amd.kube.pods import Pod
from elastic_gpu_agent_amd.kube.sitter import FakeSitter
from elastic_gpu_agent_amd.operator import GPUOperator
from elastic_gpu_agent_amd.operator.fake import FakeBackend
from elastic_gpu_agent_amd.plugins.aggregate import GPUSharePlugin
from elastic_gpu_agent_amd.plugins.config import AgentPaths, GPUPluginConfig, PluginOptions
from elastic_gpu_agent_amd.protos import deviceplugin as dp
from elastic_gpu_agent_amd.storage import Storage


# sockaddr_un.sun_path holds 107 bytes + NUL. The longest path the harness
# hangs off its root is device-plugins/elastic-gpushare-memory.sock (43) and
# tests add a sub-directory level of their own; roots up to this length
# always fit.
SOCKET_ROOT_MAX = 56


def short_tmp_base(prefix: str = "egpu-") -> str:
    """The temp directory in which mkdtemp(prefix=prefix) leaves room for the
    agent's unix sockets: $TMPDIR unless it is too deeply nested, then a
    short world-writable one."""
    import tempfile

    base = tempfile.gettempdir()
    if len(base) + 1 + len(prefix) + 8 > SOCKET_ROOT_MAX:
        for cand in ("/tmp", "/var/tmp", "/dev/shm"):
            if os.path.isdir(cand) and os.access(cand, os.W_OK | os.X_OK):
                return cand
    return base


def short_tmpdir(prefix: str = "egpu-") -> str:
    """mkdtemp() under short_tmp_base(). The caller removes the directory."""
    import tempfile

    return tempfile.mkdtemp(prefix=prefix, dir=short_tmp_base(prefix))


@dataclass
class Harness:
    tmp: str
    gpus: int = 2
    mem_unit_mib: int = 1024  # keep fake-device counts small in tests
    storage: Storage = None
    operator: GPUOperator = None
    sitter: FakeSitter = None
    core_locator: FakeDeviceLocator = None
    mem_locator: FakeDeviceLocator = None
    plugin: GPUSharePlugin = None
    paths: AgentPaths = None

    def __post_init__(self):
        dev_root = os.path.join(self.tmp, "dev")
        limits_dir = os.path.join(self.tmp, "limits")
        plugin_dir = os.path.join(self.tmp, "device-plugins")
        os.makedirs(plugin_dir, exist_ok=True)
        self.storage = Storage(os.path.join(self.tmp, "meta.db"))
        self.operator = GPUOperator(FakeBackend(count=self.gpus), dev_root=dev_root)
        self.sitter = FakeSitter()
        self.core_locator = FakeDeviceLocator()
        self.mem_locator = FakeDeviceLocator()
        self.paths = AgentPaths(
            dev_root=dev_root,
            plugin_dir=plugin_dir,
            kubelet_socket=os.path.join(plugin_dir, "kubelet.sock"),
            limits_dir=limits_dir,
            limits_dir_host=None,  # tests: agent view == host view
            shim_host_path=os.path.join(self.tmp, "libegpu_shim.so"),
        )
        cfg = GPUPluginConfig(
            operator=self.operator,
            storage=self.storage,
            sitter=self.sitter,
            core_locator=self.core_locator,
            memory_locator=self.mem_locator,
            paths=self.paths,
            options=PluginOptions(mem_unit_mib=self.mem_unit_mib),
            limits=LimitsWriter(limits_dir),
            cumask=None,
        )
        cfg.cumask = CUMaskAllocator(
            self.storage, self.operator.devices(),
            on_remask=lambda h, mask, n: cfg.limits.update_in_place(
                h, cu_mask=mask, cu_count=n),
        )
        self.plugin = GPUSharePlugin(cfg)

    def close(self):
        self.plugin.stop()
        self.storage.close()

    # -- scenario helpers --
    def add_assumed_pod(self, ns, name, container, gpu_indexes: str):
        pod = Pod(
            namespace=ns,
            name=name,
            annotations={
                consts.ELASTIC_GPU_ASSUMED_ANNOTATION: "true",
                consts.ELASTIC_GPU_CONTAINER_ANNOTATION % container: gpu_indexes,
            },
        )
        self.sitter.add(pod)
        return pod


class PluginClient:
    """egrpc client speaking the device-plugin API to a served socket.
    (GrpcioPluginClient below drives the same socket with the real gRPC
    stack for interop coverage.)"""

    def __init__(self, socket_path: str):
        from elastic_gpu_agent_amd import egrpc
        from elastic_gpu_agent_amd.protos import fastpath

        self.channel = egrpc.Channel(socket_path)
        mk = self.channel.unary_unary
        self.get_options = mk(
            dp.METHOD_GET_OPTIONS,
            request_serializer=dp.Empty.encode,
            response_deserializer=dp.DevicePluginOptions.decode,
        )
        self.allocate = mk(
            dp.METHOD_ALLOCATE,
            request_serializer=fastpath.encode_allocate_request,
            response_deserializer=dp.AllocateResponse.decode,
        )
        self.pre_start = mk(
            dp.METHOD_PRE_START_CONTAINER,
            request_serializer=fastpath.encode_prestart_request,
            response_deserializer=dp.PreStartContainerResponse.decode,
        )
        # raw-bytes variants for pre-encoded load generation (bench.py)
        self.allocate_raw = mk(
            dp.METHOD_ALLOCATE,
            response_deserializer=dp.AllocateResponse.decode,
        )
        self.pre_start_raw = mk(
            dp.METHOD_PRE_START_CONTAINER,
            response_deserializer=dp.PreStartContainerResponse.decode,
        )
        self.preferred = mk(
            dp.METHOD_GET_PREFERRED_ALLOCATION,
            request_serializer=dp.PreferredAllocationRequest.encode,
            response_deserializer=dp.PreferredAllocationResponse.decode,
        )
        self.list_and_watch = self.channel.unary_stream(
            dp.METHOD_LIST_AND_WATCH,
            request_serializer=dp.Empty.encode,
            response_deserializer=dp.ListAndWatchResponse.decode,
        )

    def close(self):
        self.channel.close()


class GrpcioPluginClient(PluginClient):
    """Same surface via grpcio — the 'real kubelet stack' direction."""

    def __init__(self, socket_path: str):
        self.channel = grpc.insecure_channel(f"unix://{socket_path}")
        mk = self.channel.unary_unary
        self.get_options = mk(
            dp.METHOD_GET_OPTIONS,
            request_serializer=dp.Empty.encode,
            response_deserializer=dp.DevicePluginOptions.decode,
        )
        self.allocate = mk(
            dp.METHOD_ALLOCATE,
            request_serializer=dp.AllocateRequest.encode,
            response_deserializer=dp.AllocateResponse.decode,
        )
        self.pre_start = mk(
            dp.METHOD_PRE_START_CONTAINER,
            request_serializer=dp.PreStartContainerRequest.encode,
            response_deserializer=dp.PreStartContainerResponse.decode,
        )
        self.preferred = mk(
            dp.METHOD_GET_PREFERRED_ALLOCATION,
            request_serializer=dp.PreferredAllocationRequest.encode,
            response_deserializer=dp.PreferredAllocationResponse.decode,
        )
        self.list_and_watch = self.channel.unary_stream(
            dp.METHOD_LIST_AND_WATCH,
            request_serializer=dp.Empty.encode,
            response_deserializer=dp.ListAndWatchResponse.decode,
        )


class FakeKubeletRegistration:
    """Records device-plugin Register calls (stand-in kubelet.sock server)."""

    def __init__(self, socket_path: str):
        self.requests: List[dict] = []
        self._event = threading.Event()
        handler = grpc.method_handlers_generic_handler(
            dp.REGISTRATION_SERVICE,
            {
                "Register": grpc.unary_unary_rpc_method_handler(
                    self._register,
                    request_deserializer=dp.RegisterRequest.decode,
                    response_serializer=dp.Empty.encode,
                )
            },
        )
        self.server = grpc.server(futures.ThreadPoolExecutor(max_workers=2))
        self.server.add_generic_rpc_handlers((handler,))
        self.server.add_insecure_port(f"unix://{socket_path}")

    def _register(self, request, context):
        self.requests.append(request)
        self._event.set()
        return {}

    def wait_for_register(self, n=1, timeout=10.0) -> bool:
        import time

        deadline = time.time() + timeout
        while len(self.requests) < n and time.time() < deadline:
            time.sleep(0.05)
        return len(self.requests) >= n

    def start(self):
        self.server.start()

    def stop(self):
        self.server.stop(grace=0.2)


# ---- file-backed fakes: kubelet-side state shared across forked workers ----
# (production workers use the REAL podresources locator and API-watch sitter,
# which are process-safe by nature; these exist for the bench/tests where the
# kubelet side is simulated and must be visible to pre-forked agent workers)

class FileDeviceLocator:
    """hash→PodContainer table as one file per hash under a shared dir."""

    def __init__(self, root: str):
        self.root = root
        os.makedirs(root, exist_ok=True)

    def assign(self, device_hash: str, pc) -> None:
        tmpf = os.path.join(self.root, f".{device_hash}.tmp")
        with open(tmpf, "w") as f:
            f.write(f"{pc.namespace}\n{pc.name}\n{pc.container}\n")
        os.replace(tmpf, os.path.join(self.root, device_hash))

    def locate(self, device):
        from elastic_gpu_agent_amd.types import PodContainer

        try:
            with open(os.path.join(self.root, device.hash)) as f:
                ns, name, container = f.read().splitlines()[:3]
        except FileNotFoundError:
            raise KeyError(f"no assignment for {device.hash}")
        return PodContainer(ns, name, container)


class FileSitter:
    """Pod objects as JSON files under a shared dir (annotations only)."""

    def __init__(self, root: str):
        import json as _json

        self.root = root
        self._json = _json
        os.makedirs(root, exist_ok=True)

    def _path(self, ns, name):
        return os.path.join(self.root, f"{ns}__{name}.json")

    def add(self, pod) -> None:
        p = self._path(pod.namespace, pod.name)
        with open(p + ".tmp", "w") as f:
            self._json.dump({"namespace": pod.namespace, "name": pod.name,
                             "uid": getattr(pod, "uid", ""),
                             "annotations": pod.annotations}, f)
        os.replace(p + ".tmp", p)

    def remove(self, namespace: str, name: str) -> None:
        try:
            os.unlink(self._path(namespace, name))
        except FileNotFoundError:
            pass

    def get_pod(self, namespace: str, name: str):
        from elastic_gpu_agent_amd.kube.client import NotFound
        from elastic_gpu_agent_amd.kube.pods import Pod

        try:
            with open(self._path(namespace, name)) as f:
                obj = self._json.load(f)
        except FileNotFoundError:
            raise NotFound(f"{namespace}/{name}")
        return Pod(namespace=obj["namespace"], name=obj["name"],
                   uid=obj.get("uid", ""), annotations=obj.get("annotations", {}))

    def get_pod_from_api_server(self, namespace: str, name: str):
        return self.get_pod(namespace, name)

    def api_pod_keys(self):
        out = set()
        for fn in os.listdir(self.root):
            if fn.endswith(".json"):
                ns, _, name = fn[:-5].partition("__")
                out.add(f"{ns}/{name}")
        return out

    def set_delete_hook(self, hook) -> None:
        pass

    def start(self) -> None:
        pass

    def has_synced(self) -> bool:
        return True


def build_worker_harness(tmp: str, gpus: int, mem_unit_mib: int, backend=None):
    """Plugin stack for ONE pre-forked worker process: private Storage
    connection on the shared DB, DB-coordinated CU-mask allocator, and the
    file-backed kubelet-side fakes under the shared tmp dir."""
    from elastic_gpu_agent_amd.isolation import DbCUMaskAllocator

    dev_root = os.path.join(tmp, "dev")
    limits_dir = os.path.join(tmp, "limits")
    plugin_dir = os.path.join(tmp, "device-plugins")
    os.makedirs(plugin_dir, exist_ok=True)
    db_path = os.path.join(tmp, "meta.db")
    storage = Storage(db_path)
    operator = GPUOperator(backend or FakeBackend(count=gpus), dev_root=dev_root)
    sitter = FileSitter(os.path.join(tmp, "podstate"))
    core_locator = FileDeviceLocator(os.path.join(tmp, "assign-core"))
    mem_locator = FileDeviceLocator(os.path.join(tmp, "assign-mem"))
    paths = AgentPaths(
        dev_root=dev_root,
        plugin_dir=plugin_dir,
        kubelet_socket=os.path.join(plugin_dir, "kubelet.sock"),
        limits_dir=limits_dir,
        limits_dir_host=None,
        shim_host_path=os.path.join(tmp, "libegpu_shim.so"),
    )
    limits = LimitsWriter(limits_dir)
    cfg = GPUPluginConfig(
        operator=operator,
        storage=storage,
        sitter=sitter,
        core_locator=core_locator,
        memory_locator=mem_locator,
        paths=paths,
        options=PluginOptions(mem_unit_mib=mem_unit_mib),
        limits=limits,
        cumask=DbCUMaskAllocator(
            db_path, operator.devices(),
            on_remask=lambda h, m, n: limits.update_in_place(
                h, cu_mask=m, cu_count=n)),
    )
    return GPUSharePlugin(cfg), storage
