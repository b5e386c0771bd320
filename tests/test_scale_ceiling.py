"""Device-ID ceiling at full contract scale (SURVEY §7 risk 4).

8 GPUs × 1-MiB memory units = 8 × 294,912 = 2,359,296 fake device IDs on one
node. These tests exercise the three pressure points at that scale on CPU:

1. ListAndWatch snapshot: encode size and time for the full inventory.
2. podresources List responses near/over the reference's 16 MiB client cap
   (ref pkg/kube/locator.go:34): our client must survive them and the C++
   digest must keep locate() fast.
3. Locator scan cost with a loaded node.
"""
import os
import time

import pytest

from elastic_gpu_agent_amd import consts
from elastic_gpu_agent_amd.types import Device, PodContainer

from helpers import Harness

FULL_MEM_UNITS = 294912  # 288 GiB at 1 MiB


@pytest.mark.timeout(300)
def test_listandwatch_snapshot_8gpu_1mib():
    """Full 8-GPU 1-MiB snapshot: 2.36 M devices encode in bounded time and
    the cached-encode path makes re-sends free."""
    import tempfile

    tmp = tempfile.mkdtemp()
    h = Harness(tmp, gpus=8, mem_unit_mib=1)
    try:
        t0 = time.perf_counter()
        groups = h.plugin.memory.device_groups()
        from elastic_gpu_agent_amd.protos import fastpath

        encoded = fastpath.encode_list_and_watch(groups)
        dt = time.perf_counter() - t0
        n_devices = sum(len(ids) for ids, _ in groups)
        assert n_devices == 8 * FULL_MEM_UNITS
        size_mb = len(encoded) / 2**20
        print(f"LISTANDWATCH_8GPU_1MIB devices={n_devices} "
              f"size={size_mb:.1f}MB encode={dt*1e3:.0f}ms")
        # kubelet re-reads the stream on reconnect: the encode must be
        # sub-second even for the full node inventory
        assert dt < 5.0, f"snapshot encode took {dt:.1f}s"
        # a snapshot is ~60 MB; it streams over the local socket (no gRPC
        # 4 MiB default applies — kubelet sets unlimited for device plugins)
        assert size_mb > 20
    finally:
        h.close()


@pytest.mark.timeout(600)
def test_locator_digest_at_16mib_cap(tmp_path):
    """A podresources List response crossing the reference's 16 MiB message
    cap: our client accepts it and the C++ digest locate stays fast.

    20 pods × 73,728 IDs ≈ 1.47 M IDs ≈ 17.5 MB encoded — the reference
    client (grpc maxmsg 16 MiB, locator.go:34) would REFUSE this response;
    the MI355X agent must not."""
    from elastic_gpu_agent_amd.kube.locator import KubeletDeviceLocator
    from elastic_gpu_agent_amd.kube.podresources_server import PodResourcesServer

    sock = str(tmp_path / "podresources.sock")
    srv = PodResourcesServer(sock)
    pods = []
    units = 73728
    for p in range(20):
        gpu = p % 8
        # IDs unique per pod: prefixed with the pod number
        ids = [f"{gpu}-{p:02d}-{i:06d}" for i in range(units)]
        srv.set_assignment("bench", f"pod-{p}", "main",
                           consts.RESOURCE_GPU_MEMORY, ids)
        pods.append((f"pod-{p}", ids))
    srv.start()
    loc = KubeletDeviceLocator(consts.RESOURCE_GPU_MEMORY, sock)
    try:
        raw = loc._list_raw_once()
        size_mb = len(raw) / 2**20
        assert size_mb > 16, f"response only {size_mb:.1f} MB — not over the cap"

        target_name, target_ids = pods[13]
        d = Device.new(target_ids, consts.RESOURCE_GPU_MEMORY)
        t0 = time.perf_counter()
        pc = loc.locate(d)
        dt = time.perf_counter() - t0
        assert pc == PodContainer("bench", target_name, "main")
        print(f"LOCATE_OVER_CAP response={size_mb:.1f}MB locate={dt*1e3:.0f}ms")
        assert dt < 2.0, f"locate took {dt:.2f}s on a loaded node"

        # miss path also bounded (scans everything)
        ghost = Device.new(["9-000001"], consts.RESOURCE_GPU_MEMORY)
        t0 = time.perf_counter()
        with pytest.raises(KeyError):
            loc.locate(ghost)
        assert time.perf_counter() - t0 < 2.0
    finally:
        loc.close()
        srv.stop()


def test_podresources_digest_groups_split_entries(tmp_path):
    """≥1.21 kubelet shape: one ContainerDevices entry PER ID must hash to
    the same set as the merged form (ref locator.go:66-89 dual handling)."""
    from elastic_gpu_agent_amd import _fastwire
    from elastic_gpu_agent_amd.protos import podresources as pr

    ids = [f"0-{i:02d}" for i in range(30)]
    split = {"pod_resources": [{"name": "p", "namespace": "ns", "containers": [
        {"name": "c", "devices": [
            {"resource_name": consts.RESOURCE_GPU_CORE, "device_ids": [i]}
            for i in ids
        ]}]}]}
    merged = {"pod_resources": [{"name": "p", "namespace": "ns", "containers": [
        {"name": "c", "devices": [
            {"resource_name": consts.RESOURCE_GPU_CORE, "device_ids": ids}
        ]}]}]}
    d = Device.new(ids, consts.RESOURCE_GPU_CORE)
    for shape in (split, merged):
        rows = _fastwire.podresources_digest(pr.ListPodResourcesResponse.encode(shape))
        assert ("ns", "p", "c", consts.RESOURCE_GPU_CORE, d.hash, 30) in rows


@pytest.mark.timeout(300)
def test_listandwatch_wire_delivery_8gpu_1mib(tmp_path):
    """The full snapshot must also DELIVER over the wire promptly (kubelet
    re-reads it on every reconnect): raw-stream the 58 MB mem snapshot and
    bound the time. (Decode here is the Go kubelet's job; our Python
    decode of 2.36 M devices takes ~26 s and is not on any agent path.)"""
    from elastic_gpu_agent_amd import egrpc
    from elastic_gpu_agent_amd.protos import deviceplugin as dp

    h = Harness(str(tmp_path), gpus=8, mem_unit_mib=1)
    h.plugin.memory_server.serve()
    h.plugin.memory_server.wait_ready()
    ch = egrpc.Channel(h.plugin.memory_server.socket_path)
    try:
        stream = ch.unary_stream(dp.METHOD_LIST_AND_WATCH,
                                 request_serializer=dp.Empty.encode)
        t0 = time.perf_counter()
        it = stream({})
        first = next(it)
        dt = time.perf_counter() - t0
        print(f"LAW_DELIVERY size={len(first)/2**20:.1f}MB t={dt:.2f}s")
        assert len(first) > 50 * 2**20
        assert dt < 10.0, f"snapshot delivery took {dt:.1f}s"
        it.close()
    finally:
        ch.close()
        h.close()
