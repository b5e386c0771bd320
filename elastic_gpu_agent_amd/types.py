"""Domain types: device-set identity and per-pod allocation records.

Wire/disk compatible with the reference's state (ref: pkg/types/device.go:11-54,
pkg/types/pod.go:10-62): a Device is a sorted fake-device-ID list identified by
the first 8 hex chars of sha256(":".join(sorted_ids)); pod state serializes as
JSON ``{container: {"Hash": .., "List": [..], "ResourceName": ..}}`` keyed by
``namespace/name`` so a node can be migrated from the reference agent's DB.
"""
from __future__ import annotations

import hashlib
import json
from dataclasses import dataclass, field
from typing import Dict, Iterable, List

from .protos import fastpath


def hash_device_ids(sorted_ids: List[str]) -> str:
    return hashlib.sha256(":".join(sorted_ids).encode()).hexdigest()[:8]


@dataclass(frozen=True)
class Device:
    """An allocated set of fake device IDs for one resource name.

    At the 1-MiB gpu-memory contract unit a device set holds up to ~295k
    IDs; the wire fast path (fastwire.decode_prestart_digest2) delivers the
    sorted list pre-serialized as a JSON array fragment instead of Python
    strings. Such a Device carries ``list_json`` + ``count`` with an empty
    ``list``; ``n_ids`` abstracts over both forms and ``val()`` splices the
    fragment verbatim into the reference-format record.

    A large set of consecutive IDs arrives (decode_prestart_digest3) and is
    stored as ``runs_json`` + ``count``: [[prefix, width, start, count], ...]
    (fastpath.ids_to_runs). ``ids()``, ``to_json_obj()`` and
    ``to_json_bytes()`` expand it on demand and stay reference-format;
    ``to_stored_bytes()`` is what the store's own rows hold."""

    hash: str
    list: tuple
    resource_name: str
    count: int = -1          # -1 → len(list)
    list_json: bytes = b""   # pre-serialized sorted JSON array (C++ digest)
    runs_json: bytes = b""   # the same set as ID runs, compact JSON

    @staticmethod
    def new(device_ids: Iterable[str], resource_name: str = "") -> "Device":
        ids = tuple(sorted(device_ids))
        return Device(hash=hash_device_ids(list(ids)), list=ids, resource_name=resource_name)

    @staticmethod
    def from_digest(h: str, count: int, list_json: bytes,
                    resource_name: str = "") -> "Device":
        return Device(hash=h, list=(), resource_name=resource_name,
                      count=count, list_json=list_json)

    @staticmethod
    def from_runs(h: str, count: int, runs_json: bytes,
                  resource_name: str = "") -> "Device":
        return Device(hash=h, list=(), resource_name=resource_name,
                      count=count, runs_json=runs_json)

    @property
    def n_ids(self) -> int:
        return self.count if self.count >= 0 else len(self.list)

    def _list_fragment(self) -> bytes:
        """The sorted IDs as a JSON array fragment (digest and runs forms)."""
        if self.runs_json:
            return fastpath.expand_runs(self.runs_json, self.count)
        return self.list_json

    def ids(self) -> tuple:
        """Materialized sorted ID tuple (lazily decoded for digest form)."""
        if self.list or not (self.list_json or self.runs_json):
            return self.list
        return tuple(json.loads(self._list_fragment()))

    def equals(self, other: "Device") -> bool:
        return (
            self.hash == other.hash
            and self.ids() == other.ids()
            and self.resource_name == other.resource_name
        )

    # JSON shape uses Go field names for reference-state compatibility.
    def to_json_obj(self) -> dict:
        return {"Hash": self.hash, "List": list(self.ids()),
                "ResourceName": self.resource_name}

    def to_json_bytes(self) -> bytes:
        """Record bytes; splices the pre-serialized list when present
        (byte-identical to json.dumps of to_json_obj)."""
        if (self.list_json or self.runs_json) and not self.list:
            return (b'{"Hash":' + json.dumps(self.hash).encode()
                    + b',"List":' + self._list_fragment()
                    + b',"ResourceName":' + json.dumps(self.resource_name).encode()
                    + b"}")
        return json.dumps(self.to_json_obj(), separators=(",", ":")).encode()

    def to_stored_bytes(self) -> bytes:
        """What the store's row holds: {"Hash","Runs","N","ResourceName"} for
        a set that qualifies as runs, to_json_bytes() for every other."""
        runs = self.runs_json
        if not runs and len(self.list) >= fastpath.RUNS_MIN_IDS:
            runs = fastpath.ids_to_runs(self.list)
        if not runs:
            return self.to_json_bytes()
        return (b'{"Hash":' + json.dumps(self.hash).encode()
                + b',"Runs":' + runs
                + b',"N":' + str(self.n_ids).encode()
                + b',"ResourceName":' + json.dumps(self.resource_name).encode()
                + b"}")

    @staticmethod
    def from_json_obj(obj: dict) -> "Device":
        if "Runs" in obj:
            runs, n = obj["Runs"], obj.get("N")
            if type(n) is not int or n < 0 or not isinstance(runs, list):
                raise ValueError("runs record: bad N or Runs")
            try:
                total = sum(r[3] for r in runs)
            except (TypeError, IndexError):
                raise ValueError("runs record: malformed run") from None
            if total != n:
                raise ValueError(f"runs record: N={n} but the runs hold {total}")
            return Device.from_runs(
                obj.get("Hash", ""), n,
                json.dumps(runs, separators=(",", ":")).encode(),
                obj.get("ResourceName", ""))
        return Device(
            hash=obj.get("Hash", ""),
            list=tuple(obj.get("List") or ()),
            resource_name=obj.get("ResourceName", ""),
        )


@dataclass(frozen=True)
class PodContainer:
    namespace: str
    name: str
    container: str

    def __str__(self) -> str:
        return f"{self.namespace}/{self.name}:{self.container}"

    def pod(self) -> str:
        return f"{self.namespace}/{self.name}"


@dataclass
class PodInfo:
    namespace: str
    name: str
    container_device_map: Dict[str, Device] = field(default_factory=dict)

    def key(self) -> str:
        return f"{self.namespace}/{self.name}"

    def val(self) -> bytes:
        # byte-identical to json.dumps(..., separators=(",", ":")) of the
        # {container: to_json_obj()} map, but splices pre-serialized device
        # lists so 295k-ID sets never round-trip through Python objects
        parts = []
        for c, d in self.container_device_map.items():
            parts.append(json.dumps(c).encode() + b":" + d.to_json_bytes())
        return b"{" + b",".join(parts) + b"}"

    def stored_val(self) -> bytes:
        """The store's row: val() with each large consecutive set held as
        runs (Device.to_stored_bytes). Equal to val() when no set qualifies."""
        parts = []
        for c, d in self.container_device_map.items():
            parts.append(json.dumps(c).encode() + b":" + d.to_stored_bytes())
        return b"{" + b",".join(parts) + b"}"

    @staticmethod
    def from_raw(key: str, val: bytes) -> "PodInfo":
        parts = key.split("/")
        if len(parts) != 2:
            raise ValueError(f"error key format: {key}")
        obj = json.loads(val.decode()) if val else {}
        return PodInfo(
            namespace=parts[0],
            name=parts[1],
            container_device_map={c: Device.from_json_obj(d) for c, d in obj.items()},
        )


@dataclass
class GPUDevice:
    """One enumerated physical MI355X (or fake) GPU.

    The reference's operator returned {UUID, GPUIndex, Memory}
    (ref: pkg/operator/base.go:77-83); the MI355X-native record additionally
    carries everything placement and materialization need: the DRM render-node
    minor (the injectable device node), CU count, NUMA node, and the xGMI peer
    set used for topology-aware preferred allocation.
    """

    uuid: str
    index: int
    memory_bytes: int
    drm_render_minor: int = 128
    drm_card: int = 0
    cu_count: int = 256
    xcd_count: int = 8
    numa_node: int = 0
    xgmi_peers: tuple = ()  # GPU indexes directly linked over xGMI
    compute_partition: str = "SPX"

    @property
    def memory_mib(self) -> int:
        return self.memory_bytes // (1024 * 1024)
