"""Hot-path codecs for the device-plugin RPCs.

Uses the native _fastwire accelerator when built (native/fastwire.cpp;
built by `python -m elastic_gpu_agent_amd.native.build`), falling back to the
pure-Python wire codec with identical semantics — the test-suite asserts
both agree byte-for-byte. At 1-MiB memory units a 72 GiB allocation carries
73,728 device IDs; the accelerator turns a ~73 ms decode into ~2 ms.
"""
from __future__ import annotations

from typing import List

from . import deviceplugin as dp
from .protowire import encode_varint

try:
    from elastic_gpu_agent_amd import _fastwire  # built in-tree

    HAVE_NATIVE = True
except ImportError:  # pure-Python fallback (same wire semantics)
    _fastwire = None
    HAVE_NATIVE = False


def decode_allocate_request(buf: bytes) -> dict:
    """AllocateRequest → {"container_requests": [{"devicesIDs": [...]}, ...]}"""
    if _fastwire is not None:
        lists = _fastwire.decode_nested_string_lists(buf)
        return {"container_requests": [{"devicesIDs": ids} for ids in lists]}
    return dp.AllocateRequest.decode(buf)


def decode_allocate_request_digest(buf: bytes) -> dict:
    """Server-side Allocate deserializer: per container, (device-set hash,
    id count) — all the handler needs — computed in C++ without building the
    ID list (an Allocate at the reference-exact 1-MiB memory units can carry
    ~295k IDs; materializing them cost more than the rest of the RPC)."""
    if _fastwire is not None and hasattr(_fastwire, "digest_allocate_request"):
        return {
            "container_requests": [
                {"digest": (h, n)} for h, n in _fastwire.digest_allocate_request(buf)
            ]
        }
    from ..types import Device

    out = []
    for cr in dp.AllocateRequest.decode(buf).get("container_requests", []):
        ids = cr.get("devicesIDs", [])
        d = Device.new(ids)
        out.append({"digest": (d.hash, len(ids))})
    return {"container_requests": out}


def decode_preferred_request_digest(buf: bytes) -> dict:
    """GetPreferredAllocation deserializer for huge ID pools (gpu-memory at
    1-MiB units: kubelet sends ~295k available IDs per admission). Produces
    per-GPU availability COUNTS (all the single-GPU pick policy needs) plus
    the raw buffer for on-demand extraction of the chosen GPU's IDs —
    never materializing the pool as Python strings."""
    if _fastwire is not None and hasattr(_fastwire, "preferred_digest"):
        crs = []
        for i, (counts, must, size) in enumerate(_fastwire.preferred_digest(buf)):
            crs.append(
                {
                    "counts": {int(g): int(n) for g, n in counts.items()},
                    "must_include_deviceIDs": list(must),
                    "allocation_size": int(size),
                    "_raw": buf,
                    "_index": i,
                }
            )
        return {"container_requests": crs}
    return dp.PreferredAllocationRequest.decode(buf)


def extract_preferred(raw: bytes, index: int, gpu: int, n: int) -> bytes:
    """Encoded ContainerPreferredAllocationResponse body: the lexicographically
    first ``n`` available IDs of ``gpu`` in container ``index`` of ``raw``."""
    return _fastwire.preferred_extract(raw, index, gpu, n)


def encode_preferred_response(resp: dict) -> bytes:
    """PreferredAllocationResponse encoder accepting either materialized
    ``deviceIDs`` lists or pre-encoded ``raw`` container bodies (the digest
    path's zero-materialization output)."""
    out = bytearray()
    for cr in resp.get("container_responses", []):
        body = cr.get("raw")
        if body is None:
            ids = cr.get("deviceIDs", [])
            if _fastwire is not None:
                body = _fastwire.encode_string_list(ids)
            else:
                body = b"".join(
                    b"\x0a" + encode_varint(len(i.encode())) + i.encode() for i in ids
                )
        out += b"\x0a" + encode_varint(len(body)) + body
    return bytes(out)


def encode_allocate_request(req: dict) -> bytes:
    """Client-side fast path (bench / tests; kubelet's own Go encoder plays
    this role in production)."""
    if _fastwire is not None:
        lists = [cr.get("devicesIDs", []) for cr in req.get("container_requests", [])]
        return _fastwire.encode_nested_string_lists(lists)
    return dp.AllocateRequest.encode(req)


def encode_allocate_response(resp: dict) -> bytes:
    """Server-side response half of the Allocate hot path (the headline p50
    metric): the Python MessageSpec encoder costs ~21 µs per fractional-pod
    response; the C++ encoder ~2 µs. Byte-identical output (asserted in
    tests/test_fastpath.py)."""
    if _fastwire is not None:
        return _fastwire.encode_allocate_response(resp)
    return dp.AllocateResponse.encode(resp)


def encode_prestart_request(req: dict) -> bytes:
    if _fastwire is not None:
        return _fastwire.encode_string_list(req.get("devicesIDs", []))
    return dp.PreStartContainerRequest.encode(req)


def decode_prestart_request(buf: bytes) -> dict:
    if _fastwire is not None:
        return {"devicesIDs": _fastwire.decode_string_list(buf)}
    return dp.PreStartContainerRequest.decode(buf)


def decode_prestart_request_digest(buf: bytes) -> dict:
    """PreStart deserializer: device-set hash + count + the sorted ID list
    pre-serialized as a JSON fragment, all from one C++ pass. The handler
    persists the fragment verbatim (Device.from_digest), so at the 1-MiB
    contract unit the ~295k IDs never materialize as Python strings."""
    if _fastwire is not None and hasattr(_fastwire, "decode_prestart_digest3"):
        # a large set of consecutive IDs comes back as its runs fragment and
        # the ~200 KB literal list is never built (see ids_to_runs)
        h, n, frag, is_runs = _fastwire.decode_prestart_digest3(buf)
        return {"devicesIDs": [], "device_hash": h, "device_count": n,
                "list_runs" if is_runs else "list_json": frag}
    if _fastwire is not None and hasattr(_fastwire, "decode_prestart_digest2"):
        h, n, list_json = _fastwire.decode_prestart_digest2(buf)
        return {"devicesIDs": [], "device_hash": h, "device_count": n,
                "list_json": list_json}
    if _fastwire is not None and hasattr(_fastwire, "decode_prestart_digest"):
        ids, h = _fastwire.decode_prestart_digest(buf)
        return {"devicesIDs": ids, "device_hash": h}
    return decode_prestart_request(buf)


# ---- hash memo: PreStart reuses the hash Allocate just computed --------------
# For a set that is stored as runs, the runs fragment names the sorted list
# exactly, so the native Allocate digest leaves fragment -> hash in a bounded
# per-process memo and the PreStart digest takes it (and removes it) instead
# of hashing the same ~200 KB again; a miss only hashes (native/hashmemo.h).
# The pure-Python codecs have no memo.
HASH_MEMO_ENTRIES = 256  # hashmemo.h kMemoEntries


def hash_memo_configure(entries: int) -> None:
    """Entry cap of the memo; 0 turns it off and empties it."""
    if _fastwire is not None and hasattr(_fastwire, "hash_memo_configure"):
        _fastwire.hash_memo_configure(entries)


def hash_memo_stats() -> dict:
    """puts / hits / misses / evictions / entries / cap ({} without the
    native module)."""
    if _fastwire is not None and hasattr(_fastwire, "hash_memo_stats"):
        return dict(_fastwire.hash_memo_stats())
    return {}


# ---- ID runs: how the store keeps a large device set -----------------------
# A sorted set of mostly consecutive IDs ("0-000000" .. "0-018431") is kept as
# [[prefix, width, start, count], ...] instead of its literal list. The rules
# (native/idruns.h): an ID is run-encodable when it ends in a
# maximal run of 1..18 ASCII digits and holds no byte json.dumps would escape;
# an ID with the prefix and width of its predecessor and value == previous + 1
# extends the run, anything else starts one; a set is stored as runs only
# when every ID is run-encodable, it has >= RUNS_MIN_IDS IDs and at most
# count / RUNS_PER_IDS runs. The pure-Python versions below give the same
# bytes as the native ones (tests/test_record_runs.py).
RUNS_MIN_IDS = 1024
RUNS_PER_IDS = 8
RUNS_MAX_WIDTH = 18
RUNS_MAX_EXPANDED = 4 << 20  # idruns.h kRunsMaxExpanded


def _split_run_id(s: str):
    """(prefix, width, value) of a run-encodable ID, else None."""
    n = len(s)
    w = 0
    while w < n and "0" <= s[n - 1 - w] <= "9":
        w += 1
    if w == 0 or w > RUNS_MAX_WIDTH:
        return None
    prefix = s[:n - w]
    for ch in prefix:
        if ch < " " or ch > "\x7f" or ch in '"\\':
            return None
    return prefix, w, int(s[n - w:])


def _py_ids_to_runs(sorted_ids):
    n = len(sorted_ids)
    if n < RUNS_MIN_IDS:
        return None
    runs = []
    last = None  # (prefix, width, next value)
    for s in sorted_ids:
        t = _split_run_id(s)
        if t is None:
            return None
        if last is not None and t == last:
            runs[-1][3] += 1
        else:
            if len(runs) >= n // RUNS_PER_IDS:
                return None
            runs.append([t[0], t[1], t[2], 1])
        last = (t[0], t[1], t[2] + 1)
    import json

    return json.dumps(runs, separators=(",", ":")).encode()


def _py_expand_runs(frag: bytes, count: int) -> bytes:
    import json

    if b"\\" in frag:  # prefixes are stored unescaped
        raise RuntimeError("runs: bad prefix")
    try:
        runs = json.loads(frag.decode("ascii"))
    except ValueError as e:
        raise RuntimeError(f"runs: malformed fragment: {e}") from None
    if not isinstance(runs, list) or count < 0:
        raise RuntimeError("runs: malformed fragment")
    left, total = count, 2
    for r in runs:
        if not (isinstance(r, list) and len(r) == 4 and isinstance(r[0], str)
                and all(type(x) is int and x >= 0 for x in r[1:])):
            raise RuntimeError("runs: malformed fragment")
        prefix, width, start, n = r
        if any(ch < " " or ch > "\x7f" or ch in '"\\' for ch in prefix):
            raise RuntimeError("runs: bad prefix")
        if not 1 <= width <= RUNS_MAX_WIDTH:
            raise RuntimeError("runs: bad width")
        if n < 1 or n > left:
            raise RuntimeError("runs: count mismatch")
        left -= n
        if start + n > 10 ** width:
            raise RuntimeError("runs: past the width")
        total += n * (len(prefix) + width + 3)
        if total > RUNS_MAX_EXPANDED:
            raise RuntimeError("runs: too large")
    if left:
        raise RuntimeError("runs: count mismatch")
    parts = []
    for prefix, width, start, n in runs:
        parts.extend(f'"{prefix}{v:0{width}d}"' for v in range(start, start + n))
    return ("[" + ",".join(parts) + "]").encode()


def ids_to_runs(sorted_ids):
    """Runs fragment of an already sorted ID list, or None when the set does
    not qualify and keeps its literal list."""
    if _fastwire is not None and hasattr(_fastwire, "ids_to_runs"):
        return _fastwire.ids_to_runs(list(sorted_ids))
    return _py_ids_to_runs(sorted_ids)


def expand_runs(frag: bytes, count: int) -> bytes:
    """Runs fragment + the record's ID count -> the literal list fragment,
    json.dumps(ids, separators=(",", ":")). Raises on a fragment that does
    not describe exactly ``count`` IDs."""
    if _fastwire is not None and hasattr(_fastwire, "expand_runs"):
        return _fastwire.expand_runs(frag, count)
    return _py_expand_runs(frag, count)


# Precomputable per-GPU Device suffix: health + topology are identical for
# every fake device of a GPU.
def device_suffix(health: str, numa_node: int) -> bytes:
    health_b = health.encode()
    topo = dp.TopologyInfo.encode({"nodes": [{"ID": numa_node}]})
    return (
        b"\x12" + encode_varint(len(health_b)) + health_b  # Device.health (2)
        + b"\x1a" + encode_varint(len(topo)) + topo  # Device.topology (3)
    )


def encode_list_and_watch(groups: List[tuple]) -> bytes:
    """groups: [(ids, suffix_bytes)] → serialized ListAndWatchResponse."""
    if _fastwire is not None:
        return b"".join(_fastwire.encode_device_list(ids, suffix) for ids, suffix in groups)
    out = bytearray()
    for ids, suffix in groups:
        for did in ids:
            id_b = did.encode()
            body = b"\x0a" + encode_varint(len(id_b)) + id_b + suffix
            out += b"\x0a" + encode_varint(len(body)) + body
    return bytes(out)
