"""Isolation control plane: CU-mask bookkeeping + per-allocation limits files.

The data plane is the hand-written HSA interposer (native/egpu_shim.cpp,
loaded into containers via HSA_TOOLS_LIB) which applies CU masks with
``hsa_amd_queue_cu_set_mask`` and enforces HBM quotas by intercepting HSA
memory-pool allocation. This module is the agent-side half:

- ``CUMaskAllocator``: picks disjoint XCD-round-robin CU sets per GPU for
  live fractional allocations (persisted in the storage aux table so masks
  survive agent restarts and are reclaimed by GC).
- ``LimitsWriter``: writes the per-allocation ``<hash>.json`` limits file the
  shim reads inside the container (mounted by the Allocate response).

The reference has no open-source equivalent (its QoS lived in the closed qGPU
driver) — this layer is MI355X-scoped, not a port.
"""
from __future__ import annotations

import json
import os
import threading
from typing import Dict, List, Optional, Tuple

from .. import consts
from ..types import GPUDevice
from .cumask import mask_hex, mask_words_from_cus, parse_mask_hex

try:
    from .._fastwire import atomic_write as _native_atomic_write
except ImportError:  # pure-Python fallback in LimitsWriter._atomic_write
    _native_atomic_write = None

AUX_MASK_PREFIX = "mask/"  # aux key: mask/<alloc_hash> -> json record

# QoS rank order: reclaim flows strictly downhill (a high-priority pod may
# shrink low/normal pods; normal may shrink low; equals never preempt each
# other — they overlap, the documented oversubscription mode).
_PRIORITY_RANK = {"low": 0, "normal": 1, "high": 2}


def priority_rank(priority: Optional[str]) -> int:
    return _PRIORITY_RANK.get(priority or "normal", 1)


class _Alloc:
    __slots__ = ("gpu", "cus", "rank", "orig_n_cus")

    def __init__(self, gpu: int, cus: set, rank: int, orig_n_cus: int):
        self.gpu = gpu
        self.cus = cus
        self.rank = rank
        self.orig_n_cus = orig_n_cus  # pre-shrink size (== len(cus) if never shrunk)


class CUMaskAllocator:
    """Allocates disjoint CU sets (spread across XCDs) per physical GPU.

    Occupancy is reconstructed from the storage aux table on startup, so a
    restarted agent keeps honoring masks of running pods (the Restore path
    the reference declared but never implemented — pkg/manager/manager.go:20).

    QoS under contention (round-2 redesign): MES gang-schedules AQL queues
    round-robin regardless of hsa_amd_queue_set_priority (measured on
    MI355X: two fully-overlapped spinning queues at LOW vs HIGH completed
    identical work — profiles/qos_priority_null_r02). Priority therefore
    buys *CU exclusivity*, the resource the hardware does arbitrate: when a
    higher-priority allocation cannot be satisfied from free CUs, the
    allocator RECLAIMS pairs from lower-priority live allocations (shrinking
    their masks in place, lowest rank first), and re-expands them when
    capacity frees up. ``on_remask(hash, mask_hex, n_cus)`` tells the agent
    to rewrite the victim's limits file; the shim's watcher re-applies the
    narrowed mask to the victim's LIVE queues within its poll interval.
    """

    def __init__(self, storage, devices: List[GPUDevice], on_remask=None):
        self._storage = storage
        self._devices = {d.index: d for d in devices}
        self._lock = threading.Lock()
        self.on_remask = on_remask  # fn(alloc_hash, mask_hex, n_cus) | None
        # In-memory occupancy cache, rebuilt from the aux table at startup
        # (restart safety) and maintained on allocate/release: per-allocation
        # work must not scan every live record (O(n²) under churn).
        self._used: Dict[int, set] = {}
        self._by_hash: Dict[str, _Alloc] = {}
        for key, val in storage.aux_items(AUX_MASK_PREFIX):
            rec = json.loads(val)
            cus = self._mask_cus(rec["cu_mask"])
            gpu = rec.get("gpu_index")
            a = _Alloc(gpu, cus, priority_rank(rec.get("priority")),
                       rec.get("orig_cu_count", len(cus)))
            self._by_hash[key[len(AUX_MASK_PREFIX):]] = a
            self._used.setdefault(gpu, set()).update(cus)

    @staticmethod
    def _mask_cus(hexmask: str) -> set:
        cus = set()
        for w_i, w in enumerate(parse_mask_hex(hexmask)):
            for b in range(32):
                if w >> b & 1:
                    cus.add(w_i * 32 + b)
        return cus

    # ---- occupancy ----
    def _live_cus(self, gpu_index: int) -> set:
        return self._used.setdefault(gpu_index, set())

    def _free_pairs_by_xcd(self, gpu_index: int, total: int, xcds: int) -> List[List[int]]:
        per_xcd = total // xcds
        pairs_per_xcd = per_xcd // 2
        used = self._live_cus(gpu_index)
        return [
            [
                xcd * per_xcd + 2 * p
                for p in range(pairs_per_xcd)
                if xcd * per_xcd + 2 * p not in used
                and xcd * per_xcd + 2 * p + 1 not in used
            ]
            for xcd in range(xcds)
        ]

    @staticmethod
    def _take_round_robin(free_by_xcd: List[List[int]], want: int,
                          taken: List[int]) -> None:
        while len(taken) < want and any(free_by_xcd):
            progress = False
            for free in free_by_xcd:
                if len(taken) >= want:
                    break
                if free:
                    taken.append(free.pop(0))
                    progress = True
            if not progress:
                break

    def _persist(self, alloc_hash: str, a: _Alloc, total: int, percent: int) -> Tuple[str, int]:
        cus = sorted(a.cus)
        words = mask_words_from_cus(cus, total)
        hexmask = mask_hex(words)
        rank_name = {0: "low", 1: "normal", 2: "high"}[a.rank]
        self._storage.aux_set(
            AUX_MASK_PREFIX + alloc_hash,
            json.dumps(
                {
                    "gpu_index": a.gpu,
                    "cu_mask": hexmask,
                    "cu_count": len(cus),
                    "percent": percent,
                    "priority": rank_name,
                    "orig_cu_count": a.orig_n_cus,
                }
            ),
        )
        return hexmask, len(cus)

    def _remask_victim(self, victim_hash: str, a: _Alloc, total: int) -> None:
        """Persist a changed mask for a live allocation and notify the agent
        (limits rewrite → shim watcher re-applies to live queues)."""
        raw = self._storage.aux_get(AUX_MASK_PREFIX + victim_hash)
        percent = json.loads(raw).get("percent", 0) if raw else 0
        hexmask, n_cus = self._persist(victim_hash, a, total, percent)
        if self.on_remask is not None:
            try:
                self.on_remask(victim_hash, hexmask, n_cus)
            except Exception:  # never let a limits rewrite kill binding
                pass

    def _reclaim_locked(self, gpu_index: int, need_pairs: int, my_rank: int,
                        total: int) -> List[int]:
        """Shrink lower-priority live allocations (lowest rank first) until
        ``need_pairs`` CU pairs are freed; returns the freed pair-base CUs.
        Every victim keeps at least one pair."""
        victims = sorted(
            (
                (a.rank, h, a)
                for h, a in self._by_hash.items()
                if a.gpu == gpu_index and a.rank < my_rank and len(a.cus) > 2
            ),
            key=lambda t: (t[0], -len(t[2].cus)),
        )
        freed: List[int] = []
        changed: List[Tuple[str, _Alloc]] = []
        used = self._live_cus(gpu_index)
        for _, h, a in victims:
            if len(freed) >= need_pairs:
                break
            # give up pairs from the top of the victim's CU list, keep ≥1 pair
            pairs = sorted({cu - (cu % 2) for cu in a.cus})
            max_give = len(pairs) - 1
            give = min(max_give, need_pairs - len(freed))
            if give <= 0:
                continue
            for cu0 in pairs[-give:]:
                a.cus.discard(cu0)
                a.cus.discard(cu0 + 1)
                freed.append(cu0)
            changed.append((h, a))
        if freed:
            # CUs may still be claimed by OTHER overlapping allocations
            still = set()
            for a in self._by_hash.values():
                if a.gpu == gpu_index:
                    still |= a.cus
            for cu0 in freed:
                if cu0 not in still:
                    used.discard(cu0)
                if cu0 + 1 not in still:
                    used.discard(cu0 + 1)
            for h, a in changed:
                self._remask_victim(h, a, total)
        # hand back only pairs that are now genuinely free (an overlapping
        # sibling may still claim some)
        return [cu0 for cu0 in freed if cu0 not in used and cu0 + 1 not in used]

    def _expand_shrunk_locked(self, gpu_index: int, total: int, xcds: int) -> None:
        """After capacity frees up, grow shrunk allocations back toward their
        original size (highest rank first)."""
        shrunk = sorted(
            (
                (-a.rank, h, a)
                for h, a in self._by_hash.items()
                if a.gpu == gpu_index and len(a.cus) < a.orig_n_cus
            ),
            key=lambda t: t[0],
        )
        if not shrunk:
            return
        used = self._live_cus(gpu_index)
        for _, h, a in shrunk:
            want_pairs = (a.orig_n_cus - len(a.cus)) // 2
            if want_pairs <= 0:
                continue
            free_by_xcd = self._free_pairs_by_xcd(gpu_index, total, xcds)
            taken: List[int] = []
            self._take_round_robin(free_by_xcd, want_pairs, taken)
            if not taken:
                return  # no capacity; later releases will retry
            for cu0 in taken:
                a.cus.add(cu0)
                a.cus.add(cu0 + 1)
                used.add(cu0)
                used.add(cu0 + 1)
            self._remask_victim(h, a, total)

    def allocate(self, alloc_hash: str, gpu_index: int, percent: int,
                 priority: Optional[str] = None) -> Tuple[str, int]:
        """Pick a CU set of ``percent``% of the GPU, disjoint from live
        allocations when capacity allows. Under contention a higher-priority
        allocation reclaims pairs from lower-priority ones (see class doc);
        equal-priority oversubscription falls back to overlapping masks.
        Returns (mask_hex, n_cus)."""
        dev = self._devices.get(gpu_index)
        total = dev.cu_count if dev else consts.GFX950_CU_COUNT
        xcds = dev.xcd_count if dev else consts.GFX950_XCD_COUNT
        per_xcd = total // xcds
        from .cumask import cu_count_for_percent

        n = cu_count_for_percent(percent, total)
        pairs_per_xcd = per_xcd // 2
        rank = priority_rank(priority)
        with self._lock:
            # a re-allocation of the same hash releases its old claim first
            old = self._by_hash.pop(alloc_hash, None)
            if old is not None:
                still = set()
                for a in self._by_hash.values():
                    if a.gpu == old.gpu:
                        still |= a.cus
                self._used.setdefault(old.gpu, set()).difference_update(old.cus - still)
            used = self._live_cus(gpu_index)
            # ROCr CU masks have pair granularity: allocate whole CU pairs.
            # Water-filling round-robin over the XCDs' FREE pairs: as long as
            # free capacity exists anywhere, a new allocation never overlaps
            # (even when earlier pods fragmented some XCDs), while staying as
            # XCD-balanced as the free space allows.
            want = (n + 1) // 2
            taken: List[int] = []
            self._take_round_robin(
                self._free_pairs_by_xcd(gpu_index, total, xcds), want, taken)
            if len(taken) < want and rank > 0:
                # priority preemption: shrink lower-priority allocations
                taken.extend(self._reclaim_locked(
                    gpu_index, want - len(taken), rank, total))
            if len(taken) < want:
                # oversubscribed: overlap already-used pairs, preferring
                # pairs NOT held by any higher-priority allocation (a low
                # pod spilling over must degrade its peers, not a high
                # pod's exclusivity), spread round-robin across XCDs
                pair_max_rank: Dict[int, int] = {}
                for a in self._by_hash.values():
                    if a.gpu != gpu_index:
                        continue
                    for cu in a.cus:
                        cu0 = cu - (cu % 2)
                        if a.rank > pair_max_rank.get(cu0, -1):
                            pair_max_rank[cu0] = a.rank
                candidates = []
                for p in range(pairs_per_xcd):
                    for xcd in range(xcds):
                        cu0 = xcd * per_xcd + 2 * p
                        if cu0 not in taken:
                            candidates.append(cu0)
                # stable sort: pairs held only by <=my-rank allocations
                # first; RR order preserved within each class
                candidates.sort(key=lambda cu0: pair_max_rank.get(cu0, -1) > rank)
                taken.extend(candidates[: want - len(taken)])
            cus: List[int] = []
            for cu0 in taken[:want]:
                cus.extend((cu0, cu0 + 1))
            a = _Alloc(gpu_index, set(cus), rank, len(cus))
            hexmask, n_eff = self._persist(alloc_hash, a, total, percent)
            self._by_hash[alloc_hash] = a
            used.update(a.cus)
        return hexmask, n_eff

    def _release_cached(self, alloc_hash: str) -> Optional[int]:
        entry = self._by_hash.pop(alloc_hash, None)
        if entry is None:
            return None
        used = self._used.setdefault(entry.gpu, set())
        # only remove CUs not still claimed by another live mask
        still = set()
        for a in self._by_hash.values():
            if a.gpu == entry.gpu:
                still |= a.cus
        used.difference_update(entry.cus - still)
        return entry.gpu

    def _dev_geometry(self, gpu_index: int) -> Tuple[int, int]:
        dev = self._devices.get(gpu_index)
        total = dev.cu_count if dev else consts.GFX950_CU_COUNT
        xcds = dev.xcd_count if dev else consts.GFX950_XCD_COUNT
        return total, xcds

    def release(self, alloc_hash: str) -> None:
        with self._lock:
            gpu = self._release_cached(alloc_hash)
            if gpu is not None:
                self._expand_shrunk_locked(gpu, *self._dev_geometry(gpu))
        self._storage.aux_delete(AUX_MASK_PREFIX + alloc_hash)

    def release_many(self, hashes) -> None:
        """Batch form for GC: one cache pass + one storage transaction."""
        hashes = list(hashes)
        with self._lock:
            gpus = {self._release_cached(h) for h in hashes}
            for gpu in gpus:
                if gpu is not None:
                    self._expand_shrunk_locked(gpu, *self._dev_geometry(gpu))
        self._storage.aux_delete_many(AUX_MASK_PREFIX + h for h in hashes)

    def get(self, alloc_hash: str) -> Optional[dict]:
        raw = self._storage.aux_get(AUX_MASK_PREFIX + alloc_hash)
        return json.loads(raw) if raw else None


class _TxnAux:
    """Storage-shaped aux accessor bound to one sqlite connection inside an
    open transaction (no commits — the caller owns the txn boundary)."""

    def __init__(self, conn):
        self._conn = conn

    def aux_items(self, prefix: str = "") -> list:
        return self._conn.execute(
            "SELECT key, val FROM aux WHERE key LIKE ?", (prefix + "%",)
        ).fetchall()

    def aux_get(self, key: str):
        row = self._conn.execute("SELECT val FROM aux WHERE key=?", (key,)).fetchone()
        return row[0] if row else None

    def aux_set(self, key: str, val: str) -> None:
        self._conn.execute(
            "INSERT INTO aux(key, val) VALUES(?, ?) "
            "ON CONFLICT(key) DO UPDATE SET val=excluded.val", (key, val))

    def aux_delete(self, key: str) -> None:
        self._conn.execute("DELETE FROM aux WHERE key=?", (key,))

    def aux_delete_many(self, keys) -> None:
        self._conn.executemany("DELETE FROM aux WHERE key=?", [(k,) for k in keys])


class DbCUMaskAllocator:
    """Cross-process CU-mask allocator for the pre-forked data plane.

    Every worker process opens its own connection to the shared state DB;
    each allocate/release runs under ``BEGIN IMMEDIATE`` (the sqlite write
    lock IS the cross-process mutex), rebuilding occupancy from the mask/*
    aux rows inside the transaction — correct by construction, no shared
    memory. Mask rows are bounded by live allocations per node (hundreds),
    so the reload is cheap. Same API as CUMaskAllocator.
    """

    VER_KEY = "maskver"

    def __init__(self, db_path: str, devices: List[GPUDevice], on_remask=None):
        import sqlite3

        self._devices = list(devices)
        self.on_remask = on_remask
        import fcntl

        # same flock sidecar as Storage: cross-process handoff at kernel
        # granularity instead of sqlite's sleepy busy handler
        self._flock_fd = os.open(db_path + ".lock", os.O_CREAT | os.O_RDWR, 0o644)
        self._conn = sqlite3.connect(db_path, check_same_thread=False)
        # held across setup too: workers opening a fresh file together would
        # otherwise fail the WAL switch with "database is locked" (it needs
        # the database to itself and does not wait)
        fcntl.flock(self._flock_fd, fcntl.LOCK_EX)
        try:
            self._conn.execute("PRAGMA journal_mode=WAL")
            self._conn.execute("PRAGMA busy_timeout=10000")
            self._conn.execute(
                "CREATE TABLE IF NOT EXISTS aux (key TEXT PRIMARY KEY, val TEXT NOT NULL)"
            )
            self._conn.commit()
        finally:
            fcntl.flock(self._flock_fd, fcntl.LOCK_UN)
        self._local = threading.Lock()
        # version-cached occupancy: every mutating txn (any process) bumps
        # maskver under the flock, so the full aux rescan happens only when
        # ANOTHER process changed the mask set since our last txn
        self._cached_base: Optional[CUMaskAllocator] = None
        self._cached_ver: Optional[str] = None
        self._aux = _TxnAux(self._conn)

    def _base(self):
        ver = self._aux.aux_get(self.VER_KEY)
        if self._cached_base is None or ver != self._cached_ver or ver is None:
            self._cached_base = CUMaskAllocator(self._aux, self._devices,
                                                on_remask=self.on_remask)
        return self._cached_base

    def _bump(self) -> None:
        import uuid

        self._cached_ver = uuid.uuid4().hex
        self._aux.aux_set(self.VER_KEY, self._cached_ver)

    def _txn(self):
        class _Txn:
            def __init__(s, conn):
                s.conn = conn

            def __enter__(s):
                import fcntl

                fcntl.flock(s.fd, fcntl.LOCK_EX)
                s.conn.execute("BEGIN IMMEDIATE")
                return s

            def __exit__(s, et, ev, tb):
                import fcntl

                try:
                    if et is None:
                        try:
                            s.conn.execute("COMMIT")
                        except Exception:
                            # a failed COMMIT leaves the txn open and would
                            # poison every later BEGIN on this connection
                            try:
                                s.conn.execute("ROLLBACK")
                            except Exception:
                                pass
                            raise
                    else:
                        try:
                            s.conn.execute("ROLLBACK")
                        except Exception:
                            pass
                finally:
                    fcntl.flock(s.fd, fcntl.LOCK_UN)
                return False

        t = _Txn(self._conn)
        t.fd = self._flock_fd
        return t

    def allocate(self, alloc_hash: str, gpu_index: int, percent: int,
                 priority: Optional[str] = None) -> Tuple[str, int]:
        with self._local, self._txn():
            out = self._base().allocate(alloc_hash, gpu_index, percent,
                                        priority=priority)
            self._bump()
            return out

    def release(self, alloc_hash: str) -> None:
        with self._local, self._txn():
            self._base().release(alloc_hash)
            self._bump()

    def release_many(self, hashes) -> None:
        with self._local, self._txn():
            self._base().release_many(hashes)
            self._bump()

    def get(self, alloc_hash: str) -> Optional[dict]:
        with self._local:
            raw = self._aux.aux_get(AUX_MASK_PREFIX + alloc_hash)
        return json.loads(raw) if raw else None

    def close(self) -> None:
        with self._local:
            self._conn.close()
        try:
            os.close(self._flock_fd)
        except OSError:
            pass


class LimitsWriter:
    """Per-allocation limits files consumed by the HSA shim in-container.

    Layout: ``<limits_dir>/<hash>.json`` on the host, mounted read-only at
    ``/etc/egpu/limits-<kind>.json`` in the container. Written (empty) at
    Allocate time so kubelet can mount it, finalized at PreStart once the
    physical GPU binding is known."""

    def __init__(self, limits_dir: str):
        self.limits_dir = limits_dir
        os.makedirs(limits_dir, exist_ok=True)

    def host_path(self, alloc_hash: str) -> str:
        return os.path.join(self.limits_dir, f"{alloc_hash}.json")

    @staticmethod
    def container_path(kind: str) -> str:
        return f"/etc/egpu/limits-{kind}.json"

    def touch(self, alloc_hash: str) -> str:
        p = self.host_path(alloc_hash)
        if not os.path.exists(p):
            self._atomic_write(p, {})
        return p

    def finalize(
        self,
        alloc_hash: str,
        gpu_indexes: List[int],
        devices: List[GPUDevice],
        cu_mask: Optional[str] = None,
        cu_count: Optional[int] = None,
        mem_limit_bytes: Optional[int] = None,
        priority: Optional[str] = None,
    ) -> None:
        dev_by_idx = {d.index: d for d in devices}
        rec: Dict = {
            "version": 1,
            "gpu_indexes": gpu_indexes,
            "render_minors": [
                dev_by_idx[i].drm_render_minor for i in gpu_indexes if i in dev_by_idx
            ],
            "uuids": [dev_by_idx[i].uuid for i in gpu_indexes if i in dev_by_idx],
        }
        if cu_mask is not None:
            rec["cu_mask"] = cu_mask
            rec["cu_count"] = cu_count
        if mem_limit_bytes is not None:
            rec["mem_limit_bytes"] = mem_limit_bytes
        if priority is not None:
            rec["priority"] = priority
        self._atomic_write(self.host_path(alloc_hash), rec)

    def update_in_place(self, alloc_hash: str, **fields) -> None:
        """Merge ``fields`` into an existing limits file WITHOUT replacing the
        inode. The file is bind-mounted into its container one-to-one, so an
        os.replace would update only the host's view; in-place truncate+write
        keeps the container-visible inode current. The shim's watcher
        tolerates a torn mid-write read by retrying on its next poll tick.
        """
        path = self.host_path(alloc_hash)
        try:
            with open(path, "r+") as f:
                try:
                    rec = json.load(f)
                except ValueError:
                    rec = {}
                rec.update(fields)
                f.seek(0)
                f.truncate()
                json.dump(rec, f)
                f.flush()
                os.fsync(f.fileno())
        except FileNotFoundError:
            self._atomic_write(path, dict(fields))

    def delete(self, alloc_hash: str) -> None:
        try:
            os.unlink(self.host_path(alloc_hash))
        except FileNotFoundError:
            pass

    def read(self, alloc_hash: str) -> dict:
        with open(self.host_path(alloc_hash)) as f:
            return json.load(f)

    @staticmethod
    def _atomic_write(path: str, obj: dict) -> None:
        # unique temp name: concurrent writers of the SAME allocation (e.g. a
        # kubelet retry racing the first attempt) must not clobber each
        # other's temp file (found by tools/soak.py)
        if _native_atomic_write is not None:
            # temp file, write and rename in one GIL-free call
            # (native/bindfx.h); json.dumps gives json.dump's bytes
            _native_atomic_write(path, json.dumps(obj).encode())
            return
        import tempfile

        fd, tmp = tempfile.mkstemp(dir=os.path.dirname(path), suffix=".tmp")
        try:
            with os.fdopen(fd, "w") as f:
                json.dump(obj, f)
            os.replace(tmp, path)
        except BaseException:
            try:
                os.unlink(tmp)
            except OSError:
                pass
            raise
