"""ctypes wrapper over libegpu_kernels.so (gfx950 verification kernels).

On a GPU box these are the empirical checks behind the isolation layer:
``census()`` proves a CU mask stuck (distinct CUs observed ≤ mask popcount),
``throughput_ms()`` proves compute share scales with the mask, and
``bandwidth_gbps()`` feeds occupancy reporting. Loading fails loudly if the
extension was not built — there is no eager/Python fallback for these.
"""
from __future__ import annotations

import ctypes
import os
from typing import List

_LIB = None


def _lib():
    global _LIB
    if _LIB is None:
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                            "libegpu_kernels.so")
        if not os.path.exists(path):
            raise RuntimeError(
                f"{path} not built — run `python -m elastic_gpu_agent_amd.native.build`"
            )
        lib = ctypes.CDLL(path)
        lib.egpu_last_error.restype = ctypes.c_char_p
        lib.egpu_census.argtypes = [
            ctypes.c_int, ctypes.c_int, ctypes.c_int,
            ctypes.POINTER(ctypes.c_uint32), ctypes.c_int,
            ctypes.POINTER(ctypes.c_int),
        ]
        lib.egpu_throughput.argtypes = [
            ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_float)
        ]
        lib.egpu_bandwidth.argtypes = [
            ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_double)
        ]
        lib.egpu_qos_probe.argtypes = [
            ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_int,
            ctypes.POINTER(ctypes.c_longlong),
        ]
        lib.egpu_device_count.argtypes = [ctypes.POINTER(ctypes.c_int)]
        lib.egpu_malloc_bytes.argtypes = [ctypes.c_int, ctypes.c_uint64]
        lib.egpu_free_vram.argtypes = [ctypes.c_int]
        lib.egpu_free_vram.restype = ctypes.c_uint64
        lib.egpu_selftest.argtypes = [
            ctypes.c_int, ctypes.POINTER(_SelftestParams), ctypes.POINTER(_SelftestReport)
        ]
        lib.egpu_selftest_records.argtypes = [
            ctypes.c_int, ctypes.POINTER(_SelftestParams),
            ctypes.POINTER(ctypes.c_uint32), ctypes.c_int,
        ]
        lib.egpu_selftest_expected.argtypes = [
            ctypes.c_uint32, ctypes.c_int, ctypes.POINTER(ctypes.c_uint32)
        ]
        lib.egpu_selftest_mfma_tile.argtypes = [
            ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_int,
            ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int8),
            ctypes.POINTER(ctypes.c_int8),
        ]
        _LIB = lib
    return _LIB


class ProbeError(RuntimeError):
    pass


def _check(rc: int, what: str):
    if rc != 0:
        raise ProbeError(f"{what} failed (rc={rc}): {_lib().egpu_last_error().decode()}")


def device_count() -> int:
    n = ctypes.c_int(0)
    _check(_lib().egpu_device_count(ctypes.byref(n)), "egpu_device_count")
    return n.value


def census(device: int = 0, blocks: int = 4096, spin: int = 200000) -> List[int]:
    """Returns the distinct physical-CU identities ((xcc<<16)|cu bits) that
    executed at least one workgroup."""
    max_ids = 1024
    ids = (ctypes.c_uint32 * max_ids)()
    n = ctypes.c_int(0)
    _check(
        _lib().egpu_census(device, blocks, spin, ids, max_ids, ctypes.byref(n)),
        "egpu_census",
    )
    return list(ids[: n.value])


def throughput_ms(device: int = 0, blocks: int = 2048, iters: int = 2_000_000) -> float:
    ms = ctypes.c_float(0)
    _check(_lib().egpu_throughput(device, blocks, iters, ctypes.byref(ms)), "egpu_throughput")
    return ms.value


def bandwidth_gbps(device: int = 0, mib: int = 1024) -> float:
    g = ctypes.c_double(0)
    _check(_lib().egpu_bandwidth(device, mib, ctypes.byref(g)), "egpu_bandwidth")
    return g.value


def qos_probe(device: int = 0, seconds: float = 5.0, blocks: int = 1024,
              iters: int = 50_000) -> int:
    """Timed contention probe: completed fma launches in `seconds` wall time.
    Two concurrent processes on overlapping CU masks with different queue
    priorities turn the ratio of returns into the measured QoS outcome."""
    n = ctypes.c_longlong(0)
    _check(_lib().egpu_qos_probe(device, seconds, blocks, iters, ctypes.byref(n)),
           "egpu_qos_probe")
    return n.value


def malloc_bytes(device: int, n: int) -> int:
    """hipMalloc probe; returns hipError_t (0 = success)."""
    return _lib().egpu_malloc_bytes(device, n)


def free_vram(device: int = 0) -> int:
    return _lib().egpu_free_vram(device)


# ---------------------------------------------------------------- self-test

SELFTEST_MAX_ROUNDS = 4096
SELFTEST_MAX_LDS = 163840
SELFTEST_KINDS = {"int": 1, "fma": 2, "mfma": 4, "lds": 8}  # bad_kinds bits
_INJECT_KINDS = {"int": 1, "fma": 2, "mfma": 3, "lds": 4, "hbm": 5}
_HBM_STATUS = {0: "ok", 1: "failed", 2: "skipped", 3: "off"}


class _SelftestParams(ctypes.Structure):
    _fields_ = [
        ("blocks", ctypes.c_int32), ("rounds", ctypes.c_int32),
        ("seed", ctypes.c_uint32), ("lds_bytes", ctypes.c_uint32),
        ("hbm_bytes", ctypes.c_uint64),
        ("inject_kind", ctypes.c_int32), ("reserved", ctypes.c_int32),
        ("inject_arg", ctypes.c_uint64),
    ]


class _SelftestReport(ctypes.Structure):
    _fields_ = [
        ("version", ctypes.c_uint32), ("waves_run", ctypes.c_uint32),
        ("cus_seen", ctypes.c_uint32), ("bad_waves", ctypes.c_uint32),
        ("bad_kinds", ctypes.c_uint32), ("n_bad_cus", ctypes.c_uint32),
        ("bad_cus", ctypes.c_uint32 * 64), ("lds_bytes", ctypes.c_uint32),
        ("hbm_status", ctypes.c_int32), ("hbm_bytes_checked", ctypes.c_uint64),
        ("hbm_miscompares", ctypes.c_uint64),
        ("hbm_first_bad_offset", ctypes.c_uint64),
        ("kernel_ms", ctypes.c_float), ("hbm_ms", ctypes.c_float),
    ]


def _selftest_params(blocks, rounds, lds_bytes, hbm_bytes, seed, inject) -> _SelftestParams:
    kind, arg = 0, 0
    if inject is not None:
        name, arg = inject
        if name not in _INJECT_KINDS:
            raise ValueError(f"unknown injection kind {name!r}")
        kind = _INJECT_KINDS[name]
    return _SelftestParams(blocks, rounds, seed & 0xFFFFFFFF, lds_bytes, hbm_bytes,
                           kind, 0, arg)


def selftest(device: int = 0, blocks: int = 1024, rounds: int = 64,
             lds_bytes: int = 32768, hbm_bytes: int = 32 << 20, seed: int = 0,
             _inject=None) -> dict:
    """Active self-test: integer, FP32-FMA, MFMA and LDS checks on every wave
    of a `blocks`-workgroup grid against the host reference, then a write /
    verify pattern over `hbm_bytes` of scratch (0 = off). Bad arguments raise
    ProbeError before any HIP call. `_inject` = (kind, arg) simulates a
    miscompare (tests only): kind int/fma/mfma/lds with a workgroup index, or
    hbm with a byte offset."""
    params = _selftest_params(blocks, rounds, lds_bytes, hbm_bytes, seed, _inject)
    rep = _SelftestReport()
    _check(_lib().egpu_selftest(device, ctypes.byref(params), ctypes.byref(rep)),
           "egpu_selftest")
    return {
        "version": rep.version,
        "waves_run": rep.waves_run,
        "cus_seen": rep.cus_seen,
        "bad_waves": rep.bad_waves,
        "bad_kinds": rep.bad_kinds,
        "bad_kind_names": [k for k, bit in SELFTEST_KINDS.items() if rep.bad_kinds & bit],
        "n_bad_cus": rep.n_bad_cus,
        "bad_cus": list(rep.bad_cus[: rep.n_bad_cus]),
        "lds_bytes": rep.lds_bytes,
        "hbm_status": _HBM_STATUS.get(rep.hbm_status, str(rep.hbm_status)),
        "hbm_bytes_checked": rep.hbm_bytes_checked,
        "hbm_miscompares": rep.hbm_miscompares,
        "hbm_first_bad_offset": rep.hbm_first_bad_offset,
        "kernel_ms": rep.kernel_ms,
        "hbm_ms": rep.hbm_ms,
    }


def selftest_records(device: int = 0, blocks: int = 16, rounds: int = 64,
                     lds_bytes: int = 32768, seed: int = 0) -> List[tuple]:
    """The raw per-wave records of one compute run, in wave order:
    (cu_id, int_sig, fma_sig, mfma_sig, lds_bad)."""
    params = _selftest_params(blocks, rounds, lds_bytes, 0, seed, None)
    n = blocks * 4 if blocks > 0 else 0
    buf = (ctypes.c_uint32 * max(1, n * 5))()
    _check(_lib().egpu_selftest_records(device, ctypes.byref(params), buf, n),
           "egpu_selftest_records")
    return [tuple(buf[5 * i: 5 * i + 5]) for i in range(n)]


def selftest_expected(seed: int = 0, rounds: int = 64) -> List[tuple]:
    """Host reference: (int_sig, fma_sig, mfma_sig) of the 64 patterns. Runs
    no GPU code, so it works on a machine without one."""
    out = (ctypes.c_uint32 * (64 * 3))()
    _check(_lib().egpu_selftest_expected(seed & 0xFFFFFFFF, rounds, out),
           "egpu_selftest_expected")
    return [tuple(out[3 * p: 3 * p + 3]) for p in range(64)]


def selftest_mfma_tile(device: int = 0, pattern: int = 0, seed: int = 0, rounds: int = 1):
    """One wave's MFMA chain: (D, A, B) as nested lists — D 32x32 after
    `rounds` accumulations, A 32x16 and B 16x32 of the last round."""
    d = (ctypes.c_int32 * 1024)()
    a = (ctypes.c_int8 * 512)()
    b = (ctypes.c_int8 * 512)()
    _check(_lib().egpu_selftest_mfma_tile(device, pattern, seed & 0xFFFFFFFF, rounds, d, a, b),
           "egpu_selftest_mfma_tile")
    return ([list(d[32 * i: 32 * i + 32]) for i in range(32)],
            [list(a[16 * i: 16 * i + 16]) for i in range(32)],
            [list(b[32 * i: 32 * i + 32]) for i in range(16)])
