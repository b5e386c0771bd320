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
        lib.egpu_mxtest.argtypes = [
            ctypes.c_int, ctypes.POINTER(_MxParams), ctypes.POINTER(_MxReport)
        ]
        lib.egpu_mxtest_records.argtypes = [
            ctypes.c_int, ctypes.POINTER(_MxParams),
            ctypes.POINTER(ctypes.c_uint32), ctypes.c_int,
        ]
        lib.egpu_mxtest_expected.argtypes = [
            ctypes.c_uint32, ctypes.c_int, ctypes.POINTER(ctypes.c_uint32)
        ]
        lib.egpu_mxtest_tile.argtypes = [
            ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_int,
        ] + [ctypes.POINTER(ctypes.c_int32)] * 5
        lib.egpu_mxtest_lane_regs.argtypes = [
            ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_int,
        ] + [ctypes.POINTER(ctypes.c_uint32)] * 4
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


# ---------------------------------------------------------------- matrix sweep

MX_MAX_ROUNDS = 256
MX_PATTERNS = 16
# bad_kinds bits, in the order of the record's signatures
MX_KINDS = {"f16": 1, "i8": 2, "fp8": 4, "bf8": 8, "bf16s": 16,
            "mxfp8": 32, "mxfp6": 64, "mxfp4": 128, "mxmix": 256}
# kind -> (M, K, scaled): the tile is M x M, the operands M x K and K x M
MX_GEOMETRY = {"f16": (32, 16, False), "i8": (32, 32, False), "fp8": (32, 16, False),
               "bf8": (32, 16, False), "bf16s": (16, 32, False), "mxfp8": (32, 64, True),
               "mxfp6": (32, 64, True), "mxfp4": (32, 64, True), "mxmix": (16, 128, True)}
_MX_INDEX = {name: i for i, name in enumerate(MX_KINDS)}


class _MxParams(ctypes.Structure):
    _fields_ = [
        ("blocks", ctypes.c_int32), ("rounds", ctypes.c_int32), ("seed", ctypes.c_uint32),
        ("inject_kind", ctypes.c_int32), ("inject_block", ctypes.c_int32),
    ]


class _MxReport(ctypes.Structure):
    _fields_ = [
        ("version", ctypes.c_uint32), ("waves_run", ctypes.c_uint32),
        ("cus_seen", ctypes.c_uint32), ("bad_waves", ctypes.c_uint32),
        ("bad_kinds", ctypes.c_uint32), ("n_bad_cus", ctypes.c_uint32),
        ("bad_cus", ctypes.c_uint32 * 64), ("kernel_ms", ctypes.c_float),
    ]


def _mx_kind_index(name) -> int:
    if name not in _MX_INDEX:
        raise ValueError(f"unknown matrix kind {name!r}")
    return _MX_INDEX[name]


def _mx_params(blocks, rounds, seed, inject) -> _MxParams:
    kind, block = -1, -1
    if inject is not None:
        kind, block = _mx_kind_index(inject[0]), inject[1]
    return _MxParams(blocks, rounds, seed & 0xFFFFFFFF, kind, block)


def mx_selftest(device: int = 0, blocks: int = 1024, rounds: int = 8, seed: int = 0,
                _inject=None) -> dict:
    """Matrix sweep: every wave of a `blocks`-workgroup grid runs `rounds`
    MFMAs of every kind of MX_KINDS (f16, i8, OCP fp8/bf8, the 16x16 bf16
    shape and the block-scaled fp8/fp6/fp4/mixed forms) and is compared with
    the host reference. Bad arguments raise ProbeError before any HIP call.
    `_inject` = (kind name, workgroup) simulates a miscompare (tests only)."""
    params = _mx_params(blocks, rounds, seed, _inject)
    rep = _MxReport()
    _check(_lib().egpu_mxtest(device, ctypes.byref(params), ctypes.byref(rep)), "egpu_mxtest")
    return {
        "version": rep.version,
        "waves_run": rep.waves_run,
        "cus_seen": rep.cus_seen,
        "bad_waves": rep.bad_waves,
        "bad_kinds": rep.bad_kinds,
        "bad_kind_names": [k for k, bit in MX_KINDS.items() if rep.bad_kinds & bit],
        "n_bad_cus": rep.n_bad_cus,
        "bad_cus": list(rep.bad_cus[: rep.n_bad_cus]),
        "kernel_ms": rep.kernel_ms,
    }


def mx_selftest_records(device: int = 0, blocks: int = 4, rounds: int = 8,
                        seed: int = 0) -> List[tuple]:
    """The raw per-wave records of one sweep, in wave order:
    (cu_id, (signature of every kind, in MX_KINDS order))."""
    params = _mx_params(blocks, rounds, seed, None)
    n = blocks * 4 if blocks > 0 else 0
    w = 1 + len(MX_KINDS)
    buf = (ctypes.c_uint32 * max(1, n * w))()
    _check(_lib().egpu_mxtest_records(device, ctypes.byref(params), buf, n),
           "egpu_mxtest_records")
    return [(buf[w * i], tuple(buf[w * i + 1: w * i + w])) for i in range(n)]


def mx_selftest_expected(seed: int = 0, rounds: int = 8) -> List[dict]:
    """Host reference: for each of the 16 patterns, {kind name: signature}.
    Runs no GPU code, so it works on a machine without one."""
    n = len(MX_KINDS)
    out = (ctypes.c_uint32 * (MX_PATTERNS * n))()
    _check(_lib().egpu_mxtest_expected(seed & 0xFFFFFFFF, rounds, out), "egpu_mxtest_expected")
    return [dict(zip(MX_KINDS, out[n * p: n * p + n])) for p in range(MX_PATTERNS)]


def mx_selftest_tile(device: int = 0, kind: str = "mxfp4", pattern: int = 0, seed: int = 0,
                     rounds: int = 1):
    """One wave's chain of one kind: (D, A, B, SA, SB) as nested lists. D is
    the M x M tile after `rounds` accumulations in hash units (acc*4; i8:
    acc); A (M x K) and B (K x M) are four times the last round's operand
    values; SA (M x K/32) and SB (K/32 x M) are that round's scale exponents
    (all zero, one k-block column, for unscaled kinds)."""
    m, k, scaled = MX_GEOMETRY[kind] if kind in MX_GEOMETRY else (32, 16, False)
    index = _MX_INDEX.get(kind, -1) if isinstance(kind, str) else int(kind)
    d = (ctypes.c_int32 * 1024)()
    a = (ctypes.c_int32 * 2048)()
    b = (ctypes.c_int32 * 2048)()
    sa = (ctypes.c_int32 * 64)()
    sb = (ctypes.c_int32 * 64)()
    _check(_lib().egpu_mxtest_tile(device, index, pattern, seed & 0xFFFFFFFF, rounds,
                                   d, a, b, sa, sb), "egpu_mxtest_tile")
    nkb = k // 32 if scaled else 1

    def rows(buf, nrows, ncols):
        return [list(buf[ncols * i: ncols * i + ncols]) for i in range(nrows)]

    return rows(d, m, m), rows(a, m, k), rows(b, k, m), rows(sa, m, nkb), rows(sb, nkb, m)


def mx_selftest_lane_regs(kind: str, pattern: int = 0, seed: int = 0, round: int = 0):
    """What the 64 lanes hand to the instruction in round `round`, as encoded
    bits: (A, B, SA, SB) with A and B 64 x 8 register words and SA, SB one
    scale word per lane. Host only."""
    a = (ctypes.c_uint32 * 512)()
    b = (ctypes.c_uint32 * 512)()
    sa = (ctypes.c_uint32 * 64)()
    sb = (ctypes.c_uint32 * 64)()
    _check(_lib().egpu_mxtest_lane_regs(_MX_INDEX.get(kind, -1), pattern, seed & 0xFFFFFFFF,
                                        round, a, b, sa, sb), "egpu_mxtest_lane_regs")
    return ([list(a[8 * l: 8 * l + 8]) for l in range(64)],
            [list(b[8 * l: 8 * l + 8]) for l in range(64)], list(sa), list(sb))
