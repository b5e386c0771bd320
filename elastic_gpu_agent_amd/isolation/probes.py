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
        lib.egpu_movetest.argtypes = [
            ctypes.c_int, ctypes.POINTER(_MoveParams), ctypes.POINTER(_MoveReport)
        ]
        lib.egpu_movetest_records.argtypes = [
            ctypes.c_int, ctypes.POINTER(_MoveParams),
            ctypes.POINTER(ctypes.c_uint32), ctypes.c_int,
        ]
        lib.egpu_movetest_expected.argtypes = [
            ctypes.c_uint32, ctypes.c_int, ctypes.POINTER(ctypes.c_uint32)
        ]
        lib.egpu_movetest_tile.argtypes = [
            ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_int,
            ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32),
        ]
        lib.egpu_movetest_lane_map.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int32)]
        lib.egpu_cvttest.argtypes = [
            ctypes.c_int, ctypes.POINTER(_CvtParams), ctypes.POINTER(_CvtReport)
        ]
        lib.egpu_cvttest_records.argtypes = [
            ctypes.c_int, ctypes.POINTER(_CvtParams),
            ctypes.POINTER(ctypes.c_uint32), ctypes.c_int,
        ]
        lib.egpu_cvttest_expected.argtypes = [
            ctypes.c_uint32, ctypes.c_int, ctypes.POINTER(ctypes.c_uint32)
        ]
        lib.egpu_cvttest_tile.argtypes = [
            ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_int,
        ] + [ctypes.POINTER(ctypes.c_uint32)] * 4
        lib.egpu_cvttest_lane_regs.argtypes = [
            ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_int, ctypes.c_int,
        ] + [ctypes.POINTER(ctypes.c_uint32)] * 4
        lib.egpu_atomictest.argtypes = [
            ctypes.c_int, ctypes.POINTER(_AtomicParams), ctypes.POINTER(_AtomicReport)
        ]
        lib.egpu_atomictest_records.argtypes = [
            ctypes.c_int, ctypes.POINTER(_AtomicParams),
            ctypes.POINTER(ctypes.c_uint32), ctypes.c_int,
        ]
        lib.egpu_atomictest_expected.argtypes = [
            ctypes.c_uint32, ctypes.c_int, ctypes.POINTER(ctypes.c_uint32)
        ]
        lib.egpu_atomictest_cells.argtypes = [
            ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_int,
        ] + [ctypes.POINTER(ctypes.c_uint32)] * 3
        lib.egpu_atomictest_ops.argtypes = [
            ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_int,
        ] + [ctypes.POINTER(ctypes.c_uint32)] * 4
        lib.egpu_selftest_hbm.argtypes = [
            ctypes.c_int, ctypes.c_uint64, ctypes.c_uint32,
            ctypes.POINTER(ctypes.c_uint64), ctypes.c_int, ctypes.c_int,
            ctypes.POINTER(_SelftestReport),
        ]
        lib.egpu_selftest_hbm_image.argtypes = [
            ctypes.c_int, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p,
        ]
        lib.egpu_selftest_hbm_words.argtypes = [
            ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)
        ]
        lib.egpu_selftest_lds_words.argtypes = [
            ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)
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
        ("inject_kind", ctypes.c_int32), ("inject_sub", ctypes.c_int32),
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
    kind, arg, sub = 0, 0, 0
    if inject is not None:
        name, arg, *place = inject
        if name not in _INJECT_KINDS:
            raise ValueError(f"unknown injection kind {name!r}")
        kind = _INJECT_KINDS[name]
        if place:
            # inject_sub of egpu_selftest_params: word in bits 0..23, pass above
            word, march_pass = place
            if name != "lds" or not (0 <= word < 1 << 24 and 0 <= march_pass < 128):
                raise ValueError(f"no inject_sub encoding for {inject!r}")
            sub = word | march_pass << 24
    return _SelftestParams(blocks, rounds, seed & 0xFFFFFFFF, lds_bytes, hbm_bytes,
                           kind, sub, arg)


def selftest(device: int = 0, blocks: int = 1024, rounds: int = 64,
             lds_bytes: int = 32768, hbm_bytes: int = 32 << 20, seed: int = 0,
             _inject=None) -> dict:
    """Active self-test: integer, FP32-FMA, MFMA and LDS checks on every wave
    of a `blocks`-workgroup grid against the host reference, then a write /
    verify pattern over `hbm_bytes` of scratch (0 = off). Bad arguments raise
    ProbeError before any HIP call. `_inject` = (kind, arg) simulates a
    miscompare (tests only): kind int/fma/mfma/lds with a workgroup index, or
    hbm with a byte offset. ("lds", wg, word, pass) flips that word of the
    march in that pass (0 = pattern, 1 = complement) instead of word 0 of
    pass 0."""
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
                     lds_bytes: int = 32768, seed: int = 0, _inject=None) -> List[tuple]:
    """The raw per-wave records of one compute run, in wave order:
    (cu_id, int_sig, fma_sig, mfma_sig, lds_bad). `_inject` as for selftest
    (tests only; not hbm, no memory check runs here)."""
    params = _selftest_params(blocks, rounds, lds_bytes, 0, seed, _inject)
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


def _hbm_fields(rep: _SelftestReport) -> dict:
    return {
        "hbm_status": _HBM_STATUS.get(rep.hbm_status, str(rep.hbm_status)),
        "hbm_bytes_checked": rep.hbm_bytes_checked,
        "hbm_miscompares": rep.hbm_miscompares,
        "hbm_first_bad_offset": rep.hbm_first_bad_offset,
        "hbm_ms": rep.hbm_ms,
    }


def selftest_hbm(device: int = 0, hbm_bytes: int = 32 << 20, seed: int = 0,
                 corrupt=(), corrupt_pass: int = 0) -> dict:
    """Tests only: the memory check of selftest() alone, same grid, with bit 0
    of the words at the byte offsets `corrupt` (at most 64, distinct multiples
    of 4 inside the buffer) flipped between the write and the verify of
    `corrupt_pass` (0 = pattern, 1 = complement). Returns the hbm_* fields."""
    offsets = (ctypes.c_uint64 * max(1, len(corrupt)))(*corrupt)
    rep = _SelftestReport()
    _check(_lib().egpu_selftest_hbm(device, hbm_bytes, seed & 0xFFFFFFFF, offsets,
                                    len(corrupt), corrupt_pass, ctypes.byref(rep)),
           "egpu_selftest_hbm")
    return _hbm_fields(rep)


SELFTEST_MAX_IMAGE = (16 << 20) + 16


def selftest_hbm_image(device: int = 0, hbm_bytes: int = (1 << 20) + 16, seed: int = 0,
                       march_pass: int = 0) -> bytes:
    """Tests only: the bytes that the memory check's write launch of
    `march_pass` leaves in a buffer of `hbm_bytes` (at most 16 MiB + 16 B)."""
    ok = 0 < hbm_bytes <= SELFTEST_MAX_IMAGE and hbm_bytes % 16 == 0
    out = ctypes.create_string_buffer(hbm_bytes if ok else 1)  # bad sizes: the library says so
    _check(_lib().egpu_selftest_hbm_image(device, hbm_bytes, seed & 0xFFFFFFFF, march_pass, out),
           "egpu_selftest_hbm_image")
    return out.raw


def selftest_hbm_words(first: int, n: int, seed: int = 0) -> List[int]:
    """Host only: the four words of each of the 16-byte elements
    first .. first+n of the memory check's pattern, in memory order."""
    out = (ctypes.c_uint32 * max(1, 4 * n))()
    _check(_lib().egpu_selftest_hbm_words(first, n, seed & 0xFFFFFFFF, out),
           "egpu_selftest_hbm_words")
    return list(out[: 4 * n])


def selftest_lds_words(first: int, n: int, seed: int = 0) -> List[int]:
    """Host only: words first .. first+n of the LDS march's pattern."""
    out = (ctypes.c_uint32 * max(1, n))()
    _check(_lib().egpu_selftest_lds_words(first, n, seed & 0xFFFFFFFF, out),
           "egpu_selftest_lds_words")
    return list(out[:n])


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


# ---------------------------------------------------------------- move sweep

MOVE_MAX_ROUNDS = 256
MOVE_PATTERNS = 16
# bad_kinds bits, in the order of the record's signatures
MOVE_KINDS = {"g2l16": 1, "g2l4": 2, "b128": 4, "tr16": 8, "tr8": 16, "tr6": 32, "tr4": 64,
              "bperm": 128, "swap": 256, "dpp": 512}
# kind -> (element bits, elements a lane receives per tile through the lane
# map, source elements the map covers). A tile is 256 words; see
# move_selftest_lane_map for how elements are numbered.
MOVE_GEOMETRY = {"g2l16": (32, 4, 256), "g2l4": (32, 4, 256), "b128": (32, 4, 256),
                 "tr16": (16, 8, 512), "tr8": (8, 16, 1024), "tr6": (6, 16, 1024),
                 "tr4": (4, 32, 2048), "bperm": (32, 4, 256), "swap": (32, 4, 256),
                 "dpp": (32, 2, 128)}
_MOVE_INDEX = {name: i for i, name in enumerate(MOVE_KINDS)}

_MoveParams = _MxParams  # {blocks, rounds, seed, inject_kind, inject_block}
_MoveReport = _MxReport


def _move_params(blocks, rounds, seed, inject) -> _MoveParams:
    kind, block = -1, -1
    if inject is not None:
        if inject[0] not in _MOVE_INDEX:
            raise ValueError(f"unknown move kind {inject[0]!r}")
        kind, block = _MOVE_INDEX[inject[0]], inject[1]
    return _MoveParams(blocks, rounds, seed & 0xFFFFFFFF, kind, block)


def move_selftest(device: int = 0, blocks: int = 1024, rounds: int = 4, seed: int = 0,
                  _inject=None) -> dict:
    """Move sweep: every wave of a `blocks`-workgroup grid moves `rounds` slabs
    through every kind of MOVE_KINDS (direct global-to-LDS loads, 128-bit LDS
    accesses, the transposing LDS reads, bpermute/permute, the permlane swaps,
    DPP) and its fold of what the lanes received is compared with the host
    reference. Bad arguments raise ProbeError before any HIP call. `_inject` =
    (kind name, workgroup) simulates a miscompare (tests only)."""
    params = _move_params(blocks, rounds, seed, _inject)
    rep = _MoveReport()
    _check(_lib().egpu_movetest(device, ctypes.byref(params), ctypes.byref(rep)),
           "egpu_movetest")
    return {
        "version": rep.version,
        "waves_run": rep.waves_run,
        "cus_seen": rep.cus_seen,
        "bad_waves": rep.bad_waves,
        "bad_kinds": rep.bad_kinds,
        "bad_kind_names": [k for k, bit in MOVE_KINDS.items() if rep.bad_kinds & bit],
        "n_bad_cus": rep.n_bad_cus,
        "bad_cus": list(rep.bad_cus[: rep.n_bad_cus]),
        "kernel_ms": rep.kernel_ms,
    }


def move_selftest_records(device: int = 0, blocks: int = 4, rounds: int = 4,
                          seed: int = 0) -> List[tuple]:
    """The raw per-wave records of one sweep, in wave order:
    (cu_id, (signature of every kind, in MOVE_KINDS order))."""
    params = _move_params(blocks, rounds, seed, None)
    n = blocks * 4 if blocks > 0 else 0
    w = 1 + len(MOVE_KINDS)
    buf = (ctypes.c_uint32 * max(1, n * w))()
    _check(_lib().egpu_movetest_records(device, ctypes.byref(params), buf, n),
           "egpu_movetest_records")
    return [(buf[w * i], tuple(buf[w * i + 1: w * i + w])) for i in range(n)]


def move_selftest_expected(seed: int = 0, rounds: int = 4) -> List[dict]:
    """Host reference: for each of the 16 patterns, {kind name: signature}.
    Runs no GPU code, so it works on a machine without one."""
    n = len(MOVE_KINDS)
    out = (ctypes.c_uint32 * (MOVE_PATTERNS * n))()
    _check(_lib().egpu_movetest_expected(seed & 0xFFFFFFFF, rounds, out),
           "egpu_movetest_expected")
    return [dict(zip(MOVE_KINDS, out[n * p: n * p + n])) for p in range(MOVE_PATTERNS)]


def move_selftest_tile(device: int = 0, kind: str = "tr16", pattern: int = 0, seed: int = 0,
                       round: int = 0):
    """One wave, one kind, one round, tile 0: (regs, src). regs is 64 lists of
    the 4 register words the lane received (unused ones zero); src the 256
    source words: the LDS tile, the global words of a direct-to-LDS load, or
    for the lane kinds source register r of lane l at 64 * r + l."""
    regs = (ctypes.c_uint32 * 256)()
    src = (ctypes.c_uint32 * 256)()
    _check(_lib().egpu_movetest_tile(device, _MOVE_INDEX.get(kind, -1), pattern,
                                     seed & 0xFFFFFFFF, round, regs, src), "egpu_movetest_tile")
    return [list(regs[4 * l: 4 * l + 4]) for l in range(64)], list(src)


def move_selftest_lane_map(kind: str) -> List[List[int]]:
    """Host only: for each of the 64 lanes, the source element index of every
    element it receives (MOVE_GEOMETRY[kind][1] of them, element j at bit
    j * bits of the lane's registers). Source elements are packed little-endian
    in the tile, except tr6: element k is the 6 bits at bit 6 * (k % 16) of
    the 16-byte row k // 16. bperm: the map of round 0. dpp: registers 0 and 1
    only (2 and 3 are broadcasts)."""
    elems = MOVE_GEOMETRY[kind][1] if kind in MOVE_GEOMETRY else 1
    out = (ctypes.c_int32 * (64 * 32))()
    _check(_lib().egpu_movetest_lane_map(_MOVE_INDEX.get(kind, -1), out),
           "egpu_movetest_lane_map")
    return [list(out[elems * l: elems * l + elems]) for l in range(64)]


# ---------------------------------------------------------------- conversion sweep

CVT_MAX_ROUNDS = 64
CVT_PATTERNS = 16
# bad_kinds bits, in the order of the record's signatures
CVT_KINDS = {"enc_fp8": 1, "enc_bf8": 2, "enc_fp6": 4, "enc_bf6": 8, "enc_fp4": 16,
             "dec_fp8": 32, "dec_bf8": 64, "dec_fp6": 128, "dec_bf6": 256, "dec_fp4": 512,
             "x16": 1024, "plain": 2048}
# registers of a lane: sources, words whose untouched bits must survive, results
CVT_NSRC, CVT_NOLD, CVT_NRES = 32, 16, 32
_CVT_INDEX = {name: i for i, name in enumerate(CVT_KINDS)}

_CvtParams = _MxParams  # {blocks, rounds, seed, inject_kind, inject_block}
_CvtReport = _MxReport


def _cvt_params(blocks, rounds, seed, inject) -> _CvtParams:
    kind, block = -1, -1
    if inject is not None:
        if inject[0] not in _CVT_INDEX:
            raise ValueError(f"unknown conversion kind {inject[0]!r}")
        kind, block = _CVT_INDEX[inject[0]], inject[1]
    return _CvtParams(blocks, rounds, seed & 0xFFFFFFFF, kind, block)


def cvt_selftest(device: int = 0, blocks: int = 1024, rounds: int = 4, seed: int = 0,
                 _inject=None) -> dict:
    """Conversion sweep: every wave of a `blocks`-workgroup grid runs `rounds`
    rounds of every kind of CVT_KINDS (the block-scaled FP8, FP6 and FP4
    quantise and dequantise instructions, their 16-bit forms and the unscaled
    FP8 converts) and its fold of the raw result registers is compared with
    the host reference, bit for bit. Bad arguments raise ProbeError before any
    HIP call. `_inject` = (kind name, workgroup) simulates a miscompare (tests
    only)."""
    params = _cvt_params(blocks, rounds, seed, _inject)
    rep = _CvtReport()
    _check(_lib().egpu_cvttest(device, ctypes.byref(params), ctypes.byref(rep)), "egpu_cvttest")
    return {
        "version": rep.version,
        "waves_run": rep.waves_run,
        "cus_seen": rep.cus_seen,
        "bad_waves": rep.bad_waves,
        "bad_kinds": rep.bad_kinds,
        "bad_kind_names": [k for k, bit in CVT_KINDS.items() if rep.bad_kinds & bit],
        "n_bad_cus": rep.n_bad_cus,
        "bad_cus": list(rep.bad_cus[: rep.n_bad_cus]),
        "kernel_ms": rep.kernel_ms,
    }


def cvt_selftest_records(device: int = 0, blocks: int = 4, rounds: int = 4,
                         seed: int = 0) -> List[tuple]:
    """The raw per-wave records of one sweep, in wave order:
    (cu_id, (signature of every kind, in CVT_KINDS order))."""
    params = _cvt_params(blocks, rounds, seed, None)
    n = blocks * 4 if blocks > 0 else 0
    w = 1 + len(CVT_KINDS)
    buf = (ctypes.c_uint32 * max(1, n * w))()
    _check(_lib().egpu_cvttest_records(device, ctypes.byref(params), buf, n),
           "egpu_cvttest_records")
    return [(buf[w * i], tuple(buf[w * i + 1: w * i + w])) for i in range(n)]


def cvt_selftest_expected(seed: int = 0, rounds: int = 4) -> List[dict]:
    """Host reference: for each of the 16 patterns, {kind name: signature}.
    Runs no GPU code, so it works on a machine without one."""
    n = len(CVT_KINDS)
    out = (ctypes.c_uint32 * (CVT_PATTERNS * n))()
    _check(_lib().egpu_cvttest_expected(seed & 0xFFFFFFFF, rounds, out),
           "egpu_cvttest_expected")
    return [dict(zip(CVT_KINDS, out[n * p: n * p + n])) for p in range(CVT_PATTERNS)]


def _cvt_split(src, old, scale, res):
    return ([list(src[CVT_NSRC * l: CVT_NSRC * (l + 1)]) for l in range(64)],
            [list(old[CVT_NOLD * l: CVT_NOLD * (l + 1)]) for l in range(64)],
            list(scale),
            [list(res[CVT_NRES * l: CVT_NRES * (l + 1)]) for l in range(64)])


def cvt_selftest_tile(device: int = 0, kind: str = "enc_fp8", pattern: int = 0, seed: int = 0,
                      round: int = 0):
    """One wave, one kind, one round on the GPU: (src, old, scale, res), each a
    list over the 64 lanes: the 32 raw source registers, the 16 `old` words,
    the f32 bits of the scale operand and the 32 raw result registers (unused
    registers zero). docs/HEALTH.md says what each kind keeps where."""
    src = (ctypes.c_uint32 * (64 * CVT_NSRC))()
    old = (ctypes.c_uint32 * (64 * CVT_NOLD))()
    scale = (ctypes.c_uint32 * 64)()
    res = (ctypes.c_uint32 * (64 * CVT_NRES))()
    _check(_lib().egpu_cvttest_tile(device, _CVT_INDEX.get(kind, -1), pattern, seed & 0xFFFFFFFF,
                                    round, src, old, scale, res), "egpu_cvttest_tile")
    return _cvt_split(src, old, scale, res)


def cvt_selftest_lane_regs(kind: str, pattern: int = 0, seed: int = 0, round: int = 0):
    """Host only: what the generator emits for every lane and what the host
    reference says the instructions must return, in cvt_selftest_tile's
    shape."""
    src = (ctypes.c_uint32 * (64 * CVT_NSRC))()
    old = (ctypes.c_uint32 * (64 * CVT_NOLD))()
    scale = (ctypes.c_uint32 * 64)()
    res = (ctypes.c_uint32 * (64 * CVT_NRES))()
    u32p = ctypes.POINTER(ctypes.c_uint32)

    def at(buf, word):
        return ctypes.cast(ctypes.byref(buf, 4 * word), u32p)

    for lane in range(64):
        _check(_lib().egpu_cvttest_lane_regs(
            _CVT_INDEX.get(kind, -1), pattern, seed & 0xFFFFFFFF, round, lane,
            at(src, CVT_NSRC * lane), at(old, CVT_NOLD * lane), at(scale, lane),
            at(res, CVT_NRES * lane)), "egpu_cvttest_lane_regs")
    return _cvt_split(src, old, scale, res)


# ---------------------------------------------------------------- atomic sweep

ATOMIC_MAX_ROUNDS = 64
ATOMIC_PATTERNS = 16  # 4 groups (workgroup % 4) x 4 waves
# blocks x rounds up to which a grid-shared f64 cell stays exact
ATOMIC_GRID_MAX_WORK = 699050
# bad_kinds bits, in the order of the record's signatures
ATOMIC_KINDS = {"l_add": 1, "l_logic": 2, "l_rtn": 4, "l_cas": 8, "l_fadd": 16,
                "g_add": 32, "g_logic": 64, "g_rtn": 128, "g_cas": 256, "g_fadd": 512,
                "g_grid": 1024}
# an arena is 1024 words: 8 slots of 128; a workgroup is 256 lanes
ATOMIC_WORDS, ATOMIC_NSLOT, ATOMIC_LANES = 1024, 8, 256
# opcodes of atomic_selftest_ops, in the order of selftest_atomic_ref.h (0: the
# lane sits the slot out)
ATOMIC_OPS = ("none", "add32", "add64", "and", "or", "xor", "min_i32", "max_i32", "min_u32",
              "max_u32", "fadd32", "fadd64", "pk_f16", "pk_bf16", "fmin64", "fmax64",
              "add_rtn32", "add_rtn64", "inc", "dec", "swap", "cas32", "cas64", "claim")
_ATOMIC_INDEX = {name: i for i, name in enumerate(ATOMIC_KINDS)}

_AtomicParams = _MxParams  # {blocks, rounds, seed, inject_kind, inject_block}


class _AtomicReport(ctypes.Structure):
    _fields_ = _MxReport._fields_ + [("grid_bad_cells", ctypes.c_uint32)]


def _atomic_params(blocks, rounds, seed, inject) -> _AtomicParams:
    kind, block = -1, -1
    if inject is not None:
        if inject[0] not in _ATOMIC_INDEX:
            raise ValueError(f"unknown atomic kind {inject[0]!r}")
        kind, block = _ATOMIC_INDEX[inject[0]], inject[1]
    return _AtomicParams(blocks, rounds, seed & 0xFFFFFFFF, kind, block)


def atomic_selftest(device: int = 0, blocks: int = 1024, rounds: int = 4, seed: int = 0,
                    _inject=None) -> dict:
    """Atomic sweep: every workgroup of a `blocks`-workgroup grid runs `rounds`
    rounds of every kind of ATOMIC_KINDS (LDS and global read-modify-write
    atomics under same-address contention) and each wave's fold of the final
    cells and returned words is compared with the host reference, bit for bit;
    the grid-shared cells of g_grid are compared with their closed form
    (`grid_bad_cells`, no CU attributed). Bad arguments raise ProbeError before
    any HIP call. `_inject` = (kind name, workgroup) simulates a miscompare
    (tests only)."""
    params = _atomic_params(blocks, rounds, seed, _inject)
    rep = _AtomicReport()
    _check(_lib().egpu_atomictest(device, ctypes.byref(params), ctypes.byref(rep)),
           "egpu_atomictest")
    return {
        "version": rep.version,
        "waves_run": rep.waves_run,
        "cus_seen": rep.cus_seen,
        "bad_waves": rep.bad_waves,
        "bad_kinds": rep.bad_kinds,
        "bad_kind_names": [k for k, bit in ATOMIC_KINDS.items() if rep.bad_kinds & bit],
        "n_bad_cus": rep.n_bad_cus,
        "bad_cus": list(rep.bad_cus[: rep.n_bad_cus]),
        "kernel_ms": rep.kernel_ms,
        "grid_bad_cells": rep.grid_bad_cells,
    }


def atomic_selftest_records(device: int = 0, blocks: int = 4, rounds: int = 4,
                            seed: int = 0) -> List[tuple]:
    """The raw per-wave records of one sweep, in wave order:
    (cu_id, (signature of every kind, in ATOMIC_KINDS order; g_grid: 0))."""
    params = _atomic_params(blocks, rounds, seed, None)
    n = blocks * 4 if blocks > 0 else 0
    w = 1 + len(ATOMIC_KINDS)
    buf = (ctypes.c_uint32 * max(1, n * w))()
    _check(_lib().egpu_atomictest_records(device, ctypes.byref(params), buf, n),
           "egpu_atomictest_records")
    return [(buf[w * i], tuple(buf[w * i + 1: w * i + w])) for i in range(n)]


def atomic_selftest_expected(seed: int = 0, rounds: int = 4) -> List[dict]:
    """Host reference: for each of the 16 patterns (4 * group + wave),
    {kind name: signature}. Runs no GPU code."""
    n = len(ATOMIC_KINDS)
    out = (ctypes.c_uint32 * (ATOMIC_PATTERNS * n))()
    _check(_lib().egpu_atomictest_expected(seed & 0xFFFFFFFF, rounds, out),
           "egpu_atomictest_expected")
    return [dict(zip(ATOMIC_KINDS, out[n * p: n * p + n])) for p in range(ATOMIC_PATTERNS)]


def _atomic_pairs(buf):
    """256 x NSLOT 64-bit values from their (low, high) words."""
    return [[buf[2 * (ATOMIC_NSLOT * t + s)] | buf[2 * (ATOMIC_NSLOT * t + s) + 1] << 32
             for s in range(ATOMIC_NSLOT)] for t in range(ATOMIC_LANES)]


def atomic_selftest_cells(device: int = 0, kind: str = "l_add", group: int = 0, seed: int = 0,
                          round: int = 0):
    """One workgroup, one kind, one round on the GPU: (init, returned, final).
    init and final are the arena's 1024 words before and after the atomics;
    returned[lane][slot] is what the lane's atomic of that slot returned (0
    where none did)."""
    init = (ctypes.c_uint32 * ATOMIC_WORDS)()
    fin = (ctypes.c_uint32 * ATOMIC_WORDS)()
    ret = (ctypes.c_uint32 * (2 * ATOMIC_NSLOT * ATOMIC_LANES))()
    _check(_lib().egpu_atomictest_cells(device, _ATOMIC_INDEX.get(kind, -1), group,
                                        seed & 0xFFFFFFFF, round, init, ret, fin),
           "egpu_atomictest_cells")
    return list(init), _atomic_pairs(ret), list(fin)


def atomic_selftest_ops(kind: str, group: int = 0, seed: int = 0, round: int = 0) -> dict:
    """Host only: what the generator emits for one workgroup and what the
    header's reference makes of it, lanes applied in order. "ops"[lane][slot]
    is (opcode name, first word of the cell, operand, compare value); "init",
    "returned" and "final" have atomic_selftest_cells' shapes."""
    ops = (ctypes.c_uint32 * (6 * ATOMIC_NSLOT * ATOMIC_LANES))()
    init = (ctypes.c_uint32 * ATOMIC_WORDS)()
    fin = (ctypes.c_uint32 * ATOMIC_WORDS)()
    ret = (ctypes.c_uint32 * (2 * ATOMIC_NSLOT * ATOMIC_LANES))()
    _check(_lib().egpu_atomictest_ops(_ATOMIC_INDEX.get(kind, -1), group, seed & 0xFFFFFFFF,
                                      round, ops, init, ret, fin), "egpu_atomictest_ops")

    def one(t, s):
        w = ops[6 * (ATOMIC_NSLOT * t + s): 6 * (ATOMIC_NSLOT * t + s) + 6]
        return (ATOMIC_OPS[w[0]], w[1], w[2] | w[3] << 32, w[4] | w[5] << 32)

    return {"ops": [[one(t, s) for s in range(ATOMIC_NSLOT)] for t in range(ATOMIC_LANES)],
            "init": list(init), "returned": _atomic_pairs(ret), "final": list(fin)}
