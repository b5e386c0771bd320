"""The atomic sweep's host reference (native/selftest_atomic_ref.h) against an
independent replay of the generator's op list: exact Python ints for the
integer ops, float64 for the FP ones. No GPU.

`reference` and `canon` are also what tests/test_gpu_atomic_selftest.py holds the
device against.
"""
import math
import struct
from collections import defaultdict

import numpy as np
import pytest

from elastic_gpu_agent_amd.isolation import probes

SEED = 0x5EED1234
KINDS = list(probes.ATOMIC_KINDS)
EMPTY = 0xFFFFFFFF
WIDE = {"add64", "fadd64", "fmin64", "fmax64", "add_rtn64", "cas64"}
RETURNING = {"add_rtn32", "add_rtn64", "inc", "dec", "swap", "cas32", "cas64", "claim"}
# format of an FP op: (bits per element, largest whole number up to which all are exact)
FP = {"fadd32": (32, 2 ** 24), "fadd64": (64, 2 ** 53), "pk_f16": (16, 2 ** 11),
      "pk_bf16": (16, 2 ** 8), "fmin64": (64, 2 ** 53), "fmax64": (64, 2 ** 53)}


def decode(op, bits):
    if op == "pk_f16":
        return float(np.array([bits], np.uint16).view(np.float16)[0])
    if op == "pk_bf16":
        return struct.unpack("<f", struct.pack("<I", bits << 16))[0]
    if op == "fadd32":
        return struct.unpack("<f", struct.pack("<I", bits))[0]
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def encode(op, v):
    """v is a whole number the format holds exactly; anything else is a bug."""
    if op == "pk_f16":
        bits = int(np.array([v], np.float16).view(np.uint16)[0])
    elif op == "pk_bf16":
        full = struct.unpack("<I", struct.pack("<f", v))[0]
        assert full & 0xFFFF == 0, f"{v} is not exact in bf16"
        bits = full >> 16
    elif op == "fadd32":
        bits = struct.unpack("<I", struct.pack("<f", v))[0]
    else:
        bits = struct.unpack("<Q", struct.pack("<d", v))[0]
    assert decode(op, bits) == v, f"{v} is not exact in {op}"
    return bits


def halves(op, bits):
    return [bits & 0xFFFF, bits >> 16] if op.startswith("pk_") else [bits]


def signed(v):
    return v - (1 << 32) if v & 0x80000000 else v


def step(op, old, a, b):
    """One atomic: the cell's new value."""
    m = (1 << 64) - 1 if op in WIDE else 0xFFFFFFFF
    if op in ("add32", "add64", "add_rtn32", "add_rtn64"):
        return (old + a) & m
    if op in ("and", "or", "xor"):
        return {"and": old & a, "or": old | a, "xor": old ^ a}[op]
    if op in ("min_i32", "max_i32"):
        return (min if op == "min_i32" else max)(old, a, key=signed)
    if op in ("min_u32", "max_u32"):
        return (min if op == "min_u32" else max)(old, a)
    if op in ("fmin64", "fmax64"):
        return (min if op == "fmin64" else max)(old, a, key=lambda x: decode(op, x))
    if op in FP:
        out = [encode(op, decode(op, x) + decode(op, y)) for x, y in zip(halves(op, old), halves(op, a))]
        return out[0] | (out[1] << 16 if len(out) == 2 else 0)
    if op == "inc":
        return 0 if old >= a else old + 1
    if op == "dec":
        return a if old == 0 or old > a else old - 1
    if op == "swap":
        return a
    assert op in ("cas32", "cas64", "claim"), op
    return a if old == b else old


def reference(init, ops, order=range(probes.ATOMIC_LANES)):
    """Replays the op list, lanes in `order`: (final words, returned[lane][slot])."""
    cells = list(init)
    returned = [[0] * probes.ATOMIC_NSLOT for _ in range(probes.ATOMIC_LANES)]
    for lane in order:
        for slot, (op, cell, a, b) in enumerate(ops[lane]):
            if op == "none":
                continue
            old = cells[cell] | (cells[cell + 1] << 32 if op in WIDE else 0)
            new = step(op, old, a, b)
            cells[cell] = new & 0xFFFFFFFF
            if op in WIDE:
                cells[cell + 1] = new >> 32
            returned[lane][slot] = old if op in RETURNING else 0
    return cells, returned


def canon(ops, returned, final):
    """What does not depend on the order the lanes were served in: the final
    words (a claimed cell: its winner is not determined, so only that every lane
    is consistent with it and exactly one won) and per cell the sorted returned
    values (swap: together with the final value)."""
    final, per_cell = list(final), defaultdict(list)
    for lane in range(probes.ATOMIC_LANES):
        for slot, (op, cell, a, _) in enumerate(ops[lane]):
            if op == "claim":
                got, fin = returned[lane][slot], final[cell]
                per_cell[cell, "won"].append(got == EMPTY)
                assert (fin == a) if got == EMPTY else (fin == got), f"lane {lane} cell {cell}"
            elif op in RETURNING:
                per_cell[cell, op].append(returned[lane][slot])
                if op == "swap" and final[cell] is not None:
                    per_cell[cell, op].append(final[cell])
                    final[cell] = None
    for (cell, what), vals in per_cell.items():
        if what == "won":
            assert sum(vals) == 1, f"cell {cell}: {sum(vals)} winners"
            final[cell] = None
    return final, {k: sorted(v) for k, v in per_cell.items() if k[1] != "won"}


@pytest.mark.parametrize("group", [0, 1, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_header_equals_replay_in_both_lane_orders(kind, group):
    for rnd in (0, 1):
        h = probes.atomic_selftest_ops(kind, group, SEED, rnd)
        want = canon(h["ops"], h["returned"], h["final"])
        fwd = reference(h["init"], h["ops"])
        assert fwd == (h["final"], h["returned"]), "lane order: the header's own order, word for word"
        rev = reference(h["init"], h["ops"], reversed(range(probes.ATOMIC_LANES)))
        assert canon(h["ops"], rev[1], rev[0]) == want, "order independence"
        assert any(op != "none" for lane in h["ops"] for op, *_ in lane)


@pytest.mark.parametrize("kind", ["l_fadd", "g_fadd", "g_grid"])
def test_fp_fan_in_is_bounded_and_operands_are_plain_numbers(kind):
    fans = set()
    for group in range(4):
        for rnd in range(6):
            h = probes.atomic_selftest_ops(kind, group, SEED, rnd)
            total = {}
            lanes = defaultdict(int)
            for lane in h["ops"]:
                for op, cell, a, _ in lane:
                    if op not in FP:
                        continue
                    bits, limit = FP[op]
                    lanes[cell] += 1
                    init = h["init"][cell] | (h["init"][cell + 1] << 32 if op in WIDE else 0)
                    for i, (x, x0) in enumerate(zip(halves(op, a), halves(op, init))):
                        v = decode(op, x)
                        assert math.isfinite(v) and v == int(v) and not (v == 0 and x != 0), (op, hex(x))
                        assert v == 0 or abs(v) >= 1, "no subnormal"
                        assert op not in ("fmin64", "fmax64") or v != 0
                        if (op, cell, i) not in total:  # partial sums start from the initial cell
                            total[op, cell, i] = abs(decode(op, x0))
                        total[op, cell, i] += abs(v)
                        assert total[op, cell, i] <= limit, (op, cell, total[op, cell, i])
            fans |= set(lanes.values())
    assert {1, 2, 4, 16, 64, 128, 256} <= fans or kind == "g_grid", sorted(fans)


def test_cells_stay_inside_their_slot_and_weights_of_rounds_differ():
    for kind in KINDS:
        for group in range(4):
            h = probes.atomic_selftest_ops(kind, group, SEED, 2)
            for lane in h["ops"]:
                for slot, (op, cell, *_) in enumerate(lane):
                    assert 128 * slot <= cell and cell + (2 if op in WIDE else 1) <= 128 * (slot + 1)
    a, b = probes.atomic_selftest_expected(SEED, 2), probes.atomic_selftest_expected(SEED, 4)
    assert len(a) == 16 and all(a[p][k] != b[p][k] for p in range(16) for k in KINDS[:-1])
    assert len({a[p]["l_rtn"] for p in range(16)}) == 16 and all(r["g_grid"] == 0 for r in a)
