"""Host side of the move sweep (native/selftest_move_ref.h through
libegpu_kernels.so): lane maps, expected signatures and argument checks. None
of it uses a GPU.
"""
import pytest

from elastic_gpu_agent_amd.isolation import probes
from elastic_gpu_agent_amd.isolation.probes import ProbeError

KINDS = list(probes.MOVE_KINDS)


def test_kind_names_and_bits():
    assert KINDS == ["g2l16", "g2l4", "b128", "tr16", "tr8", "tr6", "tr4", "bperm", "swap", "dpp"]
    assert [probes.MOVE_KINDS[k] for k in KINDS] == [1 << i for i in range(len(KINDS))]
    assert not set(KINDS) & (set(probes.MX_KINDS) | set(probes._INJECT_KINDS))
    assert probes.MOVE_PATTERNS == 16


@pytest.mark.parametrize("kind", KINDS)
def test_lane_map_is_a_bijection_inside_the_slab(kind):
    bits, elems, region = probes.MOVE_GEOMETRY[kind]
    lanes = probes.move_selftest_lane_map(kind)
    assert len(lanes) == 64 and all(len(row) == elems for row in lanes)
    assert elems * bits <= 128  # four registers per lane
    assert sorted(i for row in lanes for i in row) == list(range(region))
    # the region lies inside the 256-word tile (tr6 reads 96 bits of every 128)
    assert region * (8 if kind == "tr6" else bits) <= 256 * 32
    assert lanes != [list(range(elems * l, elems * l + elems)) for l in range(64)]  # it moves


@pytest.mark.parametrize("kind", KINDS)
def test_expected_is_stable_and_depends_on_seed_and_rounds(kind):
    a, again = probes.move_selftest_expected(7, 4), probes.move_selftest_expected(7, 4)
    other_seed, five = probes.move_selftest_expected(8, 4), probes.move_selftest_expected(7, 5)
    assert len(a) == probes.MOVE_PATTERNS
    for p in range(probes.MOVE_PATTERNS):
        assert a[p][kind] == again[p][kind]
        assert a[p][kind] != other_seed[p][kind]
        assert a[p][kind] != five[p][kind]
    assert len({a[p][kind] for p in range(probes.MOVE_PATTERNS)}) == probes.MOVE_PATTERNS


@pytest.mark.parametrize("call", [
    lambda: probes.move_selftest(0, blocks=0),
    lambda: probes.move_selftest(0, blocks=65537),
    lambda: probes.move_selftest(0, rounds=0),
    lambda: probes.move_selftest(0, rounds=probes.MOVE_MAX_ROUNDS + 1),
    lambda: probes.move_selftest(0, blocks=2, _inject=("tr8", 2)),
    lambda: probes.move_selftest_records(0, blocks=0),
    lambda: probes.move_selftest_expected(0, 0),
    lambda: probes.move_selftest_expected(0, probes.MOVE_MAX_ROUNDS + 1),
    lambda: probes.move_selftest_tile(0, "nope"),
    lambda: probes.move_selftest_tile(0, "tr16", pattern=16),
    lambda: probes.move_selftest_tile(0, "tr16", pattern=-1),
    lambda: probes.move_selftest_tile(0, "tr16", round=probes.MOVE_MAX_ROUNDS),
    lambda: probes.move_selftest_lane_map("nope"),
])
def test_bad_arguments_raise_before_any_hip_call(call):
    with pytest.raises(ProbeError, match="rc=-1"):
        call()
