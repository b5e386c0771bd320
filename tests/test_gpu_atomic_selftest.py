"""Atomic sweep on a real MI355X (native/egpu_selftest_atomic.hip) and the
health policy end to end with the real probe child and --atomic.

Shapes are the smallest at which the kernels can still go wrong: rounds=2 (one
complement pair), grids of 1, 3 and 5 workgroups (5: the group index wraps
inside the grid and the groups contribute unequally to g_grid), one workgroup
for the cells. Every comparison is bit-exact. No test provokes a fault, a hang
or a timeout; the injections corrupt data only.
"""
import pytest

pytestmark = pytest.mark.gpu


def _gpu_present():
    try:
        import torch

        return torch.cuda.is_available()
    except Exception:
        return False


if not _gpu_present():
    pytest.skip("no AMD GPU present", allow_module_level=True)

from elastic_gpu_agent_amd.isolation import health, probes  # noqa: E402

from helpers import Harness  # noqa: E402
from test_atomic_ref import canon, reference  # noqa: E402  (Python ints and float64 only)

SEED = 0x5EED1234
KINDS = list(probes.ATOMIC_KINDS)
ROUND = 1  # a complement round


@pytest.mark.parametrize("group", [0, 1, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_cells_equal_replay(kind, group):
    host = probes.atomic_selftest_ops(kind, group, SEED, ROUND)
    init, returned, final = probes.atomic_selftest_cells(0, kind, group, SEED, ROUND)
    assert init == host["init"], "plain stores of the initial cells"
    want_final, want_returned = reference(init, host["ops"])
    got, want = canon(host["ops"], returned, final), canon(host["ops"], want_returned, want_final)
    bad = [(w, hex(g), hex(e)) for w, (g, e) in enumerate(zip(got[0], want[0])) if g != e]
    assert not bad, "first wrong (word, got, want): " + str(bad[:8])
    assert got[1] == want[1], "returned values per cell"


def test_device_signatures_equal_host_reference():
    """4 workgroups = every group once = every pattern once."""
    expected = probes.atomic_selftest_expected(SEED, 2)
    recs = probes.atomic_selftest_records(0, blocks=4, rounds=2, seed=SEED)
    assert len(recs) == 16
    for wave, (cu, sigs) in enumerate(recs):
        assert cu != 0xFFFFFFFF, f"wave {wave} wrote no record"
        assert dict(zip(KINDS, sigs)) == expected[wave], f"pattern {wave}"
    for wg in range(4):  # the four waves of a workgroup report one CU
        assert len({recs[4 * wg + w][0] for w in range(4)}) == 1


@pytest.mark.parametrize("blocks", [1, 3, 5])
def test_clean_pass_small_grids(blocks):
    rep = probes.atomic_selftest(0, blocks=blocks, rounds=2, seed=SEED)
    print(rep)
    assert rep["bad_waves"] == 0 and rep["bad_kinds"] == 0 and rep["bad_kind_names"] == []
    assert rep["grid_bad_cells"] == 0
    assert rep["waves_run"] == 4 * blocks
    assert 1 <= rep["cus_seen"] <= blocks
    assert rep["version"] == 1


@pytest.mark.parametrize("kind", KINDS)
def test_injected_miscompare_is_detected(kind):
    rep = probes.atomic_selftest(0, blocks=3, rounds=2, seed=SEED, _inject=(kind, 1))
    print(rep)
    assert rep["bad_kinds"] == probes.ATOMIC_KINDS[kind] and rep["bad_kind_names"] == [kind]
    if kind == "g_grid":
        assert rep["grid_bad_cells"] == 1 and rep["bad_waves"] == 0 and rep["n_bad_cus"] == 0
    else:
        assert rep["bad_waves"] == 4 and rep["grid_bad_cells"] == 0
        assert rep["n_bad_cus"] == 1 and len(rep["bad_cus"]) == 1


def test_end_to_end_injected_atomic_failure_reaches_the_reason(tmp_path, monkeypatch):
    monkeypatch.setenv(health.INJECT_ENV, "l_fadd:0")
    h = Harness(str(tmp_path), gpus=1)
    try:
        result = health.subprocess_runner(0, 120.0, atomic=True)
        assert result["outcome"] == "report", result
        assert result["report"]["bad_waves"] == 0  # the probe before the sweep is untouched
        rec = health.apply_result(h.storage, 0, result)
        assert rec["state"] == "suspect"
        assert rec["reason"] == "atomic: 4 bad wave(s) [l_fadd] on 1 CU(s)"
        assert rec["report"]["atomic"]["waves_run"] == 4 * health.PERIODIC_ATOMIC["blocks"]
    finally:
        h.close()
