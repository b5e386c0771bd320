"""Matrix sweep on a real MI355X (native/egpu_selftest_mx.hip) and the health
policy end to end with the real probe child and --matrix.

Shapes are the smallest at which the kernels can still go wrong: rounds=4,
grids of 1, 3 and 5 workgroups (5: the pattern index wraps past 16 inside the
grid), one wave for the tiles. No test provokes a fault, a hang or a timeout;
the injections corrupt data only.
"""
import numpy as np
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

from elastic_gpu_agent_amd import consts  # noqa: E402
from elastic_gpu_agent_amd.isolation import health, probes  # noqa: E402

from helpers import Harness  # noqa: E402
from test_mx_ref import mx_tile_signature  # noqa: E402

SEED = 0x5EED1234
KINDS = list(probes.MX_KINDS)
CHILD_TIMEOUT = 120.0  # of the probe child in the end-to-end tests


@pytest.mark.parametrize("blocks", [1, 3, 5])
def test_clean_pass_small_grids(blocks):
    rep = probes.mx_selftest(0, blocks=blocks, rounds=4, seed=SEED)
    print(rep)
    assert rep["bad_waves"] == 0 and rep["bad_kinds"] == 0 and rep["n_bad_cus"] == 0
    assert rep["bad_kind_names"] == []
    assert rep["waves_run"] == 4 * blocks
    assert 1 <= rep["cus_seen"] <= blocks
    assert rep["version"] == 1


@pytest.mark.parametrize("pattern", [0, 1, 15])
@pytest.mark.parametrize("kind", KINDS)
def test_tile_equals_scaled_integer_matmul(kind, pattern):
    """rounds=1: D must be exactly A @ B, every 32-element k-block scaled by
    2^(sa + sb), for the operands and scales the lanes encoded: a wrong A, B
    or C/D lane map, element packing, scale lane or scale byte shows as a
    wrong tile. D is in hash units (acc*4; i8: acc), A and B are four times
    the operand values."""
    m, k, scaled = probes.MX_GEOMETRY[kind]
    d, a, b, sa, sb = (np.array(x, dtype=np.int64)
                       for x in probes.mx_selftest_tile(0, kind, pattern, SEED, 1))
    nkb = k // 32 if scaled else 1
    assert d.shape == (m, m) and a.shape == (m, k) and b.shape == (k, m)
    assert sa.shape == (m, nkb) and sb.shape == (nkb, m)
    assert a.any() and b.any()
    limit = 48 if kind == "i8" else 24  # 4 * 12, 4 * 6
    assert np.abs(a).max() <= limit and np.abs(b).max() <= limit
    want16 = np.zeros((m, m), dtype=np.int64)  # 16 * sum(a * b * scale)
    blk = k // nkb
    for kb in range(nkb):
        part = a[:, kb * blk:(kb + 1) * blk] @ b[kb * blk:(kb + 1) * blk, :]
        e = sa[:, kb][:, None] + sb[kb, :][None, :]
        assert e.min() >= 0 and e.max() <= 2
        want16 += part << e
    assert not np.array_equal(want16, want16.T)  # asymmetric
    assert np.array_equal(d * (16 if kind == "i8" else 4), want16)
    if scaled:
        assert sa.min() != sa.max() and sb.min() != sb.max()  # both da, db values
        assert sa.max() - sa.min() == 1 and sb.max() - sb.min() == 1
    else:
        assert not sa.any() and not sb.any()


@pytest.mark.parametrize("kind", KINDS)
def test_chain_matches_reference_signature(kind):
    want = probes.mx_selftest_expected(SEED, 5)
    for pattern in (0, 15):
        d = probes.mx_selftest_tile(0, kind, pattern, SEED, 5)[0]
        assert mx_tile_signature(kind, d) == want[pattern][kind], f"pattern {pattern}"


def test_device_signatures_equal_host_reference():
    """4 workgroups = 16 waves = every pattern once."""
    expected4 = probes.mx_selftest_expected(SEED, 4)
    recs = probes.mx_selftest_records(0, blocks=4, rounds=4, seed=SEED)
    assert len(recs) == 16
    for wave, (cu, sigs) in enumerate(recs):
        assert cu != 0xFFFFFFFF, f"wave {wave} wrote no record"
        assert len(sigs) == len(KINDS)
        for kind, sig in zip(KINDS, sigs):
            assert sig == expected4[wave][kind], f"{kind}, pattern {wave}"
    # the four waves of a workgroup report one CU
    for wg in range(4):
        assert len({recs[4 * wg + w][0] for w in range(4)}) == 1


@pytest.mark.parametrize("kind", KINDS)
def test_injected_miscompare_is_detected(kind):
    rep = probes.mx_selftest(0, blocks=5, rounds=4, seed=SEED, _inject=(kind, 3))
    print(rep)
    assert rep["bad_waves"] == 4
    assert rep["bad_kinds"] == probes.MX_KINDS[kind]
    assert rep["bad_kind_names"] == [kind]
    assert rep["n_bad_cus"] == 1 and len(rep["bad_cus"]) == 1
    assert rep["waves_run"] == 4 * 5


def _matrix_runner(index, timeout, full=False, matrix=False):
    return health.subprocess_runner(index, CHILD_TIMEOUT, full=full, matrix=matrix)


def test_end_to_end_pass_with_matrix(tmp_path, monkeypatch):
    monkeypatch.delenv(health.INJECT_ENV, raising=False)
    h = Harness(str(tmp_path), gpus=1)
    try:
        m = health.HealthMonitor(h.storage, h.operator, _matrix_runner, 3600.0, matrix=True)
        out = m.run_once()
        print(out)
        rec = health.get_health(h.storage, 0)
        assert rec["state"] == "ok", rec
        assert rec["report"]["matrix"]["waves_run"] == 4 * health.PERIODIC_MATRIX["blocks"]
        assert rec["report"]["matrix"]["bad_waves"] == 0
        assert rec["report"]["waves_run"] == 4 * health.PERIODIC_PROBE["blocks"]
        assert {d["health"] for d in h.plugin.core.list_devices(True)} == {consts.HEALTHY}
    finally:
        h.close()


def test_end_to_end_injected_matrix_failure_takes_the_gpu_out(tmp_path, monkeypatch):
    monkeypatch.setenv(health.INJECT_ENV, "mxfp4")
    h = Harness(str(tmp_path), gpus=1)
    try:
        m = health.HealthMonitor(h.storage, h.operator, _matrix_runner, 3600.0, matrix=True)
        m.run_once()
        assert health.get_health(h.storage, 0)["state"] == "suspect"
        m.run_once()
        rec = health.get_health(h.storage, 0)
        assert rec["state"] == "unhealthy" and "mxfp4" in rec["reason"], rec
        assert rec["reason"].startswith("matrix: 4 bad wave(s) [mxfp4] on 1 CU(s)")
        for plugin in (h.plugin.core, h.plugin.memory):
            devs = plugin.list_devices(True)
            assert devs and {d["health"] for d in devs} == {consts.UNHEALTHY}
    finally:
        h.close()


def test_end_to_end_without_the_flag_has_no_matrix_key(tmp_path, monkeypatch):
    monkeypatch.delenv(health.INJECT_ENV, raising=False)
    h = Harness(str(tmp_path), gpus=1)
    try:
        m = health.HealthMonitor(h.storage, h.operator, _matrix_runner, 3600.0)
        m.run_once()
        rec = health.get_health(h.storage, 0)
        assert rec["state"] == "ok", rec
        assert "matrix" not in rec["report"]
    finally:
        h.close()
