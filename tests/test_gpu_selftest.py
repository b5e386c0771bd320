"""GPU self-test kernels on a real MI355X (native/egpu_selftest.hip) and the
health policy end to end with the real probe child.

Shapes are the smallest at which the kernels can still go wrong: rounds=4,
32 KiB of LDS, 1 MiB + 16 B of scratch (a tail that is no multiple of the
grid stride), grids of 1, 3 and 17 workgroups (17: the pattern index wraps
past 64 inside the grid). No test provokes a fault, a hang or a timeout; the
injections corrupt data only.
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
from test_selftest_ref import tile_signature  # noqa: E402

SEED = 0x5EED1234
SMALL = dict(rounds=4, lds_bytes=32768, hbm_bytes=(1 << 20) + 16, seed=SEED)
CHILD_TIMEOUT = 120.0  # of the probe child in the end-to-end tests


@pytest.fixture(scope="module")
def expected4():
    return probes.selftest_expected(SEED, 4)


@pytest.mark.parametrize("blocks", [1, 3, 17])
def test_clean_pass_small_shapes(blocks):
    rep = probes.selftest(0, blocks=blocks, **SMALL)
    print(rep)
    assert rep["bad_waves"] == 0 and rep["bad_kinds"] == 0 and rep["n_bad_cus"] == 0
    assert rep["hbm_miscompares"] == 0 and rep["hbm_status"] == "ok"
    assert rep["hbm_bytes_checked"] == (1 << 20) + 16
    assert rep["waves_run"] == 4 * blocks
    assert 1 <= rep["cus_seen"] <= blocks
    assert rep["lds_bytes"] == 32768 and rep["version"] == 1


def test_full_lds():
    """163,840 B: one workgroup owns the CU's whole LDS."""
    rep = probes.selftest(0, blocks=256, rounds=4, lds_bytes=163840, hbm_bytes=0, seed=SEED)
    print(rep)
    assert rep["lds_bytes"] == 163840
    assert rep["bad_waves"] == 0 and rep["waves_run"] == 4 * 256
    assert rep["hbm_status"] == "off"


def test_larger_grid_reaches_many_cus():
    rep = probes.selftest(0, blocks=2048, rounds=4, lds_bytes=32768, hbm_bytes=0, seed=SEED)
    print("cus_seen", rep["cus_seen"], "kernel_ms", rep["kernel_ms"])
    assert rep["bad_waves"] == 0 and rep["waves_run"] == 4 * 2048
    assert rep["cus_seen"] >= 64  # the bound smoke() uses for the census


@pytest.mark.parametrize("pattern", [0, 1, 63])
def test_mfma_tile_equals_integer_matmul(pattern):
    """rounds=1: D must be exactly A @ B for the A and B the lanes held, so a
    wrong A, B or C/D lane map shows as a wrong tile."""
    d, a, b = probes.selftest_mfma_tile(0, pattern, SEED, 1)
    a, b, d = np.array(a, dtype=np.int64), np.array(b, dtype=np.int64), np.array(d)
    assert a.shape == (32, 16) and b.shape == (16, 32) and d.shape == (32, 32)
    assert np.abs(a).max() <= 3 and np.abs(b).max() <= 3
    assert a.any() and b.any() and not np.array_equal(a @ b, (a @ b).T)  # asymmetric
    assert np.array_equal(d, a @ b)


def test_mfma_chain_matches_reference_signature():
    want = probes.selftest_expected(SEED, 5)
    for pattern in (0, 63):
        d, _, _ = probes.selftest_mfma_tile(0, pattern, SEED, 5)
        assert tile_signature(d) == want[pattern][2]


def test_device_signatures_equal_host_reference(expected4):
    """16 workgroups = 64 waves = every pattern once."""
    recs = probes.selftest_records(0, blocks=16, rounds=4, lds_bytes=32768, seed=SEED)
    assert len(recs) == 64
    for wave, (cu, int_sig, fma_sig, mfma_sig, lds_bad) in enumerate(recs):
        assert cu != 0xFFFFFFFF, f"wave {wave} wrote no record"
        assert int_sig == expected4[wave][0], f"integer chain, pattern {wave}"
        assert fma_sig == expected4[wave][1], f"FMA chain, pattern {wave}"
        assert mfma_sig == expected4[wave][2], f"MFMA chain, pattern {wave}"
        assert lds_bad == 0, f"LDS march, pattern {wave}"
    # the four waves of a workgroup report one CU
    for wg in range(16):
        assert len({recs[4 * wg + w][0] for w in range(4)}) == 1


@pytest.mark.parametrize("kind", ["int", "fma", "mfma", "lds"])
def test_injected_compute_miscompare_is_detected(kind):
    rep = probes.selftest(0, blocks=17, _inject=(kind, 5), **SMALL)
    print(rep)
    assert rep["bad_waves"] == 4
    assert rep["n_bad_cus"] == 1 and len(rep["bad_cus"]) == 1
    assert rep["bad_kinds"] == probes.SELFTEST_KINDS[kind]
    assert rep["bad_kind_names"] == [kind]
    assert rep["waves_run"] == 4 * 17
    assert rep["hbm_miscompares"] == 0


def test_injected_memory_miscompare_is_detected():
    rep = probes.selftest(0, blocks=17, _inject=("hbm", 4096), **SMALL)
    print(rep)
    assert rep["hbm_miscompares"] == 1
    assert rep["hbm_first_bad_offset"] == 4096
    assert rep["hbm_status"] == "failed"
    assert rep["bad_waves"] == 0


def _real_runner(index, timeout, full=False):
    return health.subprocess_runner(index, CHILD_TIMEOUT, full=full)


def test_end_to_end_pass(tmp_path, monkeypatch):
    monkeypatch.delenv(health.INJECT_ENV, raising=False)
    h = Harness(str(tmp_path), gpus=1)
    try:
        m = health.HealthMonitor(h.storage, h.operator, _real_runner, 3600.0)
        out = m.run_once()
        print(out)
        rec = health.get_health(h.storage, 0)
        assert rec["state"] == "ok", rec
        assert rec["report"]["waves_run"] == 4 * health.PERIODIC_PROBE["blocks"]
        assert rec["report"]["hbm_status"] in ("ok", "skipped")
        assert {d["health"] for d in h.plugin.core.list_devices(True)} == {consts.HEALTHY}
    finally:
        h.close()


def test_end_to_end_injected_failure_takes_the_gpu_out(tmp_path, monkeypatch):
    monkeypatch.setenv(health.INJECT_ENV, "mfma")
    h = Harness(str(tmp_path), gpus=1)
    try:
        m = health.HealthMonitor(h.storage, h.operator, _real_runner, 3600.0)
        m.run_once()
        assert health.get_health(h.storage, 0)["state"] == "suspect"
        m.run_once()
        rec = health.get_health(h.storage, 0)
        assert rec["state"] == "unhealthy" and "mfma" in rec["reason"], rec
        for plugin in (h.plugin.core, h.plugin.memory):
            devs = plugin.list_devices(True)
            assert devs and {d["health"] for d in devs} == {consts.UNHEALTHY}
    finally:
        h.close()
