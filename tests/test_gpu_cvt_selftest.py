"""Conversion sweep on a real MI355X (native/egpu_selftest_cvt.hip) and the
health policy end to end with the real probe child and --cvt.

Shapes are the smallest at which the kernels can still go wrong: rounds=2 (one
complement pair of the preserved bits), grids of 1, 3 and 5 workgroups (5: the
pattern index wraps past 16 inside the grid), one wave for the tiles. Every
comparison is bit-exact. No test provokes a fault, a hang or a timeout; the
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

from elastic_gpu_agent_amd.isolation import health, probes  # noqa: E402

from helpers import Harness  # noqa: E402
from test_cvt_ref import reference  # noqa: E402  (numpy float64 only)

SEED = 0x5EED1234
KINDS = list(probes.CVT_KINDS)
ROUND = 1  # a complement round of the preserved bits


@pytest.mark.parametrize("pattern", [0, 1, 15])
@pytest.mark.parametrize("kind", KINDS)
def test_tile_equals_numpy_conversion(kind, pattern):
    src, old, scale, res = probes.cvt_selftest_tile(0, kind, pattern, SEED, ROUND)
    got, want = np.array(res, np.uint32), reference(kind, src, old, scale)
    # register i starts from old word i (zero where the kind preserves nothing)
    used = want.any(axis=0)[:16]
    assert (got[:, :16] != np.array(old, np.uint32))[:, used].any(axis=0).all(), "a no-op leaves old"
    bad = np.argwhere(got != want)
    assert bad.size == 0, "first wrong (lane, register, got, want): " + str(
        [(int(l), int(r), hex(got[l, r]), hex(want[l, r])) for l, r in bad[:8]])


def test_device_signatures_equal_host_reference():
    """4 workgroups = 16 waves = every pattern once."""
    expected = probes.cvt_selftest_expected(SEED, 2)
    recs = probes.cvt_selftest_records(0, blocks=4, rounds=2, seed=SEED)
    assert len(recs) == 16
    for wave, (cu, sigs) in enumerate(recs):
        assert cu != 0xFFFFFFFF, f"wave {wave} wrote no record"
        assert dict(zip(KINDS, sigs)) == expected[wave], f"pattern {wave}"
    for wg in range(4):  # the four waves of a workgroup report one CU
        assert len({recs[4 * wg + w][0] for w in range(4)}) == 1


@pytest.mark.parametrize("blocks", [1, 3, 5])
def test_clean_pass_small_grids(blocks):
    rep = probes.cvt_selftest(0, blocks=blocks, rounds=2, seed=SEED)
    print(rep)
    assert rep["bad_waves"] == 0 and rep["bad_kinds"] == 0 and rep["bad_kind_names"] == []
    assert rep["waves_run"] == 4 * blocks
    assert 1 <= rep["cus_seen"] <= blocks
    assert rep["version"] == 1


@pytest.mark.parametrize("kind", KINDS)
def test_injected_miscompare_is_detected(kind):
    rep = probes.cvt_selftest(0, blocks=3, rounds=2, seed=SEED, _inject=(kind, 1))
    print(rep)
    assert rep["bad_waves"] == 4
    assert rep["bad_kinds"] == probes.CVT_KINDS[kind] and rep["bad_kind_names"] == [kind]
    assert rep["n_bad_cus"] == 1 and len(rep["bad_cus"]) == 1


def test_end_to_end_injected_cvt_failure_reaches_the_reason(tmp_path, monkeypatch):
    monkeypatch.setenv(health.INJECT_ENV, "enc_fp4:0")
    h = Harness(str(tmp_path), gpus=1)
    try:
        result = health.subprocess_runner(0, 120.0, cvt=True)
        assert result["outcome"] == "report", result
        assert result["report"]["bad_waves"] == 0  # the probe before the sweep is untouched
        rec = health.apply_result(h.storage, 0, result)
        assert rec["state"] == "suspect"
        assert rec["reason"] == "cvt: 4 bad wave(s) [enc_fp4] on 1 CU(s)"
        assert rec["report"]["cvt"]["waves_run"] == 4 * health.PERIODIC_CVT["blocks"]
    finally:
        h.close()
