"""Move sweep on a real MI355X (native/egpu_selftest_move.hip) and the health
policy end to end with the real probe child and --move.

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

from elastic_gpu_agent_amd.isolation import health, probes  # noqa: E402

from helpers import Harness  # noqa: E402

SEED = 0x5EED1234
KINDS = list(probes.MOVE_KINDS)
ROUND = 1  # a complement round, and a lane bijection other than round 0's
LANE = np.arange(64)
# source lane of each lane of a 16-lane row: row_mirror after quad_perm:[1,2,3,0],
# and row_half_mirror after row_ror:3
DPP_ROW0 = [12, 15, 14, 13, 8, 11, 10, 9, 4, 7, 6, 5, 0, 3, 2, 1]
DPP_ROW1 = [4, 3, 2, 1, 0, 15, 14, 13, 12, 11, 10, 9, 8, 7, 6, 5]


def _rearranged(kind, src):
    """What the 64 lanes must hold, 64 x 4 words, from the 256 source words:
    written with numpy only, independently of selftest_move_ref.h."""
    s = np.array(src, dtype=np.uint32)
    if kind == "g2l16":  # read back by the mirrored lane
        return s.reshape(64, 4)[::-1]
    if kind == "g2l4":  # read back 32 lanes on
        return np.roll(s.reshape(64, 4), 32, axis=0)
    if kind == "b128":
        return s.reshape(64, 4)[LANE ^ ((LANE >> 3) & 7)]
    if kind.startswith("tr"):
        bits = np.unpackbits(s.view(np.uint8), bitorder="little")
        width = int(kind[2:])
        if width == 6:  # 64 rows of 16 bytes, 16 elements in the first 12; blocks of 16 rows
            got = bits.reshape(4, 16, 128)[:, :, :96].reshape(4, 16, 16, 6).transpose(0, 2, 1, 3)
            got = np.concatenate([got.reshape(64, 96), np.zeros((64, 32), np.uint8)], axis=1)
        else:  # two reads of 512 bytes; per 16 lanes an E x 16 matrix, lane i gets column i
            e = 64 // width
            got = bits.reshape(2, 4, e, 16, width).transpose(1, 3, 0, 2, 4).reshape(64, 128)
        return np.packbits(got, axis=1, bitorder="little").view(np.uint32)
    r = s.reshape(4, 64)  # lane kinds: source register, lane
    if kind == "bperm":
        to = (LANE * ((10 * ROUND + 5) & 63) + ((17 * ROUND + 3) & 63)) & 63
        back = np.argsort(to)
        return np.stack([r[0][to], r[1][to], r[2][back], r[3][back]], axis=1)
    if kind == "swap":
        a, b = r[0].reshape(4, 16), r[1].reshape(4, 16)
        return np.stack([np.concatenate([a[0], b[0], a[2], b[2]]),
                         np.concatenate([a[1], b[1], a[3], b[3]]),
                         np.concatenate([r[2][:32], r[3][:32]]),
                         np.concatenate([r[2][32:], r[3][32:]])], axis=1)
    assert kind == "dpp"
    row = 16 * (LANE // 16)
    bcast15 = list(range(16)) + [15] * 16 + [31] * 16 + [47] * 16
    bcast31 = list(range(32)) + [31] * 32
    return np.stack([r[0][row + np.tile(DPP_ROW0, 4)], r[1][row + np.tile(DPP_ROW1, 4)],
                     r[2][bcast15], r[3][bcast31]], axis=1)


@pytest.mark.parametrize("pattern", [0, 1, 15])
@pytest.mark.parametrize("kind", KINDS)
def test_tile_equals_numpy_rearrangement(kind, pattern):
    regs, src = probes.move_selftest_tile(0, kind, pattern, SEED, ROUND)
    got, want = np.array(regs, dtype=np.uint32), _rearranged(kind, src)
    unmoved = np.array(src, dtype=np.uint32).reshape((4, 64) if kind in ("bperm", "swap", "dpp")
                                                     else (64, 4))
    assert not np.array_equal(want, unmoved if unmoved.shape == (64, 4) else unmoved.T)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"first wrong (lane, register): {bad[:8].tolist()}"


def test_device_signatures_equal_host_reference():
    """4 workgroups = 16 waves = every pattern once."""
    expected4 = probes.move_selftest_expected(SEED, 4)
    recs = probes.move_selftest_records(0, blocks=4, rounds=4, seed=SEED)
    assert len(recs) == 16
    for wave, (cu, sigs) in enumerate(recs):
        assert cu != 0xFFFFFFFF, f"wave {wave} wrote no record"
        assert dict(zip(KINDS, sigs)) == expected4[wave], f"pattern {wave}"
    for wg in range(4):  # the four waves of a workgroup report one CU
        assert len({recs[4 * wg + w][0] for w in range(4)}) == 1


@pytest.mark.parametrize("blocks", [1, 3, 5])
def test_clean_pass_small_grids(blocks):
    rep = probes.move_selftest(0, blocks=blocks, rounds=4, seed=SEED)
    print(rep)
    assert rep["bad_waves"] == 0 and rep["bad_kinds"] == 0 and rep["bad_kind_names"] == []
    assert rep["waves_run"] == 4 * blocks
    assert 1 <= rep["cus_seen"] <= blocks
    assert rep["version"] == 1


@pytest.mark.parametrize("kind", KINDS)
def test_injected_miscompare_is_detected(kind):
    rep = probes.move_selftest(0, blocks=3, rounds=4, seed=SEED, _inject=(kind, 1))
    print(rep)
    assert rep["bad_waves"] == 4
    assert rep["bad_kinds"] == probes.MOVE_KINDS[kind] and rep["bad_kind_names"] == [kind]
    assert rep["n_bad_cus"] == 1 and len(rep["bad_cus"]) == 1


def test_end_to_end_injected_move_failure_reaches_the_reason(tmp_path, monkeypatch):
    monkeypatch.setenv(health.INJECT_ENV, "tr16:0")
    h = Harness(str(tmp_path), gpus=1)
    try:
        result = health.subprocess_runner(0, 120.0, move=True)
        assert result["outcome"] == "report", result
        assert result["report"]["bad_waves"] == 0  # the probe before the sweep is untouched
        rec = health.apply_result(h.storage, 0, result)
        assert rec["state"] == "suspect"
        assert rec["reason"] == "move: 4 bad wave(s) [tr16] on 1 CU(s)"
        assert rec["report"]["move"]["waves_run"] == 4 * health.PERIODIC_MOVE["blocks"]
    finally:
        h.close()
