"""bench.py contract test: the driver depends on the one-line JSON output."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(300)
def test_bench_json_contract():
    out = subprocess.run(
        [sys.executable, "bench.py", "--steps", "3", "--warmup", "1",
         "--config", "kind-fake"],
        cwd=REPO, capture_output=True, text=True, timeout=280,
    )
    assert out.returncode == 0, out.stderr[-2000:]
    line = out.stdout.strip().splitlines()[-1]
    d = json.loads(line)
    assert d["metric"].startswith("fractional pods/GPU + p50 Allocate()")
    assert d["n_gpus"] == 1
    assert d["steps"] == 3 and d["warmup"] == 1
    assert d["value"] > 0 and d["higher_is_better"] is True
    assert d["scaling"] == "weak"
    assert d["data"] == "synthetic"
    assert d["p50_allocate_us"] > 0
    assert d["ms_per_step"] > 0
    assert "config" in d and d["config"]["pods_per_gpu"] > 0


@pytest.mark.timeout(300)
def test_bench_dump_outputs_repeatable(tmp_path):
    """--dump-outputs: same arguments ⇒ identical arrays run to run (what two
    builds are compared by), float64, one row per pod; --full is accepted and
    leaves the result line's contract intact."""
    import numpy as np

    dumps = []
    for name, extra in (("a", []), ("b", ["--full"])):
        out_dir = tmp_path / name
        out = subprocess.run(
            [sys.executable, "bench.py", "--gpus", "1", "--steps", "2",
             "--warmup", "1", "--config", "kind-fake",
             "--dump-outputs", str(out_dir)] + extra,
            cwd=REPO, capture_output=True, text=True, timeout=280,
        )
        assert out.returncode == 0, out.stderr[-2000:]
        d = json.loads(out.stdout.strip().splitlines()[-1])
        assert d["steps"] == 2 and d["ms_per_step"] > 0
        pods = d["config"]["global_batch"]
        assert sorted(os.listdir(out_dir)) == [
            "allocate_responses.npy", "bindings.npy"]
        arrays = {f: np.load(out_dir / f) for f in os.listdir(out_dir)}
        for a in arrays.values():
            assert a.dtype == np.float64 and a.shape[0] == pods
        assert sum(a.nbytes for a in arrays.values()) <= 64 * 2**20
        dumps.append(arrays)
    for f in dumps[0]:
        assert np.array_equal(dumps[0][f], dumps[1][f]), f
    # the rows describe the same pods: device-set hashes line up, and the
    # mixed plan's core pods carry a CU mask while its memory pods a quota
    resp, bind = dumps[0]["allocate_responses.npy"], dumps[0]["bindings.npy"]
    assert np.array_equal(resp[:, 0], bind[:, 0])
    assert (bind[0::2, 3] > 0).all() and (bind[0::2, 5:].sum(axis=1) > 0).all()
    assert (bind[1::2, 4] > 0).all() and (bind[1::2, 3] == 0).all()


@pytest.mark.timeout(300)
def test_bench_scenarios_run():
    for scenario in ("whole-gpu", "mem-fraction", "compute-fraction"):
        out = subprocess.run(
            [sys.executable, "bench.py", "--steps", "2", "--warmup", "1",
             "--config", scenario],
            cwd=REPO, capture_output=True, text=True, timeout=280,
        )
        assert out.returncode == 0, (scenario, out.stderr[-2000:])
        d = json.loads(out.stdout.strip().splitlines()[-1])
        assert d["config"]["scenario"] == scenario
