"""bench.py on one GPU: a plain run times the headline alone and --full adds the other blocks; --dump-outputs writes what
the headline path computed in its last timed step, the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--pairs", "5", "--len", "200", "--warmup", "1"]


def run_bench(*extra):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "HX_BENCH_REHEARSE"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + list(extra), cwd=ROOT, env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    lines = [l for l in out.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_plain_run_dumps_the_headline_outputs(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    line = run_bench("--steps", "3", "--dump-outputs", str(a))
    assert line["steps"] == 3 and line["metric"] == "forward-DP cells/s" and line["unit"] == "cells/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f64" and line["value"] > 0
    cells = 5 * 201 * 201
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 - cells) <= 1e-6 * cells
    for k in ("fast_mode", "exact_mode", "scaled_probability_mode", "banded_mode", "strong", "cpu_baseline"):
        assert k not in line, k
    assert sorted(os.listdir(a)) == ["forward_cells_sample.npy", "lp_end.npy"]
    lp = np.load(a / "lp_end.npy")
    assert lp.dtype == np.float64 and lp.shape == (5,) and np.all(np.isfinite(lp)) and lp[0] == line["lp_end_pair0"]
    fc = np.load(a / "forward_cells_sample.npy")
    assert fc.dtype == np.float64 and fc.shape == (5 * 4096, 5) and np.all(np.isfinite(fc))
    # the same arguments: the same inputs, so the same outputs (the number of timed steps does not change them)
    run_bench("--steps", "1", "--dump-outputs", str(b))
    assert np.array_equal(np.load(b / "lp_end.npy"), lp)
    assert np.array_equal(np.load(b / "forward_cells_sample.npy"), fc)


def test_banded_dump_is_finite(tmp_path):
    # under a band the sample stays inside the envelope, where every state of a cell has a finite value
    line = run_bench("--steps", "1", "--band", "20", "--dump-outputs", str(tmp_path))
    lp, fc = np.load(tmp_path / "lp_end.npy"), np.load(tmp_path / "forward_cells_sample.npy")
    assert lp[0] == line["lp_end_pair0"] and np.all(np.isfinite(lp))
    assert fc.shape == (5 * 4096, 5) and np.all(np.isfinite(fc))


def test_full_run_carries_the_other_blocks():
    line = run_bench("--steps", "2", "--full", "--banded-pairs", "4", "--cpu-pairs", "2")
    for k in ("fast_mode", "exact_mode", "scaled_probability_mode"):
        assert line[k]["value"] > 0, k
    assert [b["pairs_per_gpu"] for b in line["banded_mode"]["batches"]] == [4]
    assert line["cpu_baseline"]["value"] > 0 and line["lp_end_max_rel_err_vs_cpu"] <= 1e-4
    assert set(line["lp_end_max_rel_diff_to_exact"]) == {"trunc", "fast", "linear"}
