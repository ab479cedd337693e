"""Ancestor prediction (hx_sumprod_ancestors) on the shape of tools/sumprod_bench.py: 100 000 columns on a balanced tree of
16 leaves / 31 nodes with the 4-component protein mixture, residues at the leaves and wildcards at the ancestors.  Timed
twice - `best` only, and with node_post - beside hx_sumprod_columns(want_root_post=True) on the same tokens in the same
process: the kernels' duration (HIP events, hx_sumprod_last_kernel_ms) and the whole call (upload + kernels + download).
One warm-up call per variant, then `repeats` calls with the variants alternating; medians.

    python tools/ancestors_bench.py [columns] [leaves] [repeats]"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from historian_amd import capi, counts, hostmodel  # noqa: E402
from tools.sumprod_bench import balanced  # noqa: E402


def main():
    n_cols = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
    leaves = int(sys.argv[2]) if len(sys.argv) > 2 else 16
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    model = hostmodel.RateModel.load(os.path.join(ROOT, "tests", "golden", "models", "prot4.json"))
    rng = np.random.default_rng(3)
    parent, length = balanced(leaves, rng)
    n, a, c = len(parent), len(model.alphabet), model.components()
    tok = rng.integers(0, a, (n_cols, n)).astype(np.int8)
    tok[:, leaves:] = -1
    capi.init(0, hostmodel.lse_table())
    cc = counts.ColumnCounter(model, parent, length)
    ap = counts.AncestorPredictor(model, parent, length, branch_sub=[[cc.branch_sub[k, r] for k in range(c)] for r in range(n)])
    variants = {"ancestors_best": lambda: ap.run(tok), "ancestors_best_and_post": lambda: ap.run(tok, want_post=True),
                "counts_with_root_post": lambda: cc.run(tok, want_root_post=True)}
    kernel = {k: [] for k in variants}
    wall = {k: [] for k in variants}
    out = {}
    for k, f in variants.items():                      # warm-up: code objects, allocations
        out[k] = f()
    for _ in range(repeats):
        for k, f in variants.items():
            t0 = time.perf_counter()
            f()
            wall[k].append(time.perf_counter() - t0)
            kernel[k].append(capi.sumprod_kernel_ms())
    # the two entry points agree where they overlap
    assert np.array_equal(out["ancestors_best"]["best"], out["ancestors_best_and_post"]["best"])
    np.testing.assert_allclose(out["ancestors_best"]["col_log_like"], out["counts_with_root_post"]["col_log_like"], rtol=1e-12)
    n_wild = int((tok == -1).sum())
    # per component: E and G of every internal node but the root (2 A^2 each; a residue leaf's G is never made); the counts
    # call adds G of the leaves, U and D
    flops = c * 2 * (n - leaves - 1) * 2 * a * a
    scratch = 8 * c * (n * a + 2 * (n - leaves) * a + 3 * n)          # E; G and terms of the wildcards; scale factors: written once
    line = dict(metric="ancestor_columns_per_s", columns=n_cols, nodes=n, components=c, alphabet=a, wildcard_cells=n_wild,
                repeats=repeats, flops_per_column=flops, scratch_bytes_written_per_column=scratch)
    for k in variants:
        ms = statistics.median(kernel[k])
        line[k] = dict(kernel_ms_median=ms, kernel_ms_min=min(kernel[k]), kernel_ms_max=max(kernel[k]),
                       call_ms_median=1e3 * statistics.median(wall[k]), columns_per_s_kernel=n_cols / (ms * 1e-3))
    line["kernel_time_vs_counts"] = line["ancestors_best"]["kernel_ms_median"] / line["counts_with_root_post"]["kernel_ms_median"]
    print(json.dumps(line))
    capi.shutdown()


if __name__ == "__main__":
    main()
