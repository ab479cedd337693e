"""Throughput of the maximum-likelihood distance matrix (hx_distance_matrix): a simulated protein alignment of 512 and of 64
sequences x 1000 columns under LG or WAG.  Warm-up and 7 timed calls; the kernels' own duration (HIP events) as median
[min, max]; likelihood evaluations per second; achieved fp64 flop/s, counted as 2 A^3 per A x A product the searches
actually took, against the vector-ALU peak; and the C++ host restatement (HX_HOST_DISTANCES' path) on one core over the
first 512 of the same pairs, extrapolated to all of them.

    python tools/distance_bench.py [lg|wag] [output file]"""
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from historian_amd import capi, hostmodel  # noqa: E402

VECTOR_PEAK = 78.6e12        # fp64 vector-ALU flop/s of an MI355X (README: the figure hx_sumprod is held against)
RUNS = 7


def simulate(model, leaves, cols, rng, branch=.12, gap=.05):
    """rows evolved down a balanced binary tree, every branch `branch` substitutions per site long, then some gaps"""
    p = model.sub_prob(branch)[0]
    cdf = np.cumsum(p / p.sum(axis=1, keepdims=True), axis=1)
    pi = np.asarray(model.root[0])
    level = [rng.choice(len(pi), size=cols, p=pi / pi.sum())]
    while len(level) < leaves:
        nxt = []
        for row in level:
            for _ in range(2):
                u = rng.random(cols)
                nxt.append(np.minimum((u[:, None] > cdf[row]).sum(axis=1), len(pi) - 1))
        level = nxt
    tok = np.stack(level).astype(np.int8)
    tok[rng.random(tok.shape) < gap] = -1
    return tok


def host_ms_per_pair(model_path, alphabet, tok, pairs):
    with tempfile.TemporaryDirectory() as d:
        fa = os.path.join(d, "rows.fa")
        with open(fa, "w") as f:
            for k, row in enumerate(tok):
                f.write(">s%d\n%s\n" % (k, "".join(alphabet[t] if t >= 0 else "-" for t in row)))
        out = subprocess.run([os.path.join(ROOT, "historian_amd", "bin", "hxtest"), "distances", fa, model_path, "100", str(pairs)],
                             stdout=subprocess.PIPE, check=True, env=dict(os.environ, HX_HOST_DISTANCES="1")).stdout.decode()
    return float([l for l in out.splitlines() if l.startswith("hostms")][0].split()[1]) / pairs


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "lg"
    out_path = sys.argv[2] if len(sys.argv) > 2 else None
    model_path = os.path.join(ROOT, "tests", "golden", "models", name + ".json")
    model = hostmodel.RateModel.load(model_path)
    a = len(model.alphabet)
    esr = hostmodel.expected_sub_rate(model)
    rates, weights = np.stack(model.sub_rate), model.cpt_weight
    capi.init(0, hostmodel.lse_table())
    lines = []
    for leaves in (64, 512):
        tok = simulate(model, leaves, 1000, np.random.default_rng(leaves))
        pairs = leaves * (leaves - 1) // 2
        capi.distance_matrix(rates, weights, esr, tok)                       # warm-up
        ms, wall = [], []
        for _ in range(RUNS):
            t0 = time.perf_counter()
            dist, evals = capi.distance_matrix(rates, weights, esr, tok)
            wall.append(1e3 * (time.perf_counter() - t0))
            ms.append(capi.distance_kernel_ms())
        products = capi.distance_products()
        med = float(np.median(ms))
        host = host_ms_per_pair(model_path, model.alphabet, tok, min(512, pairs))
        line = dict(metric="distance_matrix", model=name, sequences=leaves, columns=1000, pairs=pairs, alphabet=a,
                    kernel_ms_median=med, kernel_ms_min=min(ms), kernel_ms_max=max(ms), call_ms_median=float(np.median(wall)),
                    evaluations=int(evals.sum()), evaluations_per_pair=float(evals.mean()),
                    evaluations_per_s=float(evals.sum()) / (med * 1e-3), products=products,
                    fp64_flops_per_s=2. * a ** 3 * products / (med * 1e-3),
                    fraction_of_vector_peak=2. * a ** 3 * products / (med * 1e-3) / VECTOR_PEAK,
                    host_one_core_ms_per_pair=host, host_one_core_s_extrapolated=host * pairs * 1e-3,
                    speedup_over_one_host_core=host * pairs / med, mean_distance=float(dist[np.triu_indices(leaves, 1)].mean()))
        print(json.dumps(line))
        lines.append(json.dumps(line))
    capi.shutdown()
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
