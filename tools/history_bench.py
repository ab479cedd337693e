"""What a proposal of a tree-height chain costs on the device-resident history (hx_history.hip), beside the route the
library had before it: 64 leaves x 5000 columns, the 4-component protein mixture, residues at the leaves and wildcards at
the ancestors in every column (no gaps: every column's root is the tree's, so every proposal reaches every column).

  (a) hx_sumprod_ancestors with col_log_like: upload of tokens and matrices, the way up, the way down, the posterior
      combine, download - per proposal; the baseline
  (b) hx_history_propose with every branch (the rescale move)
  (c) hx_history_propose with three branches (the node-height move): at the shallowest and at the deepest internal node
      other than the root (fewest and most ancestors), and the mean over all internal nodes
  (d) proposals per second of a whole TreeSampler.run on the device evaluator, matrices mode (scipy's matrix exponentials on
      the host included)
  (e) hx_history_propose_lengths on the proposals of (b) and (c): the branch lengths go up, k_branch_expm (hx_expm.hip)
      computes exp(R t) in place; kernels, the expm kernel alone (hx_history_last_expm_ms), whole call
  (f) the host's time to build the matrices of (b) and of a three-branch proposal: scipy's expm (model.sub_prob, what (d)
      pays) and the C++ mirror's RateModel::getSubProbMatrix (`hxtest expmtime`)
  (g) (d) in lengths mode, in the same process

One warm-up call per variant, then `repeats` calls with the variants alternating in one process; kernel times by HIP
events (hx_sumprod_last_kernel_ms, hx_history_last_kernel_ms) and whole-call times by the host clock around calls that end
in a synchronise; median [min, max].  The matrices of (a)-(c) are computed before the clock starts.

    python tools/history_bench.py [columns] [leaves] [repeats] [chain steps] [output file]

HX_EXPM_WAVES forces the waves per matrix of k_branch_expm; the output names the setting, so the runs of
several settings, one process each, can be kept in one file one after another (profiles/r11/history_lengths_bench.txt)."""
import os
import random
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from historian_amd import capi, hostmodel  # noqa: E402
from historian_amd import treesampler as ts  # noqa: E402


def coalescent_tree(rng, leaves):
    """a random ultrametric binary tree, children before parents, root last"""
    parent, height, live, now = [-1] * leaves, [0.] * leaves, list(range(leaves)), 0.
    while len(live) > 1:
        now += float(rng.uniform(.01, .05))
        i, j = sorted(rng.choice(len(live), 2, replace=False))
        parent.append(-1)
        height.append(now)
        parent[live[i]] = parent[live[j]] = len(parent) - 1
        live = [v for k, v in enumerate(live) if k not in (i, j)] + [len(parent) - 1]
    return parent, [height[p] - height[r] if p >= 0 else 0. for r, p in enumerate(parent)]


def stat(values):
    return "%.3f [%.3f, %.3f]" % (statistics.median(values), min(values), max(values))


def main():
    arg = sys.argv[1:]
    n_cols = int(arg[0]) if len(arg) > 0 else 5000
    leaves = int(arg[1]) if len(arg) > 1 else 64
    repeats = int(arg[2]) if len(arg) > 2 else 7
    chain_steps = int(arg[3]) if len(arg) > 3 else 200
    out_file = arg[4] if len(arg) > 4 else None
    model = hostmodel.RateModel.load(os.path.join(ROOT, "tests", "golden", "models", "prot4.json"))
    rng = np.random.default_rng(3)
    parent, length = coalescent_tree(rng, leaves)
    n, a, c = len(parent), len(model.alphabet), model.components()
    child = ts.children_of(parent)
    tok = np.full((n_cols, n), -1, dtype=np.int8)
    tok[:, :leaves] = rng.integers(0, a, (n_cols, leaves))
    ins_prob = np.asarray(model.root, dtype=float).reshape(c, a)
    lcw = np.log(np.asarray(model.cpt_weight, dtype=float))

    def matrices(lengths):
        out = np.zeros((c, n, a, a))
        for r in range(n - 1):
            out[:, r] = np.asarray(model.sub_prob(lengths[r]))
        return out
    capi.init(0, hostmodel.lse_table())
    current = matrices(length)
    scaled = [t * 1.1 for t in length]
    scaled_all = matrices(scaled)
    every = list(range(n - 1))
    scaled_list = np.ascontiguousarray(scaled_all[:, every].transpose(1, 0, 2, 3))
    depth = [0] * n
    for r in range(n - 2, -1, -1):
        depth[r] = depth[parent[r]] + 1
    internal = [r for r in range(n - 1) if child[r]]
    triples = {r: [child[r][0], child[r][1], r] for r in internal}
    triple_mats = {r: np.ascontiguousarray(scaled_all[:, triples[r]].transpose(1, 0, 2, 3)) for r in internal}
    shallow, deep = min(internal, key=lambda r: depth[r]), max(internal, key=lambda r: depth[r])
    t0 = time.perf_counter()
    h = capi.History(parent, ins_prob, lcw, tok, current)
    create_ms, create_kernel = 1e3 * (time.perf_counter() - t0), h.kernel_ms()
    h.set_rates(np.asarray(model.sub_rate, dtype=float))
    expm_ms = {}

    def run_a():
        t = time.perf_counter()
        cll, _, _ = capi.sumprod_ancestors(parent, ins_prob, lcw, scaled_all, tok)
        return 1e3 * (time.perf_counter() - t), capi.sumprod_kernel_ms(), float(np.sum(cll))

    def propose(nodes, mats):
        t = time.perf_counter()
        lp = h.propose(nodes, mats)
        ms = 1e3 * (time.perf_counter() - t)
        k = h.kernel_ms()
        h.reject()
        return ms, k, lp

    def propose_lengths(name, nodes):
        lengths = [scaled[r] for r in nodes]
        t = time.perf_counter()
        lp = h.propose_lengths(nodes, lengths)
        ms = 1e3 * (time.perf_counter() - t)
        k = h.kernel_ms()
        expm_ms.setdefault(name, []).append(h.expm_ms())
        h.reject()
        return ms, k, lp
    variants = {"a": run_a, "b": lambda: propose(every, scaled_list), "c shallowest": lambda: propose(triples[shallow], triple_mats[shallow]),
                "c deepest": lambda: propose(triples[deep], triple_mats[deep]),
                "e all": lambda: propose_lengths("e all", every), "e shallowest": lambda: propose_lengths("e shallowest", triples[shallow]),
                "e deepest": lambda: propose_lengths("e deepest", triples[deep])}
    results = {k: ([], []) for k in variants}
    values = {}
    for rep in range(repeats + 1):                    # the first round warms up
        for name, fn in variants.items():
            ms, k, value = fn()
            values[name] = value
            if rep:
                results[name][0].append(ms)
                results[name][1].append(k)
    # (c) over every internal node: one warm-up round, then one timed proposal each, `repeats` rounds
    per_node = {r: ([], []) for r in internal}
    for rep in range(repeats + 1):
        for r in internal:
            ms, k, _ = propose(triples[r], triple_mats[r])
            if rep:
                per_node[r][0].append(ms)
                per_node[r][1].append(k)
    mean_call = statistics.mean(statistics.median(v[0]) for v in per_node.values())
    mean_kernel = statistics.mean(statistics.median(v[1]) for v in per_node.values())
    mean_walked = statistics.mean(3 + depth[r] for r in internal)
    per_node_e = {r: ([], []) for r in internal}
    for rep in range(repeats + 1):
        for r in internal:
            ms, k, _ = propose_lengths("e nodes", triples[r])
            if rep:
                per_node_e[r][0].append(ms)
                per_node_e[r][1].append(k)
    mean_call_e = statistics.mean(statistics.median(v[0]) for v in per_node_e.values())
    mean_kernel_e = statistics.mean(statistics.median(v[1]) for v in per_node_e.values())
    # (f) the host's exponentials: scipy (one warm-up, then `repeats` timed builds), the mirror (one process, 10 rounds of each)
    def scipy_ms(nodes):
        out = []
        for rep in range(repeats + 1):
            t = time.perf_counter()
            for r in nodes:
                model.sub_prob(scaled[r])
            out.append(1e3 * (time.perf_counter() - t))
        return out[1:]
    scipy_all, scipy_three = scipy_ms(every), scipy_ms(triples[deep])
    hxtest = os.path.join(ROOT, "historian_amd", "bin", "hxtest")
    mirror = subprocess.run([hxtest, "expmtime", os.path.join(ROOT, "tests", "golden", "models", "prot4.json"), repr(statistics.median(scaled[:-1])),
                             str(10 * (n - 1))], capture_output=True, text=True, check=True).stdout.split()
    mirror_per_branch = float(mirror[3]) / int(mirror[1])
    # (d) a whole chain
    ev = ts.DeviceEvaluator(model, parent, length, tok, mode="matrices")
    rows = ["x" * n_cols] * n                          # (the sampler reads the root's row for its length only)
    sampler = ts.TreeSampler(model, parent, length, rows, ev)
    sampler.run(10, random.Random(1))
    t0 = time.perf_counter()
    sampler.run(chain_steps, random.Random(2))
    chain_s = time.perf_counter() - t0
    # (g) the same chain in lengths mode
    lev = ts.DeviceEvaluator(model, parent, length, tok, mode="lengths")
    lsampler = ts.TreeSampler(model, parent, length, rows, lev)
    lsampler.run(10, random.Random(1))
    t0 = time.perf_counter()
    lsampler.run(chain_steps, random.Random(2))
    lchain_s = time.perf_counter() - t0
    lev.close()
    lines = ["history_bench: %d columns, %d leaves / %d nodes, C = %d, A = %d; %d timed calls per variant after one warm-up, variants alternating"
             % (n_cols, leaves, n, c, a, repeats),
             "times in ms, median [min, max]; kernel: HIP events around the call's kernels; call: host clock around the whole call",
             "k_branch_expm's waves per matrix: %s" % ("HX_EXPM_WAVES=" + os.environ["HX_EXPM_WAVES"] if os.environ.get("HX_EXPM_WAVES") else "the library's plan (HX_EXPM_WAVES not set)"),
             "create (full evaluation, upload included): call %.3f, kernel %.3f" % (create_ms, create_kernel),
             "(a) hx_sumprod_ancestors, col_log_like:   kernel %s   call %s" % (stat(results["a"][1]), stat(results["a"][0])),
             "(b) propose, all %d branches:            kernel %s   call %s" % (n - 1, stat(results["b"][1]), stat(results["b"][0])),
             "(c) propose, 3 branches, node %d (%d nodes recomputed): kernel %s   call %s"
             % (shallow, 3 + depth[shallow], stat(results["c shallowest"][1]), stat(results["c shallowest"][0])),
             "(c) propose, 3 branches, node %d (%d nodes recomputed): kernel %s   call %s"
             % (deep, 3 + depth[deep], stat(results["c deepest"][1]), stat(results["c deepest"][0])),
             "(c) mean over the %d internal nodes of the per-node medians (%.1f nodes recomputed on average): kernel %.3f   call %.3f"
             % (len(internal), mean_walked, mean_kernel, mean_call),
             "(d) TreeSampler.run, %d steps: %.1f proposals per second (%s)" % (chain_steps, chain_steps / chain_s, sampler.move_stats().strip().replace("\n", "; ")),
             "sum of the column log-likelihoods: (a) %.12g, (b) %.12g" % (values["a"], values["b"]),
             "(e) propose_lengths, all %d branches (%d matrices):   kernel %s   of which k_branch_expm %s   call %s"
             % (n - 1, c * (n - 1), stat(results["e all"][1]), stat(expm_ms["e all"][1:]), stat(results["e all"][0])),
             "(e) propose_lengths, 3 branches (%d matrices), node %d: kernel %s   of which k_branch_expm %s   call %s"
             % (3 * c, shallow, stat(results["e shallowest"][1]), stat(expm_ms["e shallowest"][1:]), stat(results["e shallowest"][0])),
             "(e) propose_lengths, 3 branches (%d matrices), node %d: kernel %s   of which k_branch_expm %s   call %s"
             % (3 * c, deep, stat(results["e deepest"][1]), stat(expm_ms["e deepest"][1:]), stat(results["e deepest"][0])),
             "(e) mean over the %d internal nodes of the per-node medians: kernel %.3f   call %.3f   (k_branch_expm, median of all: %.3f)"
             % (len(internal), mean_kernel_e, mean_call_e, statistics.median(expm_ms["e nodes"][len(internal):])),
             "(f) host, the %d branches' matrices: scipy expm %s; 3 branches: %s; the mirror's getSubProbMatrix %.3f per branch (%.3f for %d, %.3f for 3)"
             % (n - 1, stat(scipy_all), stat(scipy_three), mirror_per_branch, mirror_per_branch * (n - 1), n - 1, 3 * mirror_per_branch),
             "(g) TreeSampler.run in lengths mode, %d steps: %.1f proposals per second (%s)"
             % (chain_steps, chain_steps / lchain_s, lsampler.move_stats().strip().replace("\n", "; ")),
             "sum of the column log-likelihoods: (e) %.12g" % values["e all"]]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_file:
        os.makedirs(os.path.dirname(os.path.abspath(out_file)), exist_ok=True)
        with open(out_file, "w") as f:
            f.write(text)
    ev.close()
    h.close()
    capi.shutdown()


if __name__ == "__main__":
    main()
