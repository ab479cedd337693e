"""What the excluded-neighbour profiles of a branch cost on the device-resident history (k_history_excluded in hx_history.hip,
hx_history_excluded_profiles), on the workload of tools/history_bench.py: 64 leaves / 127 nodes x 5000 columns, the
4-component protein mixture, residues at the leaves and wildcards at the ancestors in every column.

  (a) one branch at depth 1 (a child of the root): the two pairs (parent, node), (node, parent)
  (b) the branch above the deepest node
  (c) all N - 1 branches in one call (2 (N - 1) pairs)
  (d) hx_history_propose with every branch on the same history: one full way up, the yardstick

Kernel time by HIP events (hx_history_last_kernel_ms), whole call by the host clock (the download of the profiles into
pageable host memory included); normalised, as the moves ask for them.  One warm-up call per variant, then `repeats` calls
with the variants alternating; median [min, max].  Bytes per branch: what the column kernel and the normalisation must move
at least - per column and component the messages of the siblings along the path and of the kept children ((A + 1) doubles
each: the vector and its scale factor), the two profiles written, read and written again by the normalisation - against
the 8 TB/s of the MI355X's HBM.

    python tools/condpwm_bench.py [columns] [leaves] [repeats] [output file]"""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from historian_amd import capi, hostmodel  # noqa: E402
from historian_amd import treesampler as ts  # noqa: E402
from tools.history_bench import coalescent_tree, stat  # noqa: E402

HBM_BYTES_PER_S = 8e12


def main():
    arg = sys.argv[1:]
    n_cols = int(arg[0]) if len(arg) > 0 else 5000
    leaves = int(arg[1]) if len(arg) > 1 else 64
    repeats = int(arg[2]) if len(arg) > 2 else 7
    out_file = arg[3] if len(arg) > 3 else None
    model = hostmodel.RateModel.load(os.path.join(ROOT, "tests", "golden", "models", "prot4.json"))
    rng = np.random.default_rng(3)
    parent, length = coalescent_tree(rng, leaves)
    n, a, c = len(parent), len(model.alphabet), model.components()
    child = ts.children_of(parent)
    tok = np.full((n_cols, n), -1, dtype=np.int8)
    tok[:, :leaves] = rng.integers(0, a, (n_cols, leaves))
    ins_prob = np.asarray(model.root, dtype=float).reshape(c, a)
    lcw = np.log(np.asarray(model.cpt_weight, dtype=float))
    mats = np.zeros((c, n, a, a))
    for r in range(n - 1):
        mats[:, r] = np.asarray(model.sub_prob(length[r]))
    depth = [0] * n
    for r in range(n - 2, -1, -1):
        depth[r] = depth[parent[r]] + 1
    capi.init(0, hostmodel.lse_table())
    h = capi.History(parent, ins_prob, lcw, tok, mats)
    every = list(range(n - 1))
    scaled = np.ascontiguousarray(np.asarray([model.sub_prob(length[r] * 1.1) for r in every]))
    top = next(r for r in every if depth[r] == 1)
    deep = max(every, key=lambda r: depth[r])

    def pairs_of(nodes):
        out = []
        for r in nodes:
            out += [(parent[r], r), (r, parent[r])]
        return out

    def least_bytes(nodes):
        """per branch: the path to the parent has depth[parent] steps, each reads one sibling; the parent keeps one child, the
        node its own (none at a leaf); 2 profiles written, read and written"""
        total = 0
        for r in nodes:
            messages = depth[parent[r]] + (len(child[parent[r]]) - 1) + len(child[r])
            total += n_cols * c * 8 * (messages * (a + 1) + 3 * 2 * a)
        return total

    def query(nodes):
        pairs = pairs_of(nodes)

        def run():
            t = time.perf_counter()
            out = h.excluded_profiles(pairs, normalize=True)
            return 1e3 * (time.perf_counter() - t), h.kernel_ms(), float(out[0][0, 0, 0])
        return run

    def propose():
        t = time.perf_counter()
        lp = h.propose(every, scaled)
        ms = 1e3 * (time.perf_counter() - t)
        k = h.kernel_ms()
        h.reject()
        return ms, k, lp
    variants = {"a": query([top]), "b": query([deep]), "c": query(every), "d": propose}
    results = {k: ([], []) for k in variants}
    for rep in range(repeats + 1):                    # the first round warms up
        for name, fn in variants.items():
            ms, k, _ = fn()
            if rep:
                results[name][0].append(ms)
                results[name][1].append(k)

    def roof(nodes, name):
        b, k = least_bytes(nodes), statistics.median(results[name][1])
        return "%.1f MB per branch at least, %.0f GB/s, %.1f %% of the HBM roofline" % (b / len(nodes) / 1e6, b / (k * 1e-3) / 1e9, 100 * b / (k * 1e-3) / HBM_BYTES_PER_S)
    lines = ["condpwm_bench: %d columns, %d leaves / %d nodes, C = %d, A = %d; %d timed calls per variant after one warm-up, variants alternating"
             % (n_cols, leaves, n, c, a, repeats),
             "times in ms, median [min, max]; kernel: HIP events around the call's kernels; call: host clock around the whole call (download included)",
             "(a) one branch at depth 1 (node %d):        kernel %s   call %s   %s" % (top, stat(results["a"][1]), stat(results["a"][0]), roof([top], "a")),
             "(b) the deepest branch (node %d, depth %d): kernel %s   call %s   %s" % (deep, depth[deep], stat(results["b"][1]), stat(results["b"][0]), roof([deep], "b")),
             "(c) all %d branches in one call:           kernel %s   call %s   %s" % (n - 1, stat(results["c"][1]), stat(results["c"][0]), roof(every, "c")),
             "(c) per branch: kernel %.3f" % (statistics.median(results["c"][1]) / (n - 1)),
             "(d) propose, all %d branches (one full way up): kernel %s   call %s" % (n - 1, stat(results["d"][1]), stat(results["d"][0]))]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_file:
        os.makedirs(os.path.dirname(os.path.abspath(out_file)), exist_ok=True)
        with open(out_file, "w") as f:
            f.write(text)
    h.close()
    capi.shutdown()


if __name__ == "__main__":
    main()
