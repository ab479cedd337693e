"""What it costs to make branch DP batches from the device-resident history: hx_history_branch_batch_create (the profiles,
preMultiply and calcInsProbs on the device, nothing through host memory) against the path before it - download the
profiles (hx_history_excluded_profiles), preMultiply and calcInsProbs on the host, upload (hx_branch_batch_create).  The
workload of tools/condpwm_bench.py: 64 leaves / 127 nodes, the 4-component protein mixture, residues at the leaves and
wildcards at the ancestors in every column, at a column count at which the 126 banded (band 20) matrices fit the card.

Per shape - one branch at depth 1, the deepest branch, all N - 1 branches - two variants alternate in one process:

  new     the whole call of History.branch_batch (host clock); its kernels by HIP events (hx_history_last_kernel_ms) and
          their split into profiles / insertion scores / preMultiply (hx_history_last_handoff_ms)
  parent  the whole call of History.excluded_profiles (the download into pageable memory included) plus the whole call of
          capi.BranchBatch on arrays of that size (the upload).  What lies between them, preMultiply and calcInsProbs on
          the host, is timed separately and is NOT part of the comparison: here it is numpy, not the product's host code.

Both variants allocate the same matrices (the batch's cells are allocated at creation and not touched).  One warm-up round,
then `repeats` timed rounds; median [min, max] in ms.  With a fixed order the first call of every round, the one behind the
release of the all-branches batch (gigabytes of matrices), was seen to take 0.2 s whichever it was, so every round starts one
variant further on: such a cost shows in the maxima, not in the medians.  preMultiply's rate is given in picoseconds per table log_sum_exp.

    python tools/branch_handoff_bench.py [columns] [leaves] [repeats] [output file]"""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from historian_amd import capi, hostmodel  # noqa: E402
from oracle import branch_oracle as bo  # noqa: E402
from tools.history_bench import coalescent_tree, stat  # noqa: E402

BAND = 20


def host_inputs(child, log_sub, log_ins, lcw):
    """numpy stand-ins for preMultiply and calcInsProbs (libm's log and exp, not the table): arrays to upload"""
    with np.errstate(divide="ignore", invalid="ignore"):
        terms = log_sub[None, :, :, :] + child[:, :, None, :]
        top = np.max(terms, axis=3, keepdims=True)
        y_sub = top[..., 0] + np.log(np.sum(np.exp(terms - top), axis=3))
        e = (lcw[:, None] + log_ins)[None] + child
        etop = np.max(e, axis=(1, 2), keepdims=True)
        y_emit = etop[:, 0, 0] + np.log(np.sum(np.exp(e - etop), axis=(1, 2)))
    return np.ascontiguousarray(y_sub), np.ascontiguousarray(y_emit)


def main():
    arg = sys.argv[1:]
    n_cols = int(arg[0]) if len(arg) > 0 else 2000
    leaves = int(arg[1]) if len(arg) > 1 else 64
    repeats = int(arg[2]) if len(arg) > 2 else 7
    out_file = arg[3] if len(arg) > 3 else None
    model = hostmodel.RateModel.load(os.path.join(ROOT, "tests", "golden", "models", "prot4.json"))
    rng = np.random.default_rng(3)
    parent, length = coalescent_tree(rng, leaves)
    n, a, c = len(parent), len(model.alphabet), model.components()
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
    trans = bo.trans_scores(0.02, 0.03, 0.4, 0.5)
    log_ins = np.log(ins_prob)
    log_sub = np.log(mats)
    capi.init(0, hostmodel.lse_table())
    h = capi.History(parent, ins_prob, lcw, tok, mats)
    every = list(range(n - 1))
    top = next(r for r in every if depth[r] == 1)
    deep = max(every, key=lambda r: depth[r])
    env = {r: capi.branch_guide_envelope(tok, parent[r], r) for r in every}

    def new_call(nodes):
        branches = [(r, log_sub[:, r], log_ins, trans, env[r][0], env[r][1], BAND) for r in nodes]

        def run():
            t = time.perf_counter()
            b = h.branch_batch(branches)
            ms = 1e3 * (time.perf_counter() - t)
            out = dict(call=ms, kernel=h.kernel_ms(), cells=b.total_cells())
            out["profiles"], out["ins"], out["premultiply"] = h.handoff_ms()
            b.close()
            return out
        return run

    def parent_path(nodes):
        pairs = []
        for r in nodes:
            pairs += [(parent[r], r), (r, parent[r])]

        def run():
            t = time.perf_counter()
            prof = h.excluded_profiles(pairs, normalize=True)
            down = 1e3 * (time.perf_counter() - t)
            t = time.perf_counter()
            jobs = []
            for k, r in enumerate(nodes):
                y_sub, y_emit = host_inputs(prof[2 * k + 1], log_sub[:, r], log_ins, lcw)
                jobs.append((prof[2 * k], y_sub, y_emit, trans, env[r][0], env[r][1], BAND))
            host = 1e3 * (time.perf_counter() - t)
            t = time.perf_counter()
            b = capi.BranchBatch(jobs)
            up = 1e3 * (time.perf_counter() - t)
            b.close()
            return dict(download=down, host=host, upload=up, both=down + up, download_kernel=h.kernel_ms())
        return run

    shapes = [("one branch at depth 1 (node %d)" % top, [top]), ("the deepest branch (node %d, depth %d)" % (deep, depth[deep]), [deep]),
              ("all %d branches" % (n - 1), every)]
    variants = []
    for what, nodes in shapes:
        variants.append((what, nodes, "new", new_call(nodes)))
        variants.append((what, nodes, "parent", parent_path(nodes)))
    results = [dict() for _ in variants]
    for rep in range(repeats + 1):                    # the first round warms up; each round starts one variant further on
        for k in [(rep + q) % len(variants) for q in range(len(variants))]:
            got = variants[k][3]()
            if rep:
                for key, v in got.items():
                    results[k].setdefault(key, []).append(v)
    lines = ["branch_handoff_bench: %d columns, %d leaves / %d nodes, C = %d, A = %d, band %d; %d timed calls per variant after one warm-up, variants alternating"
             % (n_cols, leaves, n, c, a, BAND, repeats),
             "times in ms, median [min, max]; call: host clock around the whole call; kernels: HIP events"]
    for k in range(0, len(variants), 2):
        what, nodes = variants[k][0], variants[k][1]
        new, old = results[k], results[k + 1]
        cells = new["cells"][0]
        inputs = sum(8 * (2 * n_cols * c * a + n_cols) for _ in nodes)
        sums = len(nodes) * n_cols * c * a * a
        pm = statistics.median(new["premultiply"])
        below = statistics.median(new["call"]) < statistics.median(old["both"])
        lines += ["%s: %d cells in the matrices (%.2f GB of state and emission planes at least), %.1f MB of per-position inputs" % (what, cells, 32e-9 * cells, 1e-6 * inputs),
                  "  new:    call %s   kernels %s = profiles %s + insertion scores %s + preMultiply %s" % (
                      stat(new["call"]), stat(new["kernel"]), stat(new["profiles"]), stat(new["ins"]), stat(new["premultiply"])),
                  "          preMultiply: %d table sums, %.2f ps per sum" % (sums, 1e9 * pm / sums),
                  "  parent: download call %s (its kernels %s) + upload call %s = %s   [host preMultiply and calcInsProbs in numpy, not compared: %s]" % (
                      stat(old["download"]), stat(old["download_kernel"]), stat(old["upload"]), stat(old["both"]), stat(old["host"])),
                  "  the new whole call lies %s the parent's download plus upload (medians %.3f against %.3f)" % (
                      "below" if below else "NOT below", statistics.median(new["call"]), statistics.median(old["both"]))]
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
