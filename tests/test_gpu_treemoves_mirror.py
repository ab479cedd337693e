"""`hxtest treemoves`: the C++ mirror's tree-height chain (csrc/host/hx_host_sampler.cpp over hx_history_*) against the
Python layer - the four likelihood parts of the initial history, every step's logAcceptProb recomputed from the printed
trees, the final tree, the move counts."""
import math
import os
import subprocess

import numpy as np
import pytest

from historian_amd import capi, counts, hostmodel
from historian_amd import treesampler as ts
from oracle import c_oracle
from tests.test_gpu_treesampler import PROT4, chain_input

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 60


@pytest.fixture(scope="module", autouse=True)
def engine():
    capi.init(0, c_oracle.table())
    yield
    capi.shutdown()


def _newick(parent, length):
    child = ts.children_of(parent)

    def text(r):
        inner = "(%s)" % ",".join(text(c) for c in child[r]) if child[r] else ""
        return "%sn%d:%s" % (inner, r, repr(float(length[r])))
    return text(len(parent) - 1) + ";"


def test_the_mirrors_chain_against_the_python_layer(tmp_path):
    js, parent, length, rows = chain_input()
    # the Newick reader numbers the nodes in post-order, children left to right: the chain's tree is numbered that way
    with open(tmp_path / "rows.fa", "w") as f:
        for r, row in enumerate(rows):
            f.write(">n%d\n%s\n" % (r, row))
    with open(tmp_path / "tree.nh", "w") as f:
        f.write(_newick(parent, length) + "\n")
    out = subprocess.run([os.path.join(ROOT, "historian_amd", "bin", "hxtest"), "treemoves", str(tmp_path / "rows.fa"), str(tmp_path / "tree.nh"),
                          PROT4, str(STEPS), "11"], capture_output=True, text=True, check=True).stdout
    lines = [l.split() for l in out.splitlines()]
    order = _postorder(parent)                                # mirror node k is our node order[k]
    model = hostmodel.RateModel(js)
    tokens = counts.tokenize_columns(model.alphabet, rows)
    ev = ts.DeviceEvaluator(model, parent, length, tokens)
    sampler = ts.TreeSampler(model, parent, length, rows, ev)
    cll = ev.history.log_like()[1]
    sub_bound = float(np.sum(1e-12 * np.abs(cll) + (np.abs(cll) < 1e-6) * 1e-13)) + len(cll) * 2. ** -53 * float(np.sum(np.abs(cll)))
    parts = [float.fromhex(v) for v in next(l for l in lines if l[0] == "parts")[1:]]
    for got, want in zip(parts[:3], sampler.parts[:3]):
        assert abs(got - want) <= 1e-12 * abs(want)
    print("substitutions: mirror %.17g, Python %.17g, bound %.3g" % (parts[3], sampler.parts[3], sub_bound))
    assert abs(parts[3] - sampler.parts[3]) <= sub_bound
    whole = float.fromhex(next(l for l in lines if l[0] == "whole")[1])
    assert abs(whole - sum(parts)) <= 1e-12 * abs(whole)

    def ours(lengths):
        out = [0.] * len(parent)
        for k, r in enumerate(order):
            out[r] = lengths[k]
        return out

    def log_likelihood(lengths):
        nodes = list(range(len(parent) - 1))
        lp_sub = ev.propose(nodes, [lengths[r] for r in nodes])
        ev.reject()
        return ts.sum_parts(sampler.log_likelihood_parts(lengths, lp_sub))
    current, current_ll = list(length), sampler.log_likelihood
    steps = [(l, lines[k + 1]) for k, l in enumerate(lines) if l[0] == "step"]
    assert len(steps) == STEPS
    tally = {"Node_height": [0, 0], "Rescale": [0, 0]}
    worst = 0.
    for head, proposed in steps:
        kind, node, lap, accepted, log_j, new_ll = head[2], int(head[3]), float.fromhex(head[4]), int(head[5]), float.fromhex(head[6]), float.fromhex(head[7])
        new = ours([float.fromhex(v) for v in proposed[1:]])
        assert ts.is_ultrametric(parent, new, 1e-9)
        want_ll = log_likelihood(new)
        # logAcceptProb = new - old + Jacobian (both proposals are symmetric), each likelihood within the bound of its terms
        bound = 2 * (sub_bound + 1e-12 * (abs(want_ll) + abs(current_ll)))
        assert abs(new_ll - want_ll) <= bound and abs(lap - (want_ll - current_ll + log_j)) <= bound, head
        worst = max(worst, abs(lap - (want_ll - current_ll + log_j)))
        if kind == "Rescale":
            assert node == -1 and abs(log_j) <= math.log(2)
        else:
            assert ts.children_of(parent)[order[node]] and (log_j == 0.) == (order[node] != len(parent) - 1)
        tally[kind][0] += 1
        tally[kind][1] += accepted
        if accepted:
            current, current_ll = new, want_ll
    print("largest |logAcceptProb - (new - old + Jacobian)| over %d steps: %.3g" % (STEPS, worst))
    final = ours([float.fromhex(v) for v in next(l for l in lines if l[0] == "final")[1:]])
    assert final == current and ts.is_ultrametric(parent, final, 1e-9)
    moves = {l[1]: (int(l[2]), int(l[3])) for l in lines if l[0] == "moves"}
    assert sum(p for p, _ in moves.values()) == STEPS and sum(a for _, a in moves.values()) == sum(t[1] for t in tally.values())
    for kind, (p, a) in tally.items():
        assert moves[kind] == (p, a) and p > 5
    assert all(moves[k] == (0, 0) for k in ("Branch_alignment", "Node_alignment", "Prune-and-regraft"))
    ev.close()


def _postorder(parent):
    child = ts.children_of(parent)
    out = []

    def visit(r):
        for c in child[r]:
            visit(c)
        out.append(r)
    visit(len(parent) - 1)
    return out
