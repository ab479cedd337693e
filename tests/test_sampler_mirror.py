"""The host-only parts of the C++ sampler mirror (csrc/host/hx_host_sampler.cpp through bin/testsampler, which makes no
device call) against historian_amd/treesampler.py and tests/history_ref.py: the prior, pairPath, the indel term in path
order, the two proposals on fixed std::mt19937 generators, Move::accept.  `make -C historian_amd/csrc/host sanitize` runs
the same program under AddressSanitizer and UBSan."""
import functools
import math
import os
import subprocess

from historian_amd import hostmodel
from historian_amd import treesampler as ts
from tests import history_ref as HR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL = os.path.join(ROOT, "tests", "golden", "reference_data", "testnj.jukescantor.json")


@functools.lru_cache(maxsize=None)
def output():
    out = subprocess.run([os.path.join(ROOT, "historian_amd", "bin", "testsampler"), MODEL], capture_output=True, text=True, check=True).stdout
    return [line.split() for line in out.splitlines()]


def lines(tag):
    return [l[1:] for l in output() if l[0] == tag]


def tree_of(fields):
    pairs = [f.split(":") for f in fields]
    return [int(p) for p, _ in pairs], [float.fromhex(d) for _, d in pairs]


def test_the_prior_and_the_newick_reader():
    parent, length = tree_of(lines("three")[0])
    assert (parent, length) == ([2, 2, 4, 4, -1], [1., 1., 2., 3., 0.])
    got = [float.fromhex(v) for v in lines("prior")[0]]
    assert got == [-5., -2.5] == [ts.SimpleTreePrior(n).tree_log_likelihood(parent, length) for n in (1., 2.)]


def test_pair_paths_and_the_indel_and_root_terms():
    model = hostmodel.RateModel.load(MODEL)
    parent, length = tree_of(lines("tree")[0])
    assert parent == [2, 2, 6, 5, 5, 6, -1]
    rows = [l[1] for l in lines("row")]
    present = [[ch != "-" for ch in row] for row in rows]
    total, n_terms, mass = 0., 0, 0.
    for fields in lines("pairpath"):
        node = int(fields[0])
        states = HR.pair_path_states(present[parent[node]], present[node])
        assert fields[1] == "".join("MID"[s] for s in states)
        terms = HR.branch_path_terms(ts.trans_prob(model, length[node]), states)
        lp = 0.
        for t in terms:
            lp += t
        assert float.fromhex(fields[2]) == lp                # the same order of the same terms: libm's log on both sides
        total += lp
        n_terms += len(terms)
        mass += sum(abs(t) for t in terms)
    assert {"I", "D"} <= set("".join(f[1] for f in lines("pairpath"))) and "DI" not in "".join(f[1] for f in lines("pairpath"))
    assert float.fromhex(lines("indels")[0][0]) == total
    by_counts = ts.indel_log_likelihood(HR.indel_counts(parent, present), model, length)
    assert abs(by_counts - total) <= 2 * (n_terms + 16) * 2. ** -53 * mass
    assert float.fromhex(lines("root")[0][0]) == ts.root_log_likelihood(model, rows[-1])


def test_the_proposals_on_fixed_generators():
    parent, length = tree_of(lines("tree")[0])
    out = output()
    moves = [(l, out[k + 1]) for k, l in enumerate(out) if l[0] in ("nodeheight", "rescale")]
    roots = others = 0
    for head, proposed in moves:
        assert proposed[0] == "proposed"
        new_parent, new = tree_of(proposed[1:])
        assert new_parent == parent and ts.is_ultrametric(parent, new, 1e-12)
        if head[0] == "rescale":
            log_j = float.fromhex(head[2])
            assert abs(log_j) <= math.log(2) and int(head[4]) == 6
            assert new == [d * math.exp(log_j) for d in length]
            continue
        node, drawn, untouched, log_j = int(head[4]), int(head[6]), int(head[8]), float.fromhex(head[10])
        changed = [int(v) for v in head[12:]]
        # random_element's generator by value: the same node from the generator a second time, which has not advanced
        assert node == drawn and untouched == 1
        left, right = ts.children_of(parent)[node]
        if parent[node] < 0:
            roots += 1
            u = (log_j + math.log(2)) / (2 * math.log(2))
            assert changed == [left, right] and 0 <= u < 1
        else:
            others += 1
            span = max(0., length[node]) + min(length[left], length[right])
            u = new[node] / span
            assert changed == [left, right, node] and log_j == 0. and 0 <= u < 1
        want, want_changed, want_j = ts.node_height_proposal(parent, length, node, u)
        assert want_changed == changed and abs(want_j - log_j) <= 1e-15
        assert all(abs(a - b) <= 4 * 2. ** -53 * max(length) for a, b in zip(want, new))
    assert roots >= 1 and others >= 1


def test_accept_and_the_move_types_drawn():
    a0, a1, _, no_draw, _, minus_inf, _, nullified = lines("accept")[0]
    assert (a0, a1, no_draw, minus_inf, nullified) == ("1", "1", "1", "0", "0")
    seen = [int(v) for v in lines("randomindex")[0]]
    assert seen[:3] == [0, 0, 0] and seen[5] == 0 and seen[3] + seen[4] == 200 and min(seen[3:5]) > 60
