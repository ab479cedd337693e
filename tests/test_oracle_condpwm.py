"""The restatement of SumProduct::logNodeExcludedPostProb (tests/condpwm_ref.py) pinned in two ways that do not share its
code: an enumeration of every assignment of the wildcards on the kept side of the excluded neighbour, and the identity that
branchConditionalDump prints (reference src/sampler.cpp:326-335).  No GPU."""
import itertools
import json
import math
import os
import subprocess

import numpy as np
import pytest

from oracle import historian_oracle as ho
from oracle import sumprod_oracle as so
from tests import condpwm_ref as CR
from tests.test_gpu_ancestors import CYCLIC, PROT4, _recon_columns
from tests.test_gpu_sumprod import _random_model, _random_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _two_component_dna():
    """DNA with two components: CYCLIC and a faster, differently rooted copy of it"""
    fast = {"rootprob": {"a": .4, "c": .3, "g": .2, "t": .1},
            "subrate": {a: {b: 2.5 * r for b, r in row.items()} for a, row in CYCLIC["subrate"].items()}}
    slow = {"rootprob": CYCLIC["rootprob"], "subrate": CYCLIC["subrate"]}
    js = {k: v for k, v in CYCLIC.items() if k not in ("rootprob", "subrate")}
    js["mixture"] = [dict(slow, weight=.7), dict(fast, weight=.3)]
    return js


def _enumerate(sp, node, exclude):
    """[C][A] probabilities: cptWeight[c] * sum over the states of every other ungapped node on node's side of `exclude` of
    the product of the branch probabilities there (and insProb at the column's root if that side holds it), node in
    state i; residues are fixed.  sp holds the column (init_column)."""
    t = sp.tree
    parent = t.parent[node]
    # the kept side: the ungapped nodes reachable from `node` without passing `exclude`
    side, stack = [], [node]
    while stack:
        r = stack.pop()
        side.append(r)
        for nb in t.child[r] + ([t.parent[r]] if t.parent[r] >= 0 else []):
            if nb != exclude and nb not in side and nb not in stack and not sp.is_gap(nb):
                stack.append(nb)
    root = next((r for r in side if t.parent[r] < 0 or sp.is_gap(t.parent[r])), None)
    # the side away from the parent holds the column's root; with the parent excluded the node is the top of its side and
    # gets no prior, not even where the parent is a gap and the node the column's root (src/sumprod.cpp:239-240)
    assert (root is not None) == (parent != exclude or sp.is_gap(parent))
    if parent == exclude:
        assert root in (None, node)
        root = None
    # fillDown does not look at the residue of a node it passes (G = insProb at the column's root, G times the branch below
    # it: src/sumprod.cpp:171, 181 - F is not a factor), so a residue at a strict ancestor of `node` is summed over like a
    # wildcard: that is what the reference computes, and what a reconstruction (wildcards inside) never meets
    above, r = set(), parent
    while r >= 0 and r in side:
        above.add(r)
        r = t.parent[r]
    domain = {r: range(sp.A) if sp.col[r] == so.WILD or r in above else [sp.tokenize(sp.col[r])] for r in side}
    others = [r for r in side if r != node]
    out = np.zeros((sp.C, sp.A))
    for cpt in range(sp.C):
        for i in domain[node]:
            total = 0.
            for states in itertools.product(*[domain[r] for r in others]):
                st = dict(zip(others, states))
                st[node] = i
                p = sp.ins_prob[cpt][st[root]] if root is not None else 1.
                for r in side:
                    if r != root and t.parent[r] in st:
                        p *= sp.branch_sub[cpt][r][st[t.parent[r]]][st[r]]
                total += p
            out[cpt][i] = total * math.exp(sp.log_cpt_weight[cpt])
    return out


def _check_enumeration(js, parent, length, columns):
    model = ho.RateModel(js)
    tree = so.Tree(parent, length, ["n%d" % k for k in range(len(parent))])
    sp = so.SumProduct(model, tree)
    rows = ["".join(col[r] for col in columns) for r in range(len(parent))]
    pairs = CR.branch_pairs(parent)
    seen, worst = 0, 0.
    for seq in so.columns_of(tree, dict(enumerate(rows))):
        sp.init_column(seq)
        sp.fill_up()
        for node, exclude in pairs:
            if sp.is_gap(node):
                continue
            got = np.asarray(CR.log_node_excluded_post_prob(sp, node, exclude, False))
            want = _enumerate(sp, node, exclude)
            assert got.shape == want.shape == (sp.C, sp.A)
            with np.errstate(divide="ignore"):
                lw = np.log(want)
            assert np.array_equal(np.isneginf(got), want == 0.), (seq, node, exclude)
            assert not np.any(np.isnan(got)) and not np.any(np.isposinf(got))
            fin = np.isfinite(got)
            dev = np.abs(got[fin] - lw[fin]) / np.maximum(1., np.abs(lw[fin]))
            worst = max(worst, float(dev.max(initial=0.)))
            assert np.all(dev <= 1e-12), (seq, node, exclude, float(dev.max()))
            seen += 1
    print("enumeration: %d profiles, worst deviation %.3g of 1e-12 max(1, |v|)" % (seen, worst))
    return rows


def test_enumeration_five_nodes_dna_two_components():
    # leaves 0, 1 under node 3; node 3 and leaf 2 under the root 4
    parent, length = [3, 3, 4, 4, -1], [.1, .25, .4, .15, 0.]
    columns = ["acg**",            # residues at the leaves, wildcards inside
               "ac-*-",            # the column's root (3) is below the tree's root
               "a*gc*",            # a leaf wildcard, a residue at an internal node
               "-cg**",            # a gap leaf beside a kept sibling
               "xx-*t",            # leaf wildcards ('x' is no residue), a residue at the root, a gap child of the root
               "--g-*",            # a parent with a single ungapped child
               "t----"]            # one ungapped leaf
    js = _two_component_dna()
    assert ho.RateModel(js).components() == 2
    rows = _check_enumeration(js, parent, length, columns)
    assert rows[4][1] == "-" and rows[3][1] == "*"           # the column whose root is below the tree's root


def test_enumeration_seven_nodes_five_letters():
    rng = np.random.default_rng(11)
    js = _random_model(rng, "acgtu", False)
    parent, length = [4, 4, 5, 5, 6, 6, -1], [.1, .2, .15, .3, .25, .05, 0.]
    columns = ["acgu***",
               "a*gt*c*",            # a leaf wildcard; a residue at an internal node
               "ac--*--",            # the column's root is node 4
               "--gt-*-",            # ... node 5
               "ac-t***",
               "u-c-**g",            # a residue at the tree's root, one child kept under each internal node
               "****a**",            # wildcards at the leaves
               "-c--*-*"]            # a chain: 1 under 4 under 6
    _check_enumeration(js, parent, length, columns)


def test_the_stand_alone_program_of_the_querys_host_code():
    """positions and block offsets, the validation of the pairs, the paths, the output offsets (csrc/hx_history_host.h)"""
    out = subprocess.run([os.path.join(ROOT, "historian_amd", "bin", "testcondpwmhost")], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.splitlines()[-1] == "testcondpwmhost: ok", out.stdout


def _case(name):
    if name == "prot4":
        with open(PROT4) as f:
            js = json.load(f)
        rng = np.random.default_rng(21)
        alphabet = js["alphabet"]
    else:
        js, rng, alphabet = CYCLIC, np.random.default_rng(22), "acgt"
    parent, length = _random_tree(rng, 9)
    return js, parent, length, _recon_columns(rng, parent, alphabet, 130)


@pytest.mark.parametrize("name", ["prot4", "acgt"])
def test_the_identity_branch_conditional_dump_prints(name):
    """the `prot4` and `acgt` cases of tests/test_gpu_history.py (the same seeds, trees and columns): for every branch and
    every column with both its ends ungapped, the two profiles and the branch between them give the column's likelihood"""
    js, parent, length, rows = _case(name)
    model = ho.RateModel(js)
    tree = so.Tree(parent, length, ["n%d" % k for k in range(len(parent))])
    sp = so.SumProduct(model, tree)
    seen, worst = 0, 0.
    for seq in so.columns_of(tree, dict(enumerate(rows))):
        sp.init_column(seq)
        sp.fill_up()
        for node, p in enumerate(parent):
            if p < 0 or sp.is_gap(node) or sp.is_gap(p):
                continue
            p_cond = np.asarray(CR.log_node_excluded_post_prob(sp, p, node, False))
            n_cond = np.asarray(CR.log_node_excluded_post_prob(sp, node, p, False))
            total = -math.inf
            for cpt in range(sp.C):
                with np.errstate(divide="ignore"):
                    terms = p_cond[cpt][:, None] + np.log(sp.branch_sub[cpt][node]) + n_cond[cpt][None, :]
                m = terms.max()
                lse = m + math.log(float(np.exp(terms - m).sum()))
                # the components as the oracle's col_log_like combines them (the table log_sum_exp, in component order)
                total = ho.log_sum_exp(total, lse - sp.log_cpt_weight[cpt])
            worst = max(worst, abs(total - sp.col_log_like))
            assert abs(total - sp.col_log_like) <= 1e-9, (node, seq, total, sp.col_log_like)
            seen += 1
    print("%s: %d (branch, column) identities, worst deviation %.3g" % (name, seen, worst))
    assert seen > 500


@pytest.mark.parametrize("inside", ["wildcards", "residues"])
def test_the_identity_where_the_path_passes_a_deep_sibling(inside):
    """logG with scale factors that are not 0.  Two 48-leaf caterpillars under one root: the path to a node of arm A passes
    the top of arm B, below which fillUp rescaled - at wildcards, or (arm B with residues inside) at residues; the columns
    allow one rule in arm B each.  The identity of branchConditionalDump pins way_down's logG = logG[parent] +
    logE[sibling] against col_log_like, which shares no code with it: on every branch of arm A and the root's two (arm A
    and the root hold wildcards inside; the identity does not hold below a residue, which fillDown does not see)."""
    leaves, arm = 48, 95
    parent = CR.double_caterpillar(leaves)
    rng = np.random.default_rng(48)
    length = [float(rng.uniform(.05, .3)) for _ in parent]
    rows = CR.double_caterpillar_rows(leaves, "*", "*" if inside == "wildcards" else "r")
    tree = so.Tree(parent, length, ["n%d" % k for k in range(len(parent))])
    sp = so.SumProduct(ho.RateModel(CYCLIC), tree)
    branches = list(range(arm)) + [2 * arm - 1]
    seen = scaled = 0
    worst = 0.
    for seq in so.columns_of(tree, dict(enumerate(rows))):
        sp.init_column(seq)
        sp.fill_up()
        wild, residue, top = CR.arm_b_rescalings(sp, leaves)
        assert top[0] != 0. and ((wild >= 1 and residue == 0) if inside == "wildcards" else (residue >= 1 and wild == 0)), (wild, residue, top)
        for node in branches:
            p = parent[node]
            scaled += CR.scaled_path_reads(sp, p)
            p_cond = np.asarray(CR.log_node_excluded_post_prob(sp, p, node, False))
            n_cond = np.asarray(CR.log_node_excluded_post_prob(sp, node, p, False))
            with np.errstate(divide="ignore"):
                terms = p_cond[0][:, None] + np.log(sp.branch_sub[0][node]) + n_cond[0][None, :]
            m = terms.max()
            total = m + math.log(float(np.exp(terms - m).sum())) - sp.log_cpt_weight[0]
            worst = max(worst, abs(total - sp.col_log_like))
            assert abs(total - sp.col_log_like) <= 1e-9, (node, total, sp.col_log_like)
            seen += 1
    print("%s inside arm B: %d identities, worst deviation %.3g; %d scale factors other than 0 along the paths" % (inside, seen, worst, scaled))
    assert seen == 4 * (arm + 1) and scaled >= 4 * (arm - 1)      # every path into arm A adds the scale factor of arm B's top
