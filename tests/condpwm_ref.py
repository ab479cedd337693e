"""TEST INFRASTRUCTURE ONLY: SumProduct::logNodeExcludedPostProb (reference src/sumprod.cpp:219-250) and
TreeAlignFuncs::getConditionalPWMs (src/sampler.cpp:356-370) restated over oracle.sumprod_oracle.SumProduct - the profile
of a node given everything on its side of a neighbour and nothing beyond it.

The way down (SumProduct::fillDown, src/sumprod.cpp:163-198) is taken along the one path from the column's root to the node
only: G of a node needs nothing else.  The loop order is the reference's - p = G[rp][i] * sub[i][j], then p *= E[s][i] for
every ungapped sibling, summed over i ascending - with the j of a row carried as one numpy vector (elementwise: the same
roundings).  PINNED by tests/test_oracle_condpwm.py: an enumeration of the wildcard assignments, and the identity that
branchConditionalDump prints (src/sampler.cpp:326-335)."""
import math

import numpy as np

from oracle import historian_oracle as ho
from oracle import sumprod_oracle as so

NEG_INF = -math.inf


def way_down(sp, node):
    """-> G [C][A], logG [C] of `node` (ungapped) in the column sp holds, after init_column and fill_up"""
    t = sp.tree
    path = [node]
    while t.parent[path[-1]] >= 0 and not sp.is_gap(t.parent[path[-1]]):
        path.append(t.parent[path[-1]])
    path.reverse()
    G, logG = [], []
    for cpt in range(sp.C):
        g, lg = sp.ins_prob[cpt].copy(), 0.
        for r in path[1:]:
            sibs = t.siblings(r)
            for s in sibs:
                lg += sp.logE[cpt][s]
            sub = sp.branch_sub[cpt][r]
            gj = np.zeros(sp.A)
            for i in range(sp.A):
                p = g[i] * sub[i]
                for s in sibs:
                    if not sp.is_gap(s):
                        p = p * sp.E[cpt][s][i]
                gj = gj + p
            g = gj
        G.append(g)
        logG.append(lg)
    return G, logG


def scaled_path_reads(sp, node):
    """how many of the scale factors that way_down(sp, node) adds to logG are not 0: logE of a sibling hanging off the path,
    below which fillUp rescaled, per component"""
    t = sp.tree
    reads = 0
    while t.parent[node] >= 0 and not sp.is_gap(t.parent[node]):
        reads += sum(sp.logE[cpt][s] != 0. for cpt in range(sp.C) for s in t.siblings(node))
        node = t.parent[node]
    return reads


def log_node_excluded_post_prob(sp, node, exclude, normalize, down=None):
    """src/sumprod.cpp:219-250, after sp.init_column(seq) and sp.fill_up().  down: way_down(sp, node) if the caller has it.
    -> [C][A] floats"""
    v, norm = _excluded(sp, node, exclude, down)
    if normalize:
        v = [[lp - norm for lp in lpp] for lpp in v]
    return v


def _excluded(sp, node, exclude, down):
    """-> the unnormalised v [C][A] and norm"""
    assert not sp.is_gap(node), "Attempt to find posterior probability of sequence at gapped position"
    t = sp.tree
    parent = t.parent[node]
    assert exclude == parent or t.parent[exclude] == node
    if parent != exclude:
        G, logG = down if down is not None else way_down(sp, node)
    wild = sp.col[node] == so.WILD
    init = [0. if wild else NEG_INF] * sp.A
    if not wild:
        init[sp.tokenize(sp.col[node])] = 0.
    v, norm = [], NEG_INF
    for cpt in range(sp.C):
        lpp = [lp + sp.log_cpt_weight[cpt] for lp in init]
        for child in t.child[node]:
            if child != exclude:
                for i in range(sp.A):
                    lpp[i] += so._log(sp.E[cpt][child][i]) + sp.logE[cpt][child]
        for i in range(sp.A):
            lpp[i] += 0 if parent == exclude else (so._log(G[cpt][i]) + logG[cpt])
            norm = ho.log_sum_exp(norm, lpp[i])
        v.append(lpp)
    return v, norm


def conditional_pwms(sp, rows, pairs, normalize):
    """getConditionalPWMs for a list of (node, excluded neighbour) pairs over the alignment `rows` (one string per node,
    '-' a gap): -> a list of [len(node)][C][A] arrays, row p the node's p-th ungapped column"""
    v, norm, _, _ = conditional_pwms_and_norms(sp, rows, pairs)
    return [a - n[:, None, None] for a, n in zip(v, norm)] if normalize else v


def conditional_pwms_and_norms(sp, rows, pairs):
    """-> the unnormalised profiles (a list of [len][C][A]), the norm of every row (a list of [len]: the normalised profile
    is the one minus the other, the subtraction logNodeExcludedPostProb makes) and how many of the children's messages that
    were read carried a scale factor (logE != 0: one of fillUp's rescalings below them), and how many of the siblings' scale
    factors added to logG on the way down did (scaled_path_reads)"""
    out, norms, scaled, scaled_path = [[] for _ in pairs], [[] for _ in pairs], 0, 0
    for seq in so.columns_of(sp.tree, dict(enumerate(rows))):
        sp.init_column(seq)
        if not sp.ungapped:
            continue
        sp.fill_up()
        downs = {}
        for k, (node, exclude) in enumerate(pairs):
            if sp.is_gap(node):
                continue
            if sp.tree.parent[node] != exclude and node not in downs:
                downs[node] = way_down(sp, node)
            if sp.tree.parent[node] != exclude:
                scaled_path += scaled_path_reads(sp, node)
            v, norm = _excluded(sp, node, exclude, downs.get(node))
            out[k].append(v)
            norms[k].append(norm)
            scaled += sum(sp.logE[cpt][ch] != 0. for cpt in range(sp.C) for ch in sp.tree.child[node] if ch != exclude)
    return ([np.asarray(o, dtype=float).reshape(len(o), sp.C, sp.A) for o in out], [np.asarray(n, dtype=float) for n in norms], scaled,
            scaled_path)


def branch_pairs(parent):
    """the two pairs of every branch, in node order: (parent, node), (node, parent)"""
    pairs = []
    for node, p in enumerate(parent):
        if p >= 0:
            pairs += [(p, node), (node, p)]
    return pairs


def double_caterpillar(leaves):
    """two caterpillars of `leaves` leaves under one root, so that the path to the deepest node of one arm passes a sibling
    that is itself deep (the top of the other arm): arm A is the nodes 0 .. 2 leaves - 2 (leaves first, then the spine from
    the bottom up), arm B the same numbers plus 2 leaves - 1, the root last.  -> parent"""
    arm = [-1] * (2 * leaves - 1)
    arm[0] = arm[1] = leaves
    for k in range(2, leaves):
        arm[k] = leaves + k - 1
        arm[leaves + k - 2] = leaves + k - 1
    n = len(arm)
    parent = [p if p >= 0 else 2 * n for p in arm] + [p + n if p >= 0 else 2 * n for p in arm] + [-1]
    return parent


def double_caterpillar_rows(leaves, inside_a, inside_b, n_cols=4):
    """columns without gaps on double_caterpillar(leaves): unlike residues at the leaves (now and then an 'x'), a wildcard
    at the root, and inside each arm wildcards only ("*": of fillUp's two rescalings only the one at wildcards,
    src/sumprod.cpp:120-124, can fire there) or residues only ("r": only the one at residues, :133-137)"""
    n = 2 * leaves - 1
    rows = []
    for r in range(2 * n):
        a, shift, inside = (r, 0, inside_a) if r < n else (r - n, 2, inside_b)       # (the arms differ)
        if a < leaves:
            rows.append("".join("acgt"[(a + k + shift) % 4] if (a + k) % 7 else "x" for k in range(n_cols)))
        else:
            rows.append("".join("*" if inside == "*" else "acgt"[(a * 3 + k + shift) % 4] for k in range(n_cols)))
    return rows + ["*" * n_cols]


def arm_b_rescalings(sp, leaves):
    """in the column sp holds (after fill_up), on double_caterpillar(leaves): how often each of fillUp's rescaling rules
    fired inside arm B (as tests/test_gpu_history.py's probe counts them) and the scale factor its top sends to the root,
    which the path to any node of arm A adds to logG.  -> wildcard rescalings, residue rescalings, logE [C] of arm B's top"""
    n = 2 * leaves - 1
    wild = residue = 0
    for cpt in range(sp.C):
        for r in range(n, 2 * n):
            f = np.ones(sp.A)
            for ch in sp.tree.child[r]:
                f = f * sp.E[cpt][ch]
            if sp.col[r] == so.WILD:
                wild += float(f.max()) < so.RESCALE_THRESHOLD
            else:
                residue += f[sp.tokenize(sp.col[r])] < so.RESCALE_THRESHOLD
    return wild, residue, [sp.logE[cpt][2 * n - 1] for cpt in range(sp.C)]
