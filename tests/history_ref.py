"""TEST INFRASTRUCTURE: what the resident history (hx_history.hip) and the tree sampler (historian_amd/treesampler.py) are
checked against - the sum-product oracle's fill_up behind the sampler's evaluator interface, and a plain restatement of
TreeAlignFuncs::pairPath + ProbModel::getState + logBranchPathLikelihood (reference src/sampler.cpp:150-189, 439-450)."""
import math

import numpy as np

from oracle import historian_oracle as ho
from oracle import sumprod_oracle as so

MATCH, INSERT, DELETE, END = 0, 1, 2, 3


def pair_path_states(parent_present, child_present):
    """the states of pairPath(parent, child), column by column: columns empty in both rows dropped, deletions deferred
    until the next Match (or the end)"""
    out, n_del = [], 0
    for c1, c2 in zip(parent_present, child_present):
        if not (c1 or c2):
            continue
        if c1 and c2:
            out += [DELETE] * n_del + [MATCH]
            n_del = 0
        elif c2:
            out.append(INSERT)
        else:
            n_del += 1
    return out + [DELETE] * n_del


def transition_counts(states):
    """n[src Start/Match, Insert, Delete][dest Match, Insert, Delete, End] of one path, as logBranchPathLikelihood walks it"""
    n = np.zeros((3, 4), dtype=np.int64)
    state = MATCH                                   # (Start has Match's transition probabilities)
    for nxt in states + [END]:
        n[state, nxt] += 1
        state = nxt
    return n


def indel_counts(parent, present):
    """[N][3][4]; present: [N][n_cols] booleans; the root's row is zero"""
    out = np.zeros((len(parent), 3, 4), dtype=np.int64)
    for node, p in enumerate(parent):
        if p >= 0:
            out[node] = transition_counts(pair_path_states(present[p], present[node]))
    return out


def branch_path_terms(tp, states):
    """the terms log(transProb) of logBranchPathLikelihood, in path order; tp: treesampler.trans_prob's table"""
    terms, state = [], MATCH
    for nxt in states + [END]:
        terms.append(math.log(tp[state][nxt]) if tp[state][nxt] > 0 else -math.inf)
        state = nxt
    return terms


def oracle_sub_prob(omodel):
    """t -> [C] matrices exp(R t) as the oracle's SumProduct takes them"""
    return lambda t: [np.asarray(m, dtype=float) for m in ho.ProbModel(omodel, t).sub_mat]


class OracleEvaluator:
    """The sampler's evaluator over oracle.sumprod_oracle: every proposal is a full fill_up of every column."""

    def __init__(self, omodel, parent, length, rows):
        self.omodel, self.parent, self.rows = omodel, list(parent), rows
        self.tree = so.Tree(parent, length, ["n%d" % k for k in range(len(parent))])
        self.sp = so.SumProduct(omodel, self.tree)
        self.sub_prob = oracle_sub_prob(omodel)
        self.columns = list(so.columns_of(self.tree, dict(enumerate(rows))))
        self.present = [[ch not in "-." for ch in row] for row in rows]
        self.cll = self._evaluate()
        self.pending = None

    def _evaluate(self):
        out = []
        for seq in self.columns:
            self.sp.init_column(seq)
            self.sp.fill_up()
            out.append(self.sp.col_log_like)
        return out

    def lp_sub(self):
        return _sum_in_order(self.cll)

    def indel_counts(self):
        return indel_counts(self.parent, self.present)

    def propose(self, nodes, lengths):
        assert self.pending is None
        old = {r: [self.sp.branch_sub[cpt][r] for cpt in range(self.sp.C)] for r in nodes}
        for r, t in zip(nodes, lengths):
            sub = self.sub_prob(t)
            for cpt in range(self.sp.C):
                self.sp.branch_sub[cpt][r] = sub[cpt]
        self.pending = (old, self._evaluate())
        return _sum_in_order(self.pending[1])

    def accept(self):
        self.cll = self.pending[1]
        self.pending = None

    def reject(self):
        for r, mats in self.pending[0].items():
            for cpt, m in enumerate(mats):
                self.sp.branch_sub[cpt][r] = m
        self.pending = None


def _sum_in_order(values):
    """TreeAlignFuncs::substLogLikelihood: lpSub += cll, column by column"""
    s = 0.
    for v in values:
        s += v
    return s


def history_sum(cll):
    """k_history_sum (hx_history.hip) restated: 1024 partial sums, thread t adding the columns t, t + 1024, ... in that
    order from 0., then added pairwise, neighbours first (strides 1, 2, 4 ... 512).  The same bits as the device's lp_sub
    for the same column likelihoods.  (The padding of the last round adds +0., which changes no bit of a sum begun at +0.)"""
    cll = np.asarray(cll, dtype=np.float64)
    rounds = -(-cll.size // 1024)
    padded = np.zeros(rounds * 1024)
    padded[:cll.size] = cll
    part = np.zeros(1024)
    for row in padded.reshape(rounds, 1024):
        part = part + row
    step = 1
    while step < 1024:
        part[::2 * step] = part[::2 * step] + part[step::2 * step]
        step *= 2
    return float(part[0])


def ultrametric_tree(rng, leaves, rate=4.):
    """parent / branch length arrays of a random ultrametric binary tree, children before parents, root last: pairs of
    live lineages joined at increasing heights"""
    parent, height, live, now = [-1] * leaves, [0.] * leaves, list(range(leaves)), 0.
    while len(live) > 1:
        now += float(rng.uniform(.05, 1.)) / rate
        i, j = sorted(rng.choice(len(live), 2, replace=False))
        node = len(parent)
        parent.append(-1)
        height.append(now)
        parent[live[i]] = parent[live[j]] = node
        live = [v for k, v in enumerate(live) if k not in (i, j)] + [node]
    return parent, [height[p] - height[r] if p >= 0 else 0. for r, p in enumerate(parent)]
