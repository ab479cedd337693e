"""Tree-height MCMC on a fixed alignment: the reference's Sampler restricted to the moves that need nothing but the
likelihood of a whole history (reference src/sampler.cpp).

  SimpleTreePrior.tree_log_likelihood          src/sampler.cpp:13-31
  root_log_likelihood                          src/sampler.cpp:372-380
  indel_log_likelihood (count form)            src/sampler.cpp:382-392, 439-450 with ProbModel::transProb (src/model.cpp:400-447)
  node_height_proposal / rescale_proposal      NodeHeightMove, RescaleMove (src/sampler.cpp:927-1003)
  TreeSampler.accept / sample / run            Move::accept (541-557), Sampler::sample / run (1678-1734)

A history is a tree (parent and branch-length arrays, children before parents, the root last) and one gapped row per node.
Its log-likelihood is tree prior + root + indels + substitutions (TreeAlignFuncs::logLikelihood, src/sampler.cpp:409-417).
The alignment is fixed, so the indel transition counts of every branch are taken once and the indel term of a proposed
tree is sum n * log(transProb) over them; the substitution term comes from an injected evaluator:

  evaluator.lp_sub()                  the current sum of the column log-likelihoods
  evaluator.indel_counts()            [N][3][4] integers, n[src Start/Match, Insert, Delete][dest Match, Insert, Delete, End]
  evaluator.propose(nodes, lengths)   the sum for the tree in which the branches above `nodes` have the new `lengths`
  evaluator.accept() / reject()       keep or drop that proposal

DeviceEvaluator is the product's: capi.History (hx_history.hip), which takes the rate matrices once and the changed
branches' lengths per proposal (or, given a sub_prob callable, that callable's matrices for the changed branches).  The
tests inject a CPU evaluator over the sum-product oracle, so the sampler's logic is checked without a GPU.

NOT built: prune-and-regraft and the alignment moves (BranchAlign, NodeAlign).  Their rates are 0 here, where the reference
gives them 1 each against 2 for NodeHeight and 2 for Rescale: this is the chain of a run with a fixed alignment and a
fixed topology.  Random numbers come from any generator with .random() -> [0, 1); they are not the reference's
std::mt19937 streams (the C++ mirror, csrc/host/hx_host_sampler.cpp, keeps those)."""
import math

import numpy as np

from . import capi

BRANCH_ALIGN, NODE_ALIGN, PRUNE_AND_REGRAFT, NODE_HEIGHT, RESCALE = range(5)
MOVE_NAMES = ("Branch alignment", "Node alignment", "Prune-and-regraft", "Node height", "Rescale")
NEG_INF = float("-inf")


def distance_from_root(parent, length):
    """Tree::distanceFromRoot for a tree with children before parents"""
    d = [0.] * len(parent)
    for r in range(len(parent) - 1, -1, -1):
        if parent[r] >= 0:
            d[r] = max(0., length[r]) + d[parent[r]]
    return d


def children_of(parent):
    child = [[] for _ in parent]
    for r, p in enumerate(parent):
        if p >= 0:
            child[p].append(r)
    return child


def is_ultrametric(parent, length, epsilon=1e-4):
    """Tree::isUltrametric (src/tree.cpp:191-202): the leaves' distances from the root agree within epsilon"""
    d, child = distance_from_root(parent, length), children_of(parent)
    leaves = [d[r] for r in range(len(parent)) if not child[r]]
    return max(leaves) - min(leaves) <= epsilon


class SimpleTreePrior:
    """The coalescent prior of src/sampler.cpp:9-31."""

    def __init__(self, population_size=1.):
        self.population_size = population_size

    def coalescence_rate(self, lineages):
        return ((float(lineages) * (lineages - 1)) / 2) / float(self.population_size)

    def tree_log_likelihood(self, parent, length):
        d, child = distance_from_root(parent, length), children_of(parent)
        for c in child:
            if len(c) not in (0, 2):
                raise ValueError("the tree is not binary")
        lineages, lp, last = 0, 0., 0.
        for r in sorted(range(len(parent)), key=lambda k: d[k], reverse=True):       # events from the tips to the root
            if lineages > 1:
                lp -= self.coalescence_rate(lineages) * (last - d[r])
            last = d[r]
            lineages += -1 if child[r] else 1
        return lp


def root_log_likelihood(model, root_row):
    """log(1 - rootExt) + log(rootExt) * (residues in the root's row); rootExtProb = insExtProb (src/sampler.h:52)"""
    root_len = sum(1 for ch in root_row if ch not in "-.")
    return math.log(1. - model.ins_ext) + math.log(model.ins_ext) * root_len


def trans_prob(model, t):
    """ProbModel::transProb as a table [src Start/Match, Insert, Delete][dest Match, Insert, Delete, End]"""
    ins, dele = 1 - math.exp(-model.ins_rate * t), 1 - math.exp(-model.del_rate * t)
    ie, de = model.ins_ext, model.del_ext
    return [[(1 - ins) * (1 - dele), ins, (1 - ins) * dele, 1 - ins],
            [(1 - ie) * (1 - dele), ie, (1 - ie) * dele, 1 - ie],
            [1 - de, 0., de, 1 - de]]


def indel_log_likelihood(counts, model, branch_length):
    """sum over the branches (every node but the last, the root) of n[src][dest] * log(transProb(src, dest)).  A term with
    n = 0 is skipped, so a branch of length zero gives -inf where an insertion or deletion sits on it, 0 where none does,
    and never 0 * -inf."""
    lp = 0.
    for node in range(len(branch_length) - 1):
        tp = trans_prob(model, branch_length[node])
        for s in range(3):
            for d in range(4):
                n = int(counts[node][s][d])
                if n:
                    lp += n * (math.log(tp[s][d]) if tp[s][d] > 0 else NEG_INF)
    return lp


def node_height_proposal(parent, length, node, u):
    """NodeHeightMove's tree (src/sampler.cpp:941-972) for the internal `node` and the uniform variate u in [0, 1).
    -> (the new branch lengths, the nodes whose branch changed, logJacobian)"""
    child = children_of(parent)[node]
    if len(child) != 2:
        raise ValueError("the tree is not binary")
    left, right = child
    new = list(length)
    l_dist, r_dist = length[left], length[right]
    min_child = min(l_dist, r_dist)
    if parent[node] < 0:
        max_log = math.log(2)
        log_multiplier = -max_log + (2 * max_log) * u
        new_min_child = min_child * math.exp(log_multiplier)
        new[left] = l_dist - min_child + new_min_child
        new[right] = r_dist - min_child + new_min_child
        return new, [left, right], log_multiplier
    p_dist = max(0., length[node])
    p_range = p_dist + min_child
    p_new = p_range * u
    c_new = p_range - p_new
    new[node] = p_new
    new[left] = (l_dist - min_child) + c_new
    new[right] = (r_dist - min_child) + c_new
    return new, [left, right, node], 0.


def rescale_proposal(length, u):
    """RescaleMove's tree (src/sampler.cpp:983-999): every branch times exp(logMultiplier), logMultiplier uniform in
    +-log 2.  -> (the new branch lengths, the nodes whose branch changed, logJacobian = logMultiplier)"""
    max_log = math.log(2)
    log_multiplier = -max_log + (2 * max_log) * u
    multiplier = math.exp(log_multiplier)
    return [d * multiplier for d in length], list(range(len(length) - 1)), log_multiplier


def random_index(weights, rng):
    """random_index (src/util.h:188-201)"""
    variate = rng.random() * sum(weights)
    for n, w in enumerate(weights):
        variate -= w
        if variate <= 0:
            return n
    return len(weights)


class Move:
    """Sampler::Move: what was proposed, and logAcceptProb = new - old + (reverse - forward + Jacobian)"""

    def __init__(self, kind, node, length, changed, log_jacobian, old_log_likelihood):
        self.kind, self.node, self.length, self.changed = kind, node, length, changed
        self.log_jacobian, self.log_forward, self.log_reverse = log_jacobian, 0., 0.
        self.old_log_likelihood = old_log_likelihood
        self.new_log_likelihood, self.parts = 0., None
        self.log_accept_prob = NEG_INF
        self.nullified = False
        self.u = None                  # the variate accept() drew, if it drew one

    def init_ratio(self, parts):
        """Move::initRatio (src/sampler.cpp:501-509); parts: (tree, root, indels, substitutions) of the new history"""
        self.parts = parts
        self.new_log_likelihood = parts[0] + parts[1] + parts[2] + parts[3]
        self.log_accept_prob = (self.new_log_likelihood - self.old_log_likelihood) + (self.log_reverse - self.log_forward + self.log_jacobian)


class DeviceEvaluator:
    """The resident history of hx_history.hip behind the evaluator interface, in one of two modes.

    "lengths" (the default when no sub_prob is given): the history takes model.sub_rate once and every proposal is its
    (node, branch length) pairs; exp(R t) is computed on the device with the bits of the C++ mirror's getSubProbMatrix.
    "matrices" (the default when sub_prob is given): sub_prob(t) -> [C] matrices exp(R t) on the host for every changed
    branch (model.sub_prob, scipy's expm, unless given), uploaded with the proposal."""

    def __init__(self, model, parent, length, tokens, sub_prob=None, stream=None, mode=None):
        self.mode = mode or ("matrices" if sub_prob else "lengths")
        if self.mode not in ("lengths", "matrices"):
            raise ValueError("mode must be 'lengths' or 'matrices'")
        self.sub_prob = (sub_prob or model.sub_prob) if self.mode == "matrices" else None
        self.stream = stream
        c, a, n = model.components(), len(model.alphabet), len(parent)
        ins_prob, log_cpt_weight = np.asarray(model.root, dtype=float).reshape(c, a), np.log(np.asarray(model.cpt_weight, dtype=float))
        if self.mode == "lengths":
            self.history = capi.History.from_lengths(parent, ins_prob, log_cpt_weight, tokens, np.asarray(model.sub_rate, dtype=float), length, stream=stream)
            return
        branch_sub = np.zeros((c, n, a, a))
        for r in range(n - 1):
            branch_sub[:, r] = np.asarray(self.sub_prob(length[r]), dtype=float)
        self.history = capi.History(parent, ins_prob, log_cpt_weight, tokens, branch_sub, stream=stream)

    def lp_sub(self):
        return self.history.log_like(0, want_columns=False)[0]

    def indel_counts(self):
        return self.history.indel_counts()

    def propose(self, nodes, lengths):
        if self.mode == "lengths":
            return self.history.propose_lengths(nodes, lengths, stream=self.stream)
        return self.history.propose(nodes, np.asarray([self.sub_prob(t) for t in lengths], dtype=float), stream=self.stream)

    def accept(self):
        self.history.accept()

    def reject(self):
        self.history.reject()

    def close(self):
        self.history.close()


class TreeSampler:
    """Sampler (src/sampler.h) for a fixed alignment and topology.  model: hostmodel.RateModel; rows: one gapped row per
    node; evaluator: see the module's docstring.  steps: one (move type, node or -1, logAcceptProb, accepted, u) per
    sample(), u the variate the acceptance drew or None."""

    def __init__(self, model, parent, length, rows, evaluator, tree_prior=None):
        self.model, self.parent, self.length, self.rows = model, list(parent), list(length), rows
        self.evaluator, self.tree_prior = evaluator, tree_prior or SimpleTreePrior()
        self.internal = [r for r, c in enumerate(children_of(parent)) if c]
        self.counts = np.asarray(evaluator.indel_counts())
        self.lp_root = root_log_likelihood(model, rows[len(parent) - 1])
        self.parts = self.log_likelihood_parts(self.length, evaluator.lp_sub())
        self.log_likelihood = sum_parts(self.parts)
        self.best_history, self.best_log_likelihood = (list(self.length), self.rows), self.log_likelihood
        # Sampler::initialize's rates with fixAlignment; prune-and-regraft is not built
        self.move_rate = [0., 0., 0., 2., 2.]
        self.moves_proposed, self.moves_accepted = [0] * 5, [0] * 5
        self.steps = []

    def log_likelihood_parts(self, length, lp_sub):
        """(tree, root, indels, substitutions) of TreeAlignFuncs::logLikelihood"""
        return (self.tree_prior.tree_log_likelihood(self.parent, length), self.lp_root,
                indel_log_likelihood(self.counts, self.model, length), lp_sub)

    def _finish(self, move):
        lp_sub = self.evaluator.propose(move.changed, [move.length[r] for r in move.changed])
        move.init_ratio(self.log_likelihood_parts(move.length, lp_sub))
        return move

    def propose_node_height(self, rng):
        """the node as randomInternalNode draws it, then the branch lengths of NodeHeightMove"""
        node = self.internal[min(int(rng.random() * len(self.internal)), len(self.internal) - 1)]
        length, changed, log_jacobian = node_height_proposal(self.parent, self.length, node, rng.random())
        return self._finish(Move(NODE_HEIGHT, node, length, changed, log_jacobian, self.log_likelihood))

    def propose_rescale(self, rng):
        length, changed, log_jacobian = rescale_proposal(self.length, rng.random())
        return self._finish(Move(RESCALE, -1, length, changed, log_jacobian, self.log_likelihood))

    def propose_move(self, rng):
        kind = random_index(self.move_rate, rng)
        if kind == NODE_HEIGHT:
            return self.propose_node_height(rng)
        if kind == RESCALE:
            return self.propose_rescale(rng)
        raise NotImplementedError("%s moves are not built" % MOVE_NAMES[kind])

    @staticmethod
    def accept(move, rng):
        """Move::accept: a nullified move is bypassed; logAcceptProb >= 0 accepts without drawing; else one variate"""
        if move.nullified:
            return False
        if move.log_accept_prob >= 0:
            return True
        move.u = rng.random()
        return move.u < math.exp(move.log_accept_prob)

    def sample(self, rng):
        move = self.propose_move(rng)
        self.moves_proposed[move.kind] += 1
        accepted = self.accept(move, rng)
        if accepted:
            self.evaluator.accept()
            self.length, self.parts, self.log_likelihood = move.length, move.parts, move.new_log_likelihood
            self.moves_accepted[move.kind] += 1
        else:
            self.evaluator.reject()
        if move.new_log_likelihood > self.best_log_likelihood:
            self.best_history, self.best_log_likelihood = (list(move.length), self.rows), move.new_log_likelihood
        self.steps.append((move.kind, move.node, move.log_accept_prob, accepted, move.u))
        return move

    def run(self, n_samples, rng):
        for _ in range(n_samples):
            self.sample(rng)

    def move_stats(self):
        return "".join("%20s: %5d moves, %5d accepted\n" % (MOVE_NAMES[t], self.moves_proposed[t], self.moves_accepted[t]) for t in range(5))


def sum_parts(parts):
    return parts[0] + parts[1] + parts[2] + parts[3]
