"""The tree sampler's logic without a GPU (historian_amd/treesampler.py with the oracle's evaluator, tests/history_ref.py):
the coalescent prior, the two proposals' arithmetic, the count form of the indel term, the acceptance rule."""
import math
import random

import numpy as np
import pytest

from historian_amd import hostmodel
from historian_amd import treesampler as ts
from oracle import historian_oracle as ho
from tests import history_ref as HR

DNA = {"alphabet": "acgt", "insrate": .03, "delrate": .04, "insextprob": .5, "delextprob": .45,
       "rootprob": {"a": .1, "c": .2, "g": .3, "t": .4},
       "subrate": {"a": {"c": 1., "g": .1}, "c": {"g": 1.2, "t": .05}, "g": {"t": .9, "a": .02}, "t": {"a": 1.1, "c": .3}}}
# leaves 0, 1 join in node 3 at height 1; node 3 and leaf 2 join in the root at height 3
THREE = ([3, 3, 4, 4, -1], [1., 1., 3., 2., 0.])


def test_the_prior_of_a_hand_computed_three_leaf_tree():
    parent, length = THREE
    assert ts.distance_from_root(parent, length) == [3., 3., 3., 2., 0.]
    # from the tips: three lineages for one unit of time (rate 3), two for two units (rate 1)
    assert ts.SimpleTreePrior().tree_log_likelihood(parent, length) == -(3. * 1. + 1. * 2.)
    assert ts.SimpleTreePrior(2.).tree_log_likelihood(parent, length) == -2.5
    assert ts.is_ultrametric(parent, length) and not ts.is_ultrametric(parent, [1., 1.2, 3., 2., 0.])


@pytest.mark.parametrize("seed", [1, 2])
def test_node_height_keeps_the_tree_ultrametric_and_the_range_fixed(seed):
    rng = np.random.default_rng(seed)
    parent, length = HR.ultrametric_tree(rng, 7)
    assert ts.is_ultrametric(parent, length, 1e-12)
    child = ts.children_of(parent)
    height = max(ts.distance_from_root(parent, length))
    for node in range(len(parent)):
        if not child[node]:
            continue
        for u in (0., .25, .5, .999):
            new, changed, log_j = ts.node_height_proposal(parent, length, node, u)
            assert ts.is_ultrametric(parent, new, 1e-12)
            assert all(new[r] == length[r] for r in range(len(parent)) if r not in changed)
            left, right = child[node]
            if parent[node] >= 0:
                assert sorted(changed) == sorted([left, right, node]) and log_j == 0.
                old_range = max(0., length[node]) + min(length[left], length[right])
                assert abs(new[node] + min(new[left], new[right]) - old_range) <= 4 * 2. ** -53 * old_range
                assert abs(max(ts.distance_from_root(parent, new)) - height) <= 1e-12
                assert min(new) >= 0.
            else:
                # the root: the coalescence time of its children is multiplied by exp(logJacobian), within a factor of 2
                assert sorted(changed) == sorted([left, right])
                assert log_j == -math.log(2) + 2 * math.log(2) * u
                old_min, new_min = min(length[left], length[right]), min(new[left], new[right])
                assert abs(new_min / old_min - math.exp(log_j)) <= 1e-12


def test_rescale_multiplies_every_branch_and_returns_the_log_multiplier():
    parent, length = HR.ultrametric_tree(np.random.default_rng(3), 6)
    for u in (0., .3, .75):
        new, changed, log_j = ts.rescale_proposal(length, u)
        assert changed == list(range(len(parent) - 1))
        assert log_j == -math.log(2) + 2 * math.log(2) * u
        assert new == [d * math.exp(log_j) for d in length]
        assert ts.is_ultrametric(parent, new, 1e-12)


def _random_presence(rng, parent, n_cols):
    """independent rows of booleans: pairPath takes any two rows"""
    return [[bool(v) for v in rng.random(n_cols) < .7] for _ in parent]


def test_the_count_form_of_the_indel_term_against_the_sequential_sum():
    rng = np.random.default_rng(5)
    model = hostmodel.RateModel(DNA)
    parent, length = HR.ultrametric_tree(rng, 6)
    present = _random_presence(rng, parent, 300)
    counts = HR.indel_counts(parent, present)
    assert counts[-1].sum() == 0 and np.all(counts[:-1].sum(axis=(1, 2)) > 0)
    # TreeAlignFuncs::indelLogLikelihood: the branches in node order, each path's terms in path order
    want, total, n_terms = 0., 0., 0
    for node in range(len(parent) - 1):
        terms = HR.branch_path_terms(ts.trans_prob(model, length[node]), HR.pair_path_states(present[parent[node]], present[node]))
        lp = 0.
        for t in terms:
            lp += t
        want += lp
        total += sum(abs(t) for t in terms)
        n_terms += len(terms)
    got = ts.indel_log_likelihood(counts, model, length)
    # two orderings of one sum of T terms (the count form multiplies first: one more rounding per distinct term, 12 a branch)
    bound = 2 * (n_terms + 16) * 2. ** -53 * total
    print("indel term: count form %.17g, path order %.17g, difference %.3g, bound %.3g over %d terms" % (got, want, abs(got - want), bound, n_terms))
    assert math.isfinite(want) and abs(got - want) <= bound


def test_a_branch_of_length_zero_gives_minus_infinity_or_zero_never_nan():
    model = hostmodel.RateModel(DNA)
    parent, length = [2, 2, -1], [0., .3, 0.]
    with_insertion = [[True, True, False, True], [True, True, True, True], [True, False, True, True]]
    counts = HR.indel_counts(parent, with_insertion)
    assert counts[0, 0, HR.INSERT] == 1
    assert ts.indel_log_likelihood(counts, model, length) == -math.inf
    only_matches = [[True, False, True, True], [True, True, True, True], [True, False, True, True]]
    counts = HR.indel_counts(parent, only_matches)
    lp = ts.indel_log_likelihood(counts, model, length)
    other = ts.indel_log_likelihood(counts, model, [.3, 0., 0.])          # (the zero-length branch now carries the insertion)
    assert math.isfinite(lp) and other == -math.inf
    just_zero = ts.indel_log_likelihood(HR.indel_counts([1, -1], [[True] * 3, [True] * 3]), model, [0., 0.])
    assert just_zero == 0. and not math.isnan(lp)


class CountingGenerator:
    def __init__(self, values=()):
        self.values, self.draws = list(values), 0

    def random(self):
        self.draws += 1
        return self.values.pop(0)


def test_the_acceptance_rule():
    def move(lap, nullified=False):
        m = ts.Move(ts.RESCALE, -1, [], [], 0., 0.)
        m.log_accept_prob, m.nullified = lap, nullified
        return m
    g = CountingGenerator()
    assert ts.TreeSampler.accept(move(0.), g) and ts.TreeSampler.accept(move(2.5), g) and g.draws == 0
    assert not ts.TreeSampler.accept(move(5., nullified=True), g) and g.draws == 0
    g = CountingGenerator([0., .5, .49, .51])
    assert not ts.TreeSampler.accept(move(-math.inf), g) and g.draws == 1           # even the smallest variate rejects
    assert not ts.TreeSampler.accept(move(math.nan), g)
    assert ts.TreeSampler.accept(move(math.log(.5)), g) and not ts.TreeSampler.accept(move(math.log(.5)), g)
    assert ts.random_index([0., 0., 0., 2., 2.], CountingGenerator([.49])) == ts.NODE_HEIGHT
    assert ts.random_index([0., 0., 0., 2., 2.], CountingGenerator([.51])) == ts.RESCALE


def _rows(rng, parent, n_cols, alphabet):
    child = ts.children_of(parent)
    rows = [[] for _ in parent]
    for _ in range(n_cols):
        col = ["-"] * len(parent)
        stack = [len(parent) - 1 if rng.random() < .7 else int(rng.integers(0, len(parent)))]
        while stack:
            r = stack.pop()
            col[r] = "*" if child[r] else alphabet[int(rng.integers(0, len(alphabet)))]
            stack.extend(c for c in child[r] if rng.random() < .85)
        for r in range(len(parent)):
            rows[r].append(col[r])
    return ["".join(r) for r in rows]


def test_a_short_chain_with_the_oracle_evaluator_keeps_its_books():
    rng = np.random.default_rng(8)
    parent, length = HR.ultrametric_tree(rng, 4)
    rows = _rows(rng, parent, 12, "acgt")
    model, omodel = hostmodel.RateModel(DNA), ho.RateModel(DNA)
    sampler = ts.TreeSampler(model, parent, length, rows, HR.OracleEvaluator(omodel, parent, length, rows))
    first = sampler.log_likelihood
    assert sampler.parts[1] == math.log(1 - .5) + math.log(.5) * sum(ch != "-" for ch in rows[-1])
    sampler.run(40, random.Random(3))
    assert sum(sampler.moves_proposed) == 40 == len(sampler.steps) and sampler.moves_proposed[:3] == [0, 0, 0]
    assert sampler.moves_accepted == [sum(1 for s in sampler.steps if s[0] == k and s[3]) for k in range(5)]
    assert 0 < sum(sampler.moves_accepted) < 40 and sampler.moves_proposed[ts.NODE_HEIGHT] > 5 < sampler.moves_proposed[ts.RESCALE]
    assert ts.is_ultrametric(parent, sampler.length, 1e-9)
    # the books: the current likelihood is that of a history evaluated afresh on the current tree
    fresh = ts.TreeSampler(model, parent, sampler.length, rows, HR.OracleEvaluator(omodel, parent, sampler.length, rows))
    assert abs(fresh.log_likelihood - sampler.log_likelihood) <= 1e-12 * abs(fresh.log_likelihood)
    assert sampler.best_log_likelihood >= max(first, sampler.log_likelihood)
    best = ts.TreeSampler(model, parent, sampler.best_history[0], rows, HR.OracleEvaluator(omodel, parent, sampler.best_history[0], rows))
    assert abs(best.log_likelihood - sampler.best_log_likelihood) <= 1e-12 * abs(best.log_likelihood)
