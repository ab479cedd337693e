"""Pins tests/walks_ref.py - Sampler::BranchMatrix::sample / logPathProb / logPostProb (reference src/sampler.cpp:1088-1160) and the
recording form of both sampled walks - by enumeration, as tests/test_oracle_branch.py and tests/test_oracle_sibling.py pin the
matrices they walk; and checks the precondition of tests/test_gpu_walks.py: on every case and word stream used there, no draw
falls within 1e-12 of a boundary between two states' shares."""
import math
import random

import pytest

from oracle import branch_oracle as bo
from oracle.historian_oracle import MT19937, NEG_INF
from tests import sibling_ref as sr
from tests import walks_cases as wc
from tests import walks_ref as wr
from tests.test_gpu_branch import random_branch

TABLE_BOUND = 1e-3          # the accuracy of the reference's table log_sum_exp, as tests/test_oracle_branch.py bounds it
# The device's exp() is good to an ulp or two (about 2e-16 relative) and a step sums at most eleven such terms, so a
# margin of 1e-12 leaves three orders of magnitude; a word has 2^-32 resolution, so a margin that small has a probability
# of about 1e-11 per step.  Derived, not measured.
MARGIN = 1e-12


def rows_of_states(path):
    return [s != bo.INSERT for s in path], [s != bo.DELETE for s in path]


def tiny(seed, nx, ny, band=None, C=1):
    x, ysub, yemit, T, xe, ye, md = random_branch(seed, nx, ny, C, 4, band, False)
    return bo.BranchMatrix(x, ysub, yemit, T, None if xe is None else list(xe), None if ye is None else list(ye), md, viterbi=False)


TINY = [(seed, nx, ny) for seed, (nx, ny) in enumerate((nx, ny) for nx in range(4) for ny in range(4))]


@pytest.mark.parametrize("seed,nx,ny", TINY)
def test_branch_posteriors_of_all_paths_sum_to_one(seed, nx, ny):
    bm = tiny(seed, nx, ny, C=1 + seed % 2)
    total = 0.
    for path in bo.enumerate_paths(nx, ny):
        rows = rows_of_states(path)
        assert sum(rows[0]) == nx and sum(rows[1]) == ny
        lp = wr.branch_log_path_prob(bm, rows)
        plain = bo.path_log_prob(bm, path)
        # the path's own score in plain floating point, unless the matrix's (table) cell value cut it down
        assert lp <= plain + 1e-12 and lp >= plain - TABLE_BOUND
        post = wr.branch_log_post_prob(bm, rows)
        assert post <= 0.
        total += math.exp(post)
    print("sum of posteriors", total)
    assert abs(total - 1.) <= TABLE_BOUND * max(1, len(bo.enumerate_paths(nx, ny)) ** .5)


def test_a_branch_path_leaving_the_envelope_scores_minus_infinity():
    bm = tiny(3, 3, 3, band=0)
    outside = [(i, j) for i in range(4) for j in range(4) if not bm.in_envelope(i, j)]
    assert outside
    i, j = outside[0]
    path = [bo.DELETE] * i + [bo.INSERT] * j + [bo.DELETE] * (3 - i) + [bo.INSERT] * (3 - j)
    assert wr.branch_log_post_prob(bm, rows_of_states(path)) == NEG_INF


def test_branch_sampled_frequencies_follow_the_posterior():
    # every alignment of a 2 x 2 pair expected at least five times in n draws: within 5 sd of its posterior
    bm = tiny(1, 2, 2)
    post = {}
    for path in bo.enumerate_paths(2, 2):
        rows = rows_of_states(path)
        post[tuple(map(tuple, rows))] = math.exp(wr.branch_log_post_prob(bm, rows))
    n = 20000
    src = sr.ListSource(random.Random(2))
    seen = {}
    for _ in range(n):
        rows = wr.branch_sample(bm, src)
        assert sum(rows[0]) == 2 and sum(rows[1]) == 2
        key = tuple(map(tuple, rows))
        seen[key] = seen.get(key, 0) + 1
    assert set(seen) <= set(post)
    held, rare = 0, 0.
    for key, p in post.items():
        if n * p < 5.:
            rare += p
            continue
        held += 1
        assert abs(seen.get(key, 0) / n - p) <= 5 * math.sqrt(p * (1 - p) / n) + TABLE_BOUND * p, (key, p, seen.get(key, 0))
    # the rarer alignments together, as one class (see tests/test_oracle_sibling.py)
    f_rare = sum(v for key, v in seen.items() if n * post[key] < 5.) / n
    print("%d of %d alignments held one by one, the rest as one class: p %.3g, drawn %.3g" % (held, len(post), rare, f_rare))
    assert held >= 2 and abs(f_rare - rare) <= 5 * math.sqrt(rare * (1 - rare) / n) + TABLE_BOUND


def test_recorded_states_spell_the_sampled_alignment_and_best_states_the_best_one():
    for c in wc.BRANCH_CASES[:4]:
        _, bm = wc.branch_matrix(c)
        w = wr.branch_walk(bm, wr.WordSource(wr.mt_words(5, 2000)))
        assert wr.branch_rows_of_states(bm, w.states) == (w.rows[0], w.rows[1])
        assert w.words_used == len(w.states) and NEG_INF < wr.branch_log_post_prob(bm, w.rows) <= 0.
        _, vm = wc.branch_matrix(c, viterbi=True)
        xp, yp = vm.best()
        assert wr.branch_rows_of_states(vm, wr.best_states(vm)) == (xp, yp)


def test_the_recording_sibling_walk_is_the_restated_one():
    # same alignment and same generator position as tests/sibling_ref.py's sample from a std::mt19937
    visits = 0
    for seed in range(6):
        m = sr.SiblingMatrix(**sr.random_case(seed, 40, 35))
        for q in range(10):
            mt = MT19937(40 + q)
            want = m.sample(sr.MTSource(mt))
            words = wr.mt_words(40 + q, 600)
            w = wr.sibling_walk(m, wr.WordSource(words))
            assert tuple(want) == tuple(w.rows)
            assert mt.next_u32() == words[w.words_used]
            assert w.words_used == len(w.states) + 2 * w.idd_visits
            visits += w.idd_visits
    assert visits > 0


def test_no_draw_of_the_gpu_tests_falls_near_a_boundary():
    worst, visits, walks = math.inf, 0, 0
    for k, c in enumerate(wc.BRANCH_CASES):
        _, bm = wc.branch_matrix(c)
        for q in range(wc.STREAMS):
            w = wr.branch_walk(bm, wr.WordSource(wc.words(k, q, c[1], c[2])))
            assert w.margin >= MARGIN, ("branch", c, q, w.margin)
            assert len(w.states) <= c[1] + c[2] + 1
            worst, walks = min(worst, w.margin), walks + 1
    for k, c in enumerate(wc.SIBLING_CASES):
        _, m = wc.sibling_matrix(c)
        for q in range(wc.STREAMS):
            w = wr.sibling_walk(m, wr.WordSource(wc.words(100 + k, q, c[1], c[2])))
            assert w.margin >= MARGIN, ("sibling", c, q, w.margin)
            assert len(w.states) <= 3 * (c[1] + c[2]) + 3          # the bound include/historian_hip.h states
            worst, walks, visits = min(worst, w.margin), walks + 1, visits + w.idd_visits
    print("%d walks, smallest margin %.3g, IDD visited %d times" % (walks, worst, visits))
    assert visits >= 1
