"""Pins tests/sibling_ref.py (Sampler::SiblingMatrix, reference src/sampler.h:226-325,
src/sampler.cpp:1185-1608) by enumeration: no reference fixture holds a sibling matrix (the reference cannot be built for want
of GSL and none of its tests drives the sampler).  On children of 0-3 x 0-3 positions every history - a sequence of columns
of the six kinds IMM, IMD, IDM, IDD, left insert, right insert - is listed, its state path fixed by get_state, and scored in
plain libm floating point with the raw lp_trans and the wait states summed explicitly (not the eliminated members the fill
uses).  A run of IDD columns between two other columns is summed in closed form, 1 / (1 - iddSelfLoopProb), so the set is
finite and the sum exact."""
import math
import random

import pytest

from oracle.historian_oracle import NEG_INF
from tests import sibling_ref as sr

KINDS = ((True, True, True), (True, False, True), (False, True, True), (False, False, True), (True, False, False), (False, True, False))
IDD_COLUMN = (False, False, True)
TABLE_BOUND = 1e-3          # the accuracy of the reference's table log_sum_exp, as tests/test_oracle_branch.py bounds it


def through_waits(m, src, dest):
    """probability of going from emitting state src to dest: directly, or through one of the three wait states"""
    def p(a, b):
        lp = m.lp_trans(a, b)
        return math.exp(lp) if lp > NEG_INF else 0.
    return p(src, dest) + sum(p(src, w) * p(w, dest) for w in (sr.WWW, sr.WWX, sr.WXW))


def histories(m):
    """[(columns, probability)] of every history inside the envelope with a positive probability; a run of IDD columns is
    one column here, its weight the closed-form sum over the run's length"""
    nx, ny = m.x_size - 1, m.y_size - 1
    idd_runs = 1. / (1. - m.idd_self_loop_prob())
    out = []

    def rec(i, j, state, prob, cols):
        if i == nx and j == ny:
            end = prob * through_waits(m, state, sr.EEE)
            if end > 0.:
                out.append((list(cols), end))
        for col in KINDS:
            if col == IDD_COLUMN and cols and cols[-1] == IDD_COLUMN:
                continue
            ni, nj = i + col[0], j + col[1]
            if ni > nx or nj > ny or not m.in_envelope(ni, nj):
                continue
            nstate = sr.get_state(state, *col)
            e = m.lp_emit(ni, nj, nstate)
            p = prob * through_waits(m, state, nstate) * (math.exp(e) if e > NEG_INF else 0.)
            if col == IDD_COLUMN:
                p *= idd_runs
            if p > 0.:
                cols.append(col)
                rec(ni, nj, nstate, p, cols)
                cols.pop()
    rec(0, 0, sr.SSS, 1., [])
    return out


def rows_of(cols):
    return [c[0] for c in cols], [c[1] for c in cols], [c[2] for c in cols]


# (seed, left positions, right positions, components, band, envelope coordinates non-decreasing): bands that cut cells, the
# degenerate 0 x n and n x 0
CASES = [(1, 2, 2, 1, None, True), (2, 3, 2, 1, None, True), (3, 2, 3, 2, None, True), (4, 3, 3, 1, 0, False), (14, 3, 3, 2, 1, False),
         (6, 1, 3, 1, None, True), (7, 0, 3, 1, None, True), (8, 3, 0, 2, None, True), (9, 0, 0, 1, None, True), (10, 3, 3, 1, 0, True),
         (11, 1, 1, 2, 0, False), (12, 3, 3, 1, None, True)]


def build(seed, nx, ny, C, band, sorted_env, **kw):
    return sr.SiblingMatrix(**sr.random_case(seed, nx, ny, C=C, band=band, sorted_env=sorted_env), **kw)


@pytest.mark.parametrize("seed,nx,ny,C,band,sorted_env", CASES)
def test_lp_end_is_the_log_of_the_summed_history_probabilities(seed, nx, ny, C, band, sorted_env):
    exact = build(seed, nx, ny, C, band, sorted_env, lse=sr.log_sum_exp_libm)
    table = build(seed, nx, ny, C, band, sorted_env)
    hs = histories(exact)
    assert hs
    if band is not None and (nx, ny) == (3, 3):
        assert any(not exact.in_envelope(i, j) for i in range(nx + 1) for j in range(ny + 1)), "the band cuts no cell"
    lp = math.log(sum(p for _, p in hs))
    print("lpEnd libm %.17g table %.17g enumerated %.17g over %d histories" % (exact.lp_end, table.lp_end, lp, len(hs)))
    assert abs(exact.lp_end - lp) <= 1e-12 * max(1., abs(lp))
    assert abs(table.lp_end - lp) <= TABLE_BOUND


@pytest.mark.parametrize("seed,nx,ny,C,band,sorted_env", CASES)
def test_posteriors_of_all_alignments_sum_to_one(seed, nx, ny, C, band, sorted_env):
    for lse, bound in ((sr.log_sum_exp_libm, 1e-12), (None, TABLE_BOUND)):
        m = build(seed, nx, ny, C, band, sorted_env, **({"lse": lse} if lse else {}))
        idd_runs = 1. / (1. - m.idd_self_loop_prob())
        total = 0.
        for cols, _ in histories(m):
            total += math.exp(m.log_post_prob(rows_of(cols))) * idd_runs ** cols.count(IDD_COLUMN)
        print("sum of posteriors", total)
        assert abs(total - 1.) <= bound


def test_a_path_leaving_the_envelope_scores_minus_infinity():
    m = build(10, 3, 3, 1, 0, True)
    outside = [(i, j) for i in range(4) for j in range(4) if not m.in_envelope(i, j)]
    assert outside
    i, j = outside[0]
    cols = [KINDS[1]] * i + [KINDS[2]] * j + [KINDS[1]] * (3 - i) + [KINDS[2]] * (3 - j)      # visits (i, j)
    assert m.log_post_prob(rows_of(cols)) == NEG_INF
    inside = [KINDS[0]] * 3
    if all(m.in_envelope(k, k) for k in range(4)):
        assert m.log_post_prob(rows_of(inside)) > NEG_INF


def collapse(rows):
    """runs of IDD columns as one column"""
    out = []
    for col in zip(*rows):
        if col == IDD_COLUMN and out and out[-1] == IDD_COLUMN:
            continue
        out.append(col)
    return tuple(out)


def test_sampled_alignments_spell_the_lengths_and_have_finite_posteriors():
    for seed, nx, ny, C, band, sorted_env in CASES:
        m = build(seed, nx, ny, C, band, sorted_env)
        src = sr.ListSource(random.Random(100 + seed))
        for _ in range(20):
            rows = m.sample(src)
            assert sum(rows[0]) == nx and sum(rows[1]) == ny and len(set(map(len, rows))) == 1
            assert all(any(col) for col in zip(*rows))
            assert NEG_INF < m.log_post_prob(rows) <= 0.


def test_sampled_frequencies_follow_the_posterior():
    # Every alignment expected at least five times in n draws: its frequency within 5 sqrt(p (1 - p) / n) of its enumerated
    # posterior p.  Below that the normal bound says nothing about a single alignment (with n p < 0.04 it is under 1 / n and
    # one draw breaks it; the 2 x 2 case expects 1.9 such draws in 20000), so the rarer alignments are held to the same
    # bound together, as one class.  Nothing here hangs on the seed: seeds 1 to 10 were run before this went in.
    m = build(1, 2, 2, 1, None, True)
    idd_runs = 1. / (1. - m.idd_self_loop_prob())
    # The reference's walk stops as soon as it stands in cell (0, 0), whatever the state (src/sampler.cpp:1346), so an IDD
    # column in front of the first residue is never written: a history that opens with one is drawn as the same history
    # without it (found here: 'IDD IMM IMM', p = 1.1e-3, was never drawn and 'IMM IMM' came 1.2e-3 too often).  The
    # restatement keeps that; the expected frequencies are the posteriors with such an opening column folded away.
    post = {}
    for cols, _ in histories(m):
        key = tuple(cols[1:] if cols and cols[0] == IDD_COLUMN else cols)
        post[key] = post.get(key, 0.) + math.exp(m.log_post_prob(rows_of(cols))) * idd_runs ** cols.count(IDD_COLUMN)
    n = 20000
    src = sr.ListSource(random.Random(2))
    seen = {}
    for _ in range(n):
        key = collapse(m.sample(src))
        seen[key] = seen.get(key, 0) + 1
    assert set(seen) <= set(post)
    common = [key for key, p in post.items() if n * p >= 5.]
    rare = [key for key, p in post.items() if n * p < 5.]
    assert len(common) >= 20 and rare
    worst = 0.
    for key in common:
        p = post[key]
        dev = abs(seen.get(key, 0) / n - p)
        sd = math.sqrt(p * (1 - p) / n)
        worst = max(worst, dev / sd)
        assert dev <= 5 * sd, (key, p, seen.get(key, 0))
    p_rare = sum(post[key] for key in rare)
    f_rare = sum(seen.get(key, 0) for key in rare) / n
    print("%d alignments, %d held one by one (worst deviation %.2f sd), %d as one class: p %.3g, drawn %.3g"
          % (len(post), len(common), worst, len(rare), p_rare, f_rare))
    assert abs(f_rare - p_rare) <= 5 * math.sqrt(p_rare * (1 - p_rare) / n)


def test_mt19937_source_draws_walks():
    from oracle.historian_oracle import MT19937
    m = build(2, 3, 2, 1, None, True)
    a = m.sample(sr.MTSource(MT19937(7)))
    assert a == m.sample(sr.MTSource(MT19937(7))) and sum(a[0]) == 3 and sum(a[1]) == 2


def test_parent_profile_is_normalised_and_matches_a_hand_computation():
    m = build(5, 3, 3, 2, None, True, lse=sr.log_sum_exp_libm)
    rows = m.sample(sr.ListSource(random.Random(3)))
    prof = m.parent_seq(rows)
    assert len(prof) == sum(rows[2])
    for pos in prof:
        assert abs(math.log(sum(math.exp(v) for row in pos for v in row))) <= 1e-12
    # one certain residue k in either child, one IMM column: parent[a] = Pl[a][k] Pr[a][k] / sum_a' Pl[a'][k] Pr[a'][k]
    A, k = 4, 2
    pl = [[.7 if a == b else .1 for b in range(A)] for a in range(A)]
    pr = [[.4 if a == b else .2 for b in range(A)] for a in range(A)]
    child = [[[0. if a == k else NEG_INF for a in range(A)]]]
    lsub = sr.pre_multiply(child, [[[math.log(v) for v in row] for row in pl]])
    rsub = sr.pre_multiply(child, [[[math.log(v) for v in row] for row in pr]])
    root = [[math.log(.25)] * A]
    pm = sr.Indel(.1, .1, .5, .5)
    one = sr.SiblingMatrix(lsub, rsub, root, sr.calc_ins_probs(child, root, [0.]), sr.calc_ins_probs(child, root, [0.]), pm, pm, .5,
                           lse=sr.log_sum_exp_libm)
    got = one.parent_seq(([True], [True], [True]))
    norm = sum(pl[a][k] * pr[a][k] for a in range(A))        # .1 * .2 * 3 + .7 * .4 = .34
    assert abs(norm - .34) < 1e-15
    for a in range(A):
        # (pre_multiply runs on the table operator: its sums over one finite term are exact)
        assert abs(got[0][0][a] - math.log(pl[a][k] * pr[a][k] / norm)) <= 1e-12


def test_transition_table_has_the_reference_s_35_members():
    m = build(1, 1, 1, 1, None, True)
    finite = [(s, d) for s in range(sr.N_STATES) for d in range(12) if m.T[s][d] > NEG_INF]
    assert len(finite) == 35 and sum(1 for s, d in finite if d == sr.EEE) == 4
    # the IDD self-loop is folded into IDD's exits
    assert m.T[sr.IDD][sr.IDD] == NEG_INF and m.lp_trans(sr.IDD, sr.IDD) == m.idd_stay()
    assert m.T[sr.IDD][sr.IMM] == m.lp_trans(sr.IDD, sr.IMM) + m.idd_exit()
    # a wait state passes on to the next parent column with the root's extension probability, whichever gaps are open
    for w in (sr.WWW, sr.WWX, sr.WXW):
        total = sum(math.exp(m.lp_trans(w, d)) for d in (sr.IMM, sr.IMD, sr.IDM, sr.IDD))
        assert abs(total - m.root_ext_prob) <= 1e-12, (sr.STATE_NAMES[w], total)


def test_product_side_score_table_is_the_restatement_s():
    # historian_amd.hostmodel.sibling_trans: what a Python caller of capi.SiblingBatch passes as hx_sibling_job.trans
    import struct
    from historian_amd import hostmodel
    for seed in (1, 2, 3):
        m = build(seed, 1, 1, 1, None, True)
        l, r = (dict(ins=pm.ins, dele=pm.dele, ins_ext=pm.ins_ext, del_ext=pm.del_ext) for pm in (m.l_pm, m.r_pm))
        got = hostmodel.sibling_trans(l, r, m.root_ext_prob)
        for s_ in range(sr.N_STATES):
            for d in range(12):
                assert struct.pack("d", got[s_, d]) == struct.pack("d", m.T[s_][d]), (sr.STATE_NAMES[s_], sr.STATE_NAMES[d])
