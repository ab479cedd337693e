"""Row N4's matrices consumed on the device (hx_pairdp.h k_pair_walk / k_pair_gather; C ABI hx_branch_batch_best_paths,
hx_*_batch_sample_paths, hx_*_batch_read_cells) against the restatements: Refiner::BranchMatrix::best
(oracle/branch_oracle.py), Sampler::BranchMatrix::sample / logPostProb (tests/walks_ref.py), Sampler::SiblingMatrix::sample /
logPostProb (tests/sibling_ref.py).  Best paths are additions and comparisons: state for state.  Sampled walks run
random_key_log with the device library's exp(); tests/test_oracle_walks.py checks on the CPU that no draw of the cases and
word streams used here (tests/walks_cases.py) falls within 1e-12 of a boundary, so every walk is compared, state for state
and word for word - none is left out."""
import copy

import numpy as np
import pytest

from historian_amd import capi
from oracle import branch_oracle as bo
from oracle import c_oracle
from tests import helpers as H
from tests import sibling_ref as sr
from tests import walks_cases as wc
from tests import walks_ref as wr
from tests.test_gpu_branch import as_job as branch_job, dense as branch_dense, random_branch
from tests.test_gpu_sibling import as_job as sibling_job, dense as sibling_dense

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def engine():
    capi.init(0, c_oracle.table())
    yield
    capi.shutdown()


def viterbi_matrix(case):
    x, ysub, yemit, T, xe, ye, md = case
    return bo.BranchMatrix(x, ysub, yemit, T, None if xe is None else list(xe), None if ye is None else list(ye), md, viterbi=True)


# ---- (a) best paths ----
BEST_CASES = [(11, 5, 7, 1, 4, None, False), (12, 70, 66, 1, 4, None, False), (13, 130, 90, 2, 4, None, False), (14, 64, 65, 1, 20, None, False),
              (15, 200, 180, 1, 4, 6, False), (16, 90, 140, 1, 4, 0, False), (17, 1, 1, 1, 4, None, False), (18, 0, 3, 1, 4, None, False),
              (19, 150, 150, 1, 20, 10, True), (20, 63, 129, 1, 4, 3, True), (21, 0, 0, 1, 4, None, False), (22, 1, 0, 1, 4, None, False),
              (23, 0, 1, 1, 4, None, False), (24, 300, 330, 1, 4, 5, False)]


def test_best_paths_state_for_state_in_a_mixed_batch():
    cases = [random_branch(*c) for c in BEST_CASES]
    b = capi.BranchBatch([branch_job(c) for c in cases])
    b.run(viterbi=True)
    assert b.max_steps() == max(c[1] + c[2] + 1 for c in BEST_CASES)
    paths, n_steps = b.best_paths()
    for k, case in enumerate(cases):
        want = viterbi_matrix(case)
        assert paths[k] == wr.best_states(want), "job %d" % k
        assert n_steps[k] == len(paths[k])
        assert wr.branch_rows_of_states(want, paths[k]) == want.best(), "job %d" % k
    # ... and alone
    for k in (0, 4, 8, 13):
        one = capi.BranchBatch([branch_job(cases[k])])
        one.run(viterbi=True)
        assert one.best_paths()[0][0] == paths[k]
        one.close()
    b.close()


@pytest.mark.parametrize("band", [None, 20])
def test_best_path_of_a_thousand_by_a_thousand(band):
    case = random_branch(41, 1000, 1000, 1, 4, band, False)
    want = viterbi_matrix(case)
    b = capi.BranchBatch([branch_job(case)])
    b.run(viterbi=True)
    paths, n_steps = b.best_paths()
    assert paths[0] == wr.best_states(want) and 1000 <= n_steps[0] <= 2001
    assert wr.branch_rows_of_states(want, paths[0]) == want.best()
    b.close()


# ---- (b) sampled paths ----
@pytest.fixture(scope="module")
def branch_mixed():
    built = [wc.branch_matrix(c) for c in wc.BRANCH_CASES]
    b = capi.BranchBatch([branch_job(case) for case, _ in built])
    b.run(viterbi=False)
    yield built, b
    b.close()


@pytest.fixture(scope="module")
def sibling_mixed():
    built = [wc.sibling_matrix(c) for c in wc.SIBLING_CASES]
    b = capi.SiblingBatch([sibling_job(case, m) for case, m in built])
    b.run()
    yield built, b
    b.close()


def test_branch_sampled_paths_state_for_state(branch_mixed):
    built, b = branch_mixed
    for q in range(wc.STREAMS):
        streams = [wc.words(k, q, c[1], c[2]) for k, c in enumerate(wc.BRANCH_CASES)]       # every job its own stream
        paths, n_steps, used = b.sample_paths(streams)
        for k, (case, bm) in enumerate(built):
            w = wr.branch_walk(bm, wr.WordSource(streams[k]))
            print("job %d stream %d: %d steps, margin %.3g" % (k, q, len(w.states), w.margin))
            assert paths[k] == w.states, "job %d stream %d" % (k, q)
            assert (n_steps[k], used[k]) == (len(w.states), w.words_used)
        if q == 0:
            for k in (0, 3, 4, 7, 9):
                one = capi.BranchBatch([branch_job(built[k][0])])
                one.run(viterbi=False)
                assert one.sample_paths([streams[k]]) == ([paths[k]], [n_steps[k]], [used[k]])
                one.close()


def test_sibling_sampled_paths_state_for_state(sibling_mixed):
    built, b = sibling_mixed
    assert b.max_steps() == max(3 * (c[1] + c[2]) + 3 for c in wc.SIBLING_CASES)
    visits = 0
    for q in range(wc.STREAMS):
        streams = [wc.words(100 + k, q, c[1], c[2]) for k, c in enumerate(wc.SIBLING_CASES)]
        paths, n_steps, used = b.sample_paths(streams)
        for k, (case, m) in enumerate(built):
            w = wr.sibling_walk(m, wr.WordSource(streams[k]))
            print("job %d stream %d: %d steps, margin %.3g, IDD %d" % (k, q, len(w.states), w.margin, w.idd_visits))
            assert paths[k] == w.states, "job %d stream %d" % (k, q)
            assert (n_steps[k], used[k]) == (len(w.states), w.words_used)
            visits += w.idd_visits
        if q == 1:
            for k in (1, 3, 4, 7, 8):
                one = capi.SiblingBatch([sibling_job(*built[k])])
                one.run()
                assert one.sample_paths([streams[k]]) == ([paths[k]], [n_steps[k]], [used[k]])
                one.close()
    assert visits >= 1          # the two words of a geometric draw were consumed and the walks still agree


# ---- (c) cells along a path ----
def test_branch_cells_along_paths_and_posteriors_from_them(branch_mixed):
    built, b = branch_mixed
    lp_end = b.lp_end()
    rng = np.random.default_rng(3)
    for k, (case, bm) in enumerate(built):
        got = b.read_matrix(k)
        X, Y = bm.x_size, bm.y_size
        picks = [(int(rng.integers(X)), int(rng.integers(Y)), int(rng.integers(3))) for _ in range(300)] + [(0, 0, 0), (X - 1, Y - 1, 2)]
        cells, lm = b.read_cells(k, picks)
        H.assert_same_bits(cells, np.array([got[i, j, s] for i, j, s in picks]), "job %d gathered cells" % k)
        for (i, j, s), v in zip(picks, lm):
            want = bm.log_match(i, j) if i > 0 and j > 0 and bm.in_envelope(i, j) else -np.inf
            H.assert_same_bits([v], [want], "job %d logMatch(%d, %d)" % (k, i, j))
        # logPostProb of a sampled path from gathered cells alone
        path = wr.branch_walk(bm, wr.WordSource(wc.words(k, 0, X - 1, Y - 1))).rows
        at = wr.path_cells_branch(path)
        cells, lm = b.read_cells(k, at)
        cell = {c: v for c, v in zip(at, cells)}
        match = {c[:2]: v for c, v in zip(at, lm)}

        def lp_emit(i, j, s):
            return match[(i, j)] if s == bo.MATCH else bm.lp_emit(i, j, s)
        got_lp = wr.branch_log_post_prob(bm, path, cell=lambda i, j, s: cell[(i, j, s)], lp_emit=lp_emit, lp_end=lp_end[k])
        H.assert_same_bits([got_lp], [wr.branch_log_post_prob(bm, path)], "job %d logPostProb" % k)
        assert -np.inf < got_lp <= 0. or not at


def test_sibling_cells_along_paths_and_posteriors_from_them(sibling_mixed):
    built, b = sibling_mixed
    lp_end = b.lp_end()
    rng = np.random.default_rng(4)
    for k, (case, m) in enumerate(built):
        got = b.read_matrix(k)
        X, Y = m.x_size, m.y_size
        picks = [(int(rng.integers(X)), int(rng.integers(Y)), int(rng.integers(11))) for _ in range(300)] + [(0, 0, 0), (X - 1, Y - 1, 10)]
        cells, lm = b.read_cells(k, picks)
        H.assert_same_bits(cells, np.array([got[i, j, s] for i, j, s in picks]), "job %d gathered cells" % k)
        for (i, j, s), v in zip(picks, lm):
            want = m.log_match(i, j) if i > 0 and j > 0 and m.in_envelope(i, j) else -np.inf
            H.assert_same_bits([v], [want], "job %d logMatch(%d, %d)" % (k, i, j))
        path = wr.sibling_walk(m, wr.WordSource(wc.words(100 + k, 0, X - 1, Y - 1))).rows
        at = wr.path_cells_sibling(path)
        cells, lm = b.read_cells(k, at)
        dev = copy.copy(m)
        dev.cells, dev.lp_end = None, lp_end[k]                    # nothing of the restatement's matrix is read
        dev._match = {c[:2]: v for c, v in zip(at, lm)}
        cell = {c: v for c, v in zip(at, cells)}
        dev.cell = lambda i, j, s, cell=cell, dev=dev: dev.lp_end if s == sr.EEE else cell[(i, j, s)]
        H.assert_same_bits([dev.log_post_prob(path)], [m.log_post_prob(path)], "job %d logPostProb" % k)
        assert -np.inf < m.log_post_prob(path) <= 0.


# ---- (d) failure codes: host-checked or early exits of the kernel ----
def test_failure_codes_leave_the_other_jobs_alone():
    good = random_branch(*wc.BRANCH_CASES[0])
    x, ysub, yemit, T, xe, ye, md = good
    dead = (x, ysub, yemit, [row[:3] + [-np.inf] for row in T], xe, ye, md)          # nothing reaches End: lpEnd = -inf
    b = capi.BranchBatch([branch_job(dead), branch_job(good)])
    with pytest.raises(capi.HxError) as e:
        b.best_paths()                                                                 # before a run
    assert e.value.code == -7
    b.run(viterbi=False)
    assert np.isneginf(b.lp_end()[0])
    with pytest.raises(capi.HxError) as e:
        b.best_paths()                                                                 # the batch ran with viterbi = 0
    assert e.value.code == -7
    streams = [wc.words(0, 0, 5, 7)] * 2
    paths, n_steps, used = b.sample_paths(streams)
    _, bm = wc.branch_matrix(wc.BRANCH_CASES[0])
    assert n_steps[0] == -1 and paths[0] is None
    assert paths[1] == wr.branch_walk(bm, wr.WordSource(streams[1])).states
    paths, n_steps, used = b.sample_paths(streams, cap=2)
    assert n_steps == [-1, -3]                                                         # cap too small
    paths, n_steps, used = b.sample_paths([streams[0], streams[1][:3]])
    assert n_steps == [-1, -6] and used[1] == 3                                        # out of words
    paths, n_steps, used = b.sample_paths([[], []])
    assert n_steps == [-1, -6] and used[1] == 0
    for k, at in ((2, [(0, 0, 0)]), (-1, [(0, 0, 0)]), (1, [(6, 0, 0)]), (1, [(0, 8, 0)]), (1, [(0, 0, 3)]), (1, [(-1, 0, 0)])):
        with pytest.raises(capi.HxError) as e:
            b.read_cells(k, at)
        assert e.value.code == -8
    b.run(viterbi=True)
    with pytest.raises(capi.HxError) as e:
        b.sample_paths(streams)                                                        # the batch ran with viterbi != 0
    assert e.value.code == -7
    paths, n_steps = b.best_paths()
    assert n_steps[0] == -1 and paths[1] == wr.best_states(viterbi_matrix(good))
    assert b.best_paths(cap=3)[1] == [-1, -3]
    b.close()


def test_sibling_failure_codes():
    case, m = wc.sibling_matrix(wc.SIBLING_CASES[0])
    job = sibling_job(case, m)
    dead_T = [row[:11] + [-np.inf] for row in m.T]
    b = capi.SiblingBatch([job[:5] + (dead_T,) + job[6:], job])
    with pytest.raises(capi.HxError) as e:
        b.sample_paths([[1], [1]])                                                     # before a run
    assert e.value.code == -7
    b.run()
    streams = [wc.words(100, 0, 5, 7)] * 2
    paths, n_steps, used = b.sample_paths(streams)
    assert n_steps[0] == -1 and paths[1] == wr.sibling_walk(m, wr.WordSource(streams[1])).states
    assert b.sample_paths(streams, cap=4)[1] == [-1, -3]
    assert b.sample_paths([[], streams[1][:5]])[1] == [-1, -6]
    with pytest.raises(capi.HxError) as e:
        b.read_cells(1, [(0, 0, 11)])
    assert e.value.code == -8
    b.close()
