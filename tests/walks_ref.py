"""TEST INFRASTRUCTURE ONLY - CPU restatement of the walks through the pair matrices of SURVEY.md section 8(f) row N4 that
oracle/branch_oracle.py and tests/sibling_ref.py do not hold:

  * Sampler::BranchMatrix::sample (reference src/sampler.cpp:1088-1120) over oracle.branch_oracle.BranchMatrix(viterbi=False),
    BranchMatrixBase::logPathProb (:1122-1154) and Sampler::BranchMatrix::logPostProb (:1156-1160);
  * both sampled walks - the three-state one and SiblingMatrix::sample (:1343-1386, restated in tests/sibling_ref.py) - in a
    form that records what a comparison with another implementation needs: the state chosen at every step (End side first),
    the 32-bit engine words consumed, the visits of IDD, and the walk's MARGIN: the smallest distance, relative to norm,
    between random_key_log's running variate (src/util.h:220-236) and zero, at the chosen state and at the states passed
    over.  A walk whose margin is far above the rounding of exp() is chosen the same by any correctly rounded-or-nearly exp().

Pinned by enumeration in tests/test_oracle_walks.py, like the restatements it stands on."""
import math

from oracle import branch_oracle as bo
from oracle.historian_oracle import NEG_INF
from tests import sibling_ref as sr


class WordSource:
    """the draws of a 32-bit engine whose words are given: random_double (src/util.h:138-142) is one word over 2^32,
    std::geometric_distribution<int>(p) as libstdc++ draws it - floor(log(1 - u) / log(1 - p)) over one canonical double, two
    words, the first the low one (tests/sibling_ref.py MTSource, oracle.historian_oracle.MT19937.canonical)"""

    def __init__(self, words):
        self.words, self.used = [int(w) for w in words], 0

    def next_u32(self):
        if self.used >= len(self.words):
            raise IndexError("out of words")
        self.used += 1
        return self.words[self.used - 1]

    def uniform(self):
        return self.next_u32() / 4294967296.0

    def canonical(self):
        s = float(self.next_u32())
        s = s + float(self.next_u32()) * 4294967296.0
        r = s / 18446744073709551616.0
        return math.nextafter(1.0, 0.0) if r >= 1.0 else r

    def geometric(self, p):
        u = self.canonical()
        return int(math.floor(math.log(1. - u) / math.log(1. - p))) if 0. < p < 1. else 0


def mt_words(seed, n):
    from oracle.historian_oracle import MT19937
    mt = MT19937(seed)
    return [mt.next_u32() for _ in range(n)]


class Walk:
    """states: the state chosen at every step, End side first; rows: the alignment, first column first; margin: see the
    module; idd_visits: steps taken standing in IDD; words_used: None when the source does not count them"""

    def __init__(self, states, rows, margin, idd_visits, words_used):
        self.states, self.rows, self.margin, self.idd_visits, self.words_used = states, rows, margin, idd_visits, words_used


def _walk(m, source, n_states, end, empty, column, lp_emit, self_loop):
    i, j, state = m.x_size - 1, m.y_size - 1, end
    cols, states, margin, idd = [], [], math.inf, 0
    while i > 0 or j > 0:
        col = column(i, j, state)
        if any(col):
            cols.append(col)
        if self_loop(state):      # the self-loop the fill eliminated is drawn outside the step
            idd += 1
            cols.extend([col] * source.geometric(m.idd_self_loop_prob()))
        si, sj = i - col[0], j - col[1]
        e = lp_emit(i, j, state)
        src = m.cells.get((si, sj), empty)
        w = [src[s] + m.T[s][state] + e for s in range(n_states)]
        top = max(w)
        assert top > NEG_INF, "traceback state has zero probability at cell (%d,%d,%d)" % (i, j, state)
        norm = 0.
        for v in w:
            norm += math.exp(v - top)
        variate = source.uniform() * norm
        for s, v in enumerate(w):
            variate -= math.exp(v - top)
            margin = min(margin, abs(variate) / norm)
            if variate <= 0:
                break
        else:
            raise AssertionError("random_key_log failed")
        states.append(s)
        i, j, state = si, sj, s
    rows = tuple([c[r] for c in reversed(cols)] for r in range(len(cols[0]) if cols else 0))
    return Walk(states, rows, margin, idd, getattr(source, "used", None))


class _NoLoop:
    def __init__(self, source):
        self.source = source

    def uniform(self):
        return self.source.uniform()

    @property
    def used(self):
        return getattr(self.source, "used", None)


def branch_column(i, j, state):
    """BranchMatrixBase::getColumn (src/sampler.cpp:1175-1183)"""
    m = state == bo.MATCH and i > 0 and j > 0
    return (m or state == bo.DELETE, m or state == bo.INSERT)


def branch_walk(bm, source):
    """Sampler::BranchMatrix::sample over a BranchMatrix(viterbi=False)"""
    assert not bm.viterbi
    w = _walk(bm, _NoLoop(source), 3, bo.END, (NEG_INF,) * 3, branch_column, bm.lp_emit, lambda s: False)
    if not w.rows:
        w.rows = ([], [])
    return w


def branch_sample(bm, source):
    """-> (x row, y row), first column first"""
    return branch_walk(bm, source).rows


def sibling_walk(m, source):
    """SiblingMatrix::sample; .rows equals tests.sibling_ref.SiblingMatrix.sample(source) from the same draws"""
    w = _walk(m, source, sr.N_STATES, sr.EEE, sr.EMPTY, sr.get_column, m.lp_emit, lambda s: s == sr.IDD)
    if not w.rows:
        w.rows = ([], [], [])
    return w


def branch_rows_of_states(bm, states):
    """the alignment a walk's recorded states spell: what a caller of hx_branch_batch_best_paths / sample_paths rebuilds"""
    i, j, state, cols = bm.x_size - 1, bm.y_size - 1, bo.END, []
    for s in states:
        col = branch_column(i, j, state)
        if any(col):
            cols.append(col)
        i, j, state = i - col[0], j - col[1], s
    assert (i, j) == (0, 0)
    return [c[0] for c in reversed(cols)], [c[1] for c in reversed(cols)]


def best_states(bm):
    """Refiner::BranchMatrix::best (oracle.branch_oracle.BranchMatrix.best) with the chosen states recorded, End side first"""
    i, j, state, states = bm.x_size - 1, bm.y_size - 1, bo.END, []
    while i > 0 or j > 0:
        x, y = branch_column(i, j, state)
        si, sj = i - x, j - y
        e = 0. if state == bo.END else bm.lp_emit(i, j, state)
        best_lp, best_s = NEG_INF, None
        for s in (bo.MATCH, bo.INSERT, bo.DELETE):
            lp = bm.cell(si, sj, s) + bm.T[s][state] + e
            if lp > best_lp:
                best_lp, best_s = lp, s
        assert best_s is not None, "could not find traceback state"
        states.append(best_s)
        i, j, state = si, sj, best_s
    return states


def get_state(dx, dy):
    """ProbModel::getState (src/model.h): the state of a column with the parent (dx) / the child (dy) ungapped"""
    return bo.MATCH if dx and dy else (bo.INSERT if dy else bo.DELETE)


def branch_log_path_prob(bm, path, cell=None, lp_emit=None):
    """BranchMatrixBase::logPathProb (src/sampler.cpp:1122-1154) of (x row, y row); cell(i, j, state) and lp_emit(i, j, state)
    may come from elsewhere (cells gathered from a device-resident matrix)"""
    cell = cell or bm.cell
    lp_emit = lp_emit or bm.lp_emit
    lp, i, j, state = 0., 0, 0, bo.MATCH
    for dx, dy in zip(*path):
        if dx:
            i += 1
        if dy:
            j += 1
        prev, state = state, get_state(dx, dy)
        if i >= bm.x_size or j >= bm.y_size or not bm.in_envelope(i, j):
            return NEG_INF
        lp += bm.T[prev][state] + lp_emit(i, j, state)
        lp = min(lp, cell(i, j, state))          # "mitigate precision errors"
    return lp + bm.T[state][bo.END]


def branch_log_post_prob(bm, path, cell=None, lp_emit=None, lp_end=None):
    """Sampler::BranchMatrix::logPostProb (src/sampler.cpp:1156-1160)"""
    lp_end = bm.lp_end if lp_end is None else lp_end
    return min(branch_log_path_prob(bm, path, cell, lp_emit), lp_end) - lp_end


def path_cells_branch(path):
    """the (i, j, state) a logPathProb of the path reads, in order"""
    out, i, j = [], 0, 0
    for dx, dy in zip(*path):
        i, j = i + bool(dx), j + bool(dy)
        out.append((i, j, get_state(dx, dy)))
    return out


def path_cells_sibling(path):
    """the (i, j, state) SiblingMatrix::logPostProb (src/sampler.cpp:1388-1412) reads, in order"""
    out, i, j, state = [], 0, 0, sr.SSS
    for dl, dr, dp in zip(*path):
        i, j = i + bool(dl), j + bool(dr)
        state = sr.get_state(state, dl, dr, dp)
        out.append((i, j, state))
    return out
