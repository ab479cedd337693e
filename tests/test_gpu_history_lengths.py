"""Proposals to the resident history as (node, branch length) pairs: exp(R t) computed on the device (k_branch_expm,
hx_expm.hip) where the column kernel reads it.

The reference is oracle.historian_oracle.sub_prob_matrix_ss - the restated gsl_linalg_exponential_ss that the C++ mirror's
RateModel::getSubProbMatrix agrees with bit for bit (tests/test_host_mirror.py) - and every comparison is of bit patterns.
tests.history_ref.oracle_sub_prob is NOT that function: it is ho.ProbModel's default, scipy's Pade expm (or the closed form
of a uniform model), which differs from the series around 1e-13; its distance from the device's matrices is printed, not
asserted.  The matrices of the larger alphabets come from tests/tree_ref._sub_prob, the same operations in numpy
(tests/test_oracle_tree.py holds it to sub_prob_matrix_ss's bits; here it is held to them again on the small models)."""
import functools
import json
import math
import os

import numpy as np
import pytest

from historian_amd import capi, counts, hostmodel
from oracle import c_oracle
from oracle import historian_oracle as ho
from tests import history_ref as HR
from tests import stream_helpers as SH
from tests import tree_ref
from tests.sumprod_edge_cases import JUKES_CANTOR, SYMBOLS
from tests.test_gpu_ancestors import CYCLIC, PROT4, _recon_columns
from tests.test_gpu_history import case as history_case
from tests.test_gpu_sumprod import _random_model, _random_tree

pytestmark = pytest.mark.gpu
THRESHOLDS = (0.01, 0.1, 1., 10., 100., 1000.)
ROW_NORMS = (.004, .04, .4, 4., 40., 400., 2500.)       # one norm inside each of the seven rows of GSL's table


@pytest.fixture(scope="module", autouse=True)
def engine():
    capi.init(0, c_oracle.table())
    yield
    capi.shutdown()


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def ss(rate, t):
    """[C][A][A]: the bits of sub_prob_matrix_ss of every component"""
    return np.asarray([tree_ref._sub_prob(r, t) for r in rate])


def table_row(norm):
    return sum(norm >= below for below in THRESHOLDS)


def _mixture(rng, a):
    """two components over SYMBOLS[:a]: a reversible one and one with a cyclic drift, weights 2 : 1"""
    alphabet = SYMBOLS[:a]
    one, two = _random_model(rng, alphabet, True), _random_model(rng, alphabet, False)
    js = {k: one[k] for k in ("alphabet", "insrate", "delrate", "insextprob", "delextprob")}
    js["mixture"] = [dict(subrate=one["subrate"], rootprob=one["rootprob"], weight=2.), dict(subrate=two["subrate"], rootprob=two["rootprob"], weight=1.)]
    return js


class Model:
    """A model on a tree of 9 nodes with 10 columns; its rate matrices are the oracle's"""

    def __init__(self, name):
        rng = np.random.default_rng(100 + len(name))
        if name == "dna":
            js = JUKES_CANTOR
        elif name == "prot4":
            with open(PROT4) as f:
                js = json.load(f)
        elif name == "cyclic":
            js = CYCLIC
        else:
            js = _mixture(rng, int(name[1:]))
        self.omodel, self.model = ho.RateModel(js), hostmodel.RateModel(js)
        self.rate = np.asarray(self.omodel.sub_rate, dtype=np.float64)
        assert bits(self.rate).tobytes() == bits(np.asarray(self.model.sub_rate)).tobytes()          # the product's model has the oracle's rates
        self.c, self.a = self.rate.shape[:2]
        self.parent, self.length = _random_tree(rng, 5)
        self.n = len(self.parent)
        self.rows = _recon_columns(rng, self.parent, js["alphabet"], 10)
        self.tokens = counts.tokenize_columns(self.model.alphabet, self.rows)
        self.ins_prob = np.asarray(self.model.root, dtype=float).reshape(self.c, self.a)
        self.log_cpt_weight = np.log(np.asarray(self.model.cpt_weight, dtype=float))
        self.max_abs = [float(np.abs(r).max()) for r in self.rate]

    def history(self, length=None):
        return capi.History.from_lengths(self.parent, self.ins_prob, self.log_cpt_weight, self.tokens, self.rate, self.length if length is None else length)

    def lengths(self):
        """[(t, what, row)]: 0; a length in each row of the table for the component with the largest rates; lengths whose norm is
        the last double below and the first one not below 1 and 10.  The row is asserted here, on the host."""
        top = max(self.max_abs)
        out = [(0., "t = 0", 0)]
        for row, norm in enumerate(ROW_NORMS):
            out.append((norm / top, "row %d" % row, row))
        for at, row in ((1., 2), (10., 3)):
            t = at / top
            while top * t >= at:
                t = float(np.nextafter(t, 0.))
            while top * float(np.nextafter(t, math.inf)) < at:
                t = float(np.nextafter(t, math.inf))
            out.append((t, "norm just below %g" % at, row))
            out.append((float(np.nextafter(t, math.inf)), "norm just above %g" % at, row + 1))
        for t, what, row in out:
            norm = float(np.max(np.abs(self.rate[int(np.argmax(self.max_abs))] * t)))
            assert table_row(norm) == row, (what, norm)
            assert norm == top * t                                                 # what hx_expm_shape is given
        below, above = out[8], out[9]
        assert top * below[0] < 1. <= top * above[0] and top * out[10][0] < 10. <= top * out[11][0]
        return out


@functools.lru_cache(maxsize=None)
def model(name):
    return Model(name)


@functools.lru_cache(maxsize=None)
def reference(name):
    """{t: [C][A][A]} the oracle's matrices of the model's lengths, computed once"""
    m = model(name)
    return {t: ss(m.rate, t) for t, _, _ in m.lengths()}


MODELS = ["dna", "prot4", "cyclic", "r5", "r21", "r33", "r64"]


# ---- (a) the matrices ----

@pytest.mark.parametrize("name", ["dna", "cyclic", "r5"])
def test_the_numpy_restatement_has_the_oracles_bits(name):
    """(no device) sub_prob_matrix_ss itself, with its skipped zero factors, on the models small enough for it"""
    m = model(name)
    for t, what, _ in m.lengths():
        for cpt in range(m.c):
            want = np.asarray(ho.sub_prob_matrix_ss(m.rate[cpt].tolist(), t))
            assert bits(want).tobytes() == bits(reference(name)[t][cpt]).tobytes(), (what, cpt)
    if name == "cyclic":
        assert np.count_nonzero(m.rate[0] == 0.) >= 4                              # exact zeros: the skipped-factor rule is exercised


@pytest.mark.parametrize("name", MODELS)
def test_the_matrices_bit_for_bit(name):
    """branch_matrix(node, 1) after propose_lengths, every length of Model.lengths on the eight branches in turn"""
    m = model(name)
    assert m.n == 9 and (m.a, m.c) == {"dna": (4, 1), "prot4": (20, 4), "cyclic": (4, 1)}.get(name, (int(name[1:]) if name[0] == "r" else 0, 2))
    lengths, want = m.lengths(), reference(name)
    pade = HR.oracle_sub_prob(m.omodel)
    h = m.history()
    current = [h.branch_matrix(r) for r in range(m.n - 1)]
    for r in range(m.n - 1):                                                       # create_from_lengths put exp(R t) of every branch in place
        assert bits(current[r]).tobytes() == bits(ss(m.rate, m.length[r])).tobytes(), r
    worst_pade = 0.
    for start in range(0, len(lengths), m.n - 1):
        chunk = lengths[start:start + m.n - 1]
        nodes = [(start + k) % (m.n - 1) for k in range(len(chunk))]
        h.propose_lengths(nodes, [t for t, _, _ in chunk])
        for node, (t, what, row) in zip(nodes, chunk):
            got = h.branch_matrix(node, 1)
            shapes = [capi.expm_shape(top, t)[:2] for top in m.max_abs]
            differ = np.argwhere(bits(got) != bits(want[t]))
            assert differ.size == 0, (name, what, shapes, differ[:4], got[tuple(differ[0])], want[t][tuple(differ[0])])
            assert bits(h.branch_matrix(node, 0)).tobytes() == bits(current[node]).tobytes()      # the current slot is untouched
            if t == 0.:
                assert bits(got).tobytes() == bits(np.tile(np.eye(m.a), (m.c, 1, 1))).tobytes()     # the identity exactly, +0 off the diagonal
            elif row < 5:
                worst_pade = max(worst_pade, float(np.max(np.abs(got - np.asarray(pade(t))))))
        for node in range(m.n - 1):                                                # a node outside the proposal: which = 1 gives the current one
            if node not in nodes:
                assert bits(h.branch_matrix(node, 1)).tobytes() == bits(current[node]).tobytes()
        h.reject()
    print("%s: %d lengths x %d components bit for bit; largest |device - history_ref.oracle_sub_prob| (scipy) %.3g" % (name, len(lengths), m.c, worst_pade))
    h.close()


def test_the_bits_do_not_depend_on_the_waves_of_a_workgroup(monkeypatch):
    """A = 20 takes seven waves (one entry a lane); one, two, four and eight (seven, four, two and one entries a lane;
    HX_EXPM_WAVES, read when a history is given its rates) must give the same matrices"""
    m = model("prot4")
    lengths, want = m.lengths(), reference("prot4")
    for waves in ("1", "2", "4", "8"):
        monkeypatch.setenv("HX_EXPM_WAVES", waves)
        h = m.history()
        chunk = lengths[1:m.n]
        h.propose_lengths(list(range(m.n - 1)), [t for t, _, _ in chunk])
        for node, (t, what, _) in enumerate(chunk):
            assert bits(h.branch_matrix(node, 1)).tobytes() == bits(want[t]).tobytes(), (waves, what)
        h.close()


# ---- (b) evaluations: 17 nodes x 130 columns of the 4 x 20 mixture, as tests/test_gpu_history.py ----

class Evaluations:
    def __init__(self):
        c = history_case("prot4")
        self.c = c
        self.rate = np.asarray(c.omodel.sub_rate, dtype=np.float64)
        self._mats = {}

    def mats(self, t):
        if t not in self._mats:
            self._mats[t] = ss(self.rate, t)
        return self._mats[t]

    def matrices(self, length):
        out = np.zeros((self.c.c, self.c.n, self.c.a, self.c.a))
        for r in range(self.c.n - 1):
            out[:, r] = self.mats(length[r])
        return out

    def from_lengths(self, length, stream=None):
        c = self.c
        return capi.History.from_lengths(c.parent, c.ins_prob, c.log_cpt_weight, c.tokens, self.rate, length, stream=stream)

    def fresh(self, length):
        """what a history created with the oracle's matrices of `length` holds"""
        h = self.c.history(branch_sub=self.matrices(length))
        out = h.log_like()
        h.close()
        return out

    def fresh_proposal(self, length, nodes, proposed):
        """the issue's reference: `propose` with the oracle's matrices of the proposed lengths on a history freshly created
        with the oracle's matrices of `length` -> (lp_sub, col_log_like) of that proposal.  (tests/test_gpu_history.py pins
        such a proposal to a history created on the proposed tree, bit for bit; both are asserted equal here.)"""
        h = self.c.history(branch_sub=self.matrices(length))
        lp = h.propose(nodes, np.asarray([self.mats(proposed[r]) for r in nodes]))
        out = h.log_like(1)
        h.close()
        assert lp == out[0] and same(out, self.fresh(proposed))
        return out


@functools.lru_cache(maxsize=None)
def evaluations():
    return Evaluations()


def same(a, b):
    return a[0] == b[0] and a[1].tobytes() == b[1].tobytes()


def test_creation_from_lengths_is_creation_from_the_oracles_matrices_and_two_runs_agree():
    e = evaluations()
    assert (e.c.n, len(e.c.want)) == (17, 130)
    want = e.fresh(e.c.length)
    h, again = e.from_lengths(e.c.length), e.from_lengths(e.c.length)
    assert same(h.log_like(), want) and same(again.log_like(), want)
    assert h.kernel_ms() > 0
    lp = [x.propose_lengths([0, 3, 7], [.11, .22, .33]) for x in (h, again)]
    assert lp[0] == lp[1] and same(h.log_like(1), again.log_like(1))
    for r in (0, 3, 7):
        assert h.branch_matrix(r, 1).tobytes() == again.branch_matrix(r, 1).tobytes()
    h.close()
    again.close()


def test_proposals_of_lengths_are_proposals_of_the_oracles_matrices():
    """every internal node's {node, children} through propose_lengths, against `propose` with the oracle's matrices on a
    freshly created history; alternately rejected and accepted (the next one builds on it); at every third node the same
    proposal is first made with matrices and rejected, so that a matrices proposal stands between two lengths proposals and
    the lengths proposal after it finds the slots where it left them; then every branch at once"""
    e = evaluations()
    c = e.c
    child = ts_children(c.parent)
    rng = np.random.default_rng(6)
    h = e.from_lengths(c.length)
    length, current = list(c.length), h.log_like()
    n_internal = n_interleaved = 0
    for node in range(c.n):
        if not child[node]:
            continue
        n_internal += 1
        nodes = list(child[node]) + ([node] if node != c.n - 1 else [])
        proposed = list(length)
        for r in nodes:
            proposed[r] = float(rng.uniform(.01, .8))
        want = e.fresh_proposal(length, nodes, proposed)
        if n_internal % 3 == 0:
            n_interleaved += 1
            lp = h.propose(nodes, np.asarray([e.mats(proposed[r]) for r in nodes]))
            assert lp == want[0] and same(h.log_like(1), want), node
            for r in nodes:
                assert bits(h.branch_matrix(r, 1)).tobytes() == bits(e.mats(proposed[r])).tobytes()
            h.reject()
            assert same(h.log_like(0), current), node
        lp = h.propose_lengths(nodes, [proposed[r] for r in nodes])
        got = h.log_like(1)
        assert lp == got[0] and same(got, want), node
        assert want[0] != current[0] and same(h.log_like(0), current), node
        for r in nodes:
            assert bits(h.branch_matrix(r, 1)).tobytes() == bits(e.mats(proposed[r])).tobytes() and bits(h.branch_matrix(r, 0)).tobytes() == bits(e.mats(length[r])).tobytes()
        if node % 2:
            h.reject()
            assert same(h.log_like(0), current), node
        else:
            h.accept()
            assert same(h.log_like(0), want), node
            length, current = proposed, want
    assert n_internal == 8 and n_interleaved == 2
    # a second proposal on top of a rejected and of an accepted one was each step above; now every branch (the rescale move)
    nodes = list(range(c.n - 1))
    proposed = [t * 1.37 for t in length]
    want = e.fresh_proposal(length, nodes, proposed)
    assert h.propose_lengths(nodes, proposed[:-1]) == want[0] and same(h.log_like(1), want)
    h.accept()
    assert same(h.log_like(0), want)
    for r in nodes:
        assert bits(h.branch_matrix(r)).tobytes() == bits(e.mats(proposed[r])).tobytes()
    h.close()


def ts_children(parent):
    child = [[] for _ in parent]
    for r, p in enumerate(parent):
        if p >= 0:
            child[p].append(r)
    return child


def test_rates_given_to_a_history_of_matrices():
    """hx_history_set_rates on a history created from matrices: lengths proposals from then on, matrices still"""
    e = evaluations()
    c = e.c
    h = c.history(branch_sub=e.matrices(c.length))
    h.set_rates(e.rate)
    proposed = list(c.length)
    proposed[2], proposed[5] = .4, .04
    want = e.fresh(proposed)
    assert h.propose_lengths([5, 2], [.04, .4]) == want[0] and same(h.log_like(1), want)
    h.reject()
    assert h.propose([2, 5], np.asarray([e.mats(.4), e.mats(.04)])) == want[0]
    h.close()


# ---- (c) refusals ----

def _code(fn):
    with pytest.raises(capi.HxError) as e:
        fn()
    return e.value.code


def test_every_refusal_and_that_nothing_ran():
    m = model("cyclic")
    ok = dict(parent=m.parent, ins_prob=m.ins_prob, log_cpt_weight=m.log_cpt_weight, tokens=m.tokens, rate=m.rate, lengths=m.length)

    def create(**kw):
        return lambda: capi.History.from_lengths(**dict(ok, **kw))
    for bad in (-1e-300, math.nan, math.inf, -math.inf, 1.7e308):                     # (1.7e308: max|R| t overflows)
        lengths = list(m.length)
        lengths[3] = bad
        assert _code(create(lengths=lengths)) == -8, bad
    lengths = list(m.length)
    lengths[m.n - 1] = math.nan                                                    # the root's is not read
    capi.History.from_lengths(**dict(ok, lengths=lengths)).close()
    for bad in (math.nan, math.inf):
        rate = m.rate.copy()
        rate[0, 1, 2] = bad
        assert _code(create(rate=rate)) == -8
    assert _code(create(parent=[-1] + list(m.parent[1:]))) == -5                   # hx_history_create's own refusals come first

    # a history without rates
    plain = capi.History(m.parent, m.ins_prob, m.log_cpt_weight, m.tokens, np.tile(np.eye(m.a), (m.c, m.n, 1, 1)))
    ms, state = plain.kernel_ms(), plain.log_like()
    plain_mats = [plain.branch_matrix(r) for r in range(m.n - 1)]
    assert _code(lambda: plain.propose_lengths([0], [.1])) == -7
    assert plain.kernel_ms() == ms and same(plain.log_like(), state)
    for r in range(m.n - 1):
        assert plain.branch_matrix(r, 0).tobytes() == plain_mats[r].tobytes()
    plain.close()

    h = m.history()
    ms, state, mats = h.kernel_ms(), h.log_like(), [h.branch_matrix(r) for r in range(m.n - 1)]

    def unchanged(ms_now=None):
        assert h.kernel_ms() == (ms if ms_now is None else ms_now) and same(h.log_like(0), state)
        for r in range(m.n - 1):
            assert h.branch_matrix(r, 0).tobytes() == mats[r].tobytes()
    assert ms > 0
    for bad in (-.1, -1e-300, math.nan, math.inf, -math.inf, 1.7e308):
        assert _code(lambda: h.propose_lengths([1, 0], [.1, bad])) == -8, bad       # a length that is negative, NaN or infinite
        unchanged()
    for node in (-1, m.n - 1, m.n):                                                # outside 0 .. N - 2; N - 1 is the root
        assert _code(lambda: h.propose_lengths([node], [.1])) == -8
        unchanged()
        assert _code(lambda: h.branch_matrix(node)) == -8
    assert _code(lambda: h.propose_lengths([2, 2], [.1, .2])) == -1                # a node named twice
    unchanged()
    assert _code(lambda: h.propose_lengths([], [])) == -1
    unchanged()
    assert _code(lambda: h.branch_matrix(0, 1)) == -7                              # nothing pending
    assert _code(lambda: h.branch_matrix(0, 2)) == -1
    assert _code(h.accept) == -7 and _code(h.reject) == -7
    unchanged()
    rate = m.rate.copy()
    rate[0, 0, 0] = math.nan
    assert _code(lambda: h.set_rates(rate)) == -8
    unchanged()
    h.propose_lengths([0], [.3])                                                   # (the refused set_rates left the rates in place)
    ms2, proposed, new0 = h.kernel_ms(), h.log_like(1), h.branch_matrix(0, 1)
    assert bits(new0).tobytes() == bits(ss(m.rate, .3)).tobytes()
    assert _code(lambda: h.propose_lengths([1], [.2])) == -7                       # a proposal is pending
    unchanged(ms2)
    assert _code(lambda: h.propose([1], mats[1][None])) == -7
    unchanged(ms2)
    assert _code(lambda: h.set_rates(m.rate)) == -7
    unchanged(ms2)
    assert same(h.log_like(1), proposed) and h.branch_matrix(0, 1).tobytes() == new0.tobytes()
    h.reject()
    unchanged(ms2)
    h.close()


# ---- (d) streams ----

def test_lengths_on_a_delayed_stream():
    """create_from_lengths and propose_lengths return when their kernels are done, so "still busy" is checked immediately
    before each; the expm kernel, the column kernel and the sum all follow the delay on the caller's stream"""
    SH.one_hip_runtime()
    SH.cycles_per_ms()
    m = model("r21")
    proposed = [t * .8 for t in m.length]
    nodes = [0, 1, m.parent[0]] if m.parent[0] == m.parent[1] else [0, m.parent[0]]
    h = m.history()
    want = (h.log_like(), h.propose_lengths(nodes, [proposed[r] for r in nodes]), h.log_like(1), [h.branch_matrix(r, 1) for r in nodes])
    h.close()
    streams = SH.Streams()
    try:
        a = streams.new()
        streams.busy(a)
        SH.assert_busy(a, "History.from_lengths")
        h = capi.History.from_lengths(m.parent, m.ins_prob, m.log_cpt_weight, m.tokens, m.rate, m.length, stream=SH.handle(a))
        got0 = h.log_like()
        streams.busy(a)
        SH.assert_busy(a, "History.propose_lengths")
        lp = h.propose_lengths(nodes, [proposed[r] for r in nodes], stream=SH.handle(a))
        got1, mats = h.log_like(1), [h.branch_matrix(r, 1) for r in nodes]
    finally:
        streams.release()
    h.close()
    assert same(got0, want[0]) and lp == want[1] and same(got1, want[2])
    for got, w in zip(mats, want[3]):
        assert got.tobytes() == w.tobytes()
