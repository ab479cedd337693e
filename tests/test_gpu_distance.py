"""hx_distance_matrix / hx_distance_neg_log_like (historian_amd/csrc/hx_distance.hip) against tests/tree_ref.py.

What is compared, and why so tightly.  exp(R t) on the device performs the host's IEEE operations in the host's order, so it
has the host's bits; tJC's log is taken on the host.  The one operation of a likelihood evaluation whose rounding may differ
is the device's log(p_ab), and the terms n_ab log(p_ab) are added in one fixed order on both sides:

  * f(t) agrees to 1e-13 relative: each log within 1 ulp on either side, at most 400 same-sign terms added in one order,
    (2 + 400 / 2) * 1.1e-16 < 3e-14.
  * a distance is the outcome of comparisons of such values.  Where every comparison of a pair's search has a relative gap
    of 1e-9 or more in tree_ref (the project's near-tie tolerance, hx_trace.hip) the device takes the same branches and the
    distance has the same bits.  A pair with a narrower gap somewhere is `flagged`: its distance must be finite and inside
    the bracket, and at most 2 % of the pairs of a matrix may be flagged.  On the 903 pairs of the PF16593 fixture tree_ref
    flags 4 with the restated series on the CPU (as it does with scipy's expm); the 6 pairs of testnj.fa: none."""
import os

import numpy as np
import pytest

from tests import stream_helpers as SH       # (imports torch before the library is loaded: one HIP runtime)
from historian_amd import capi
from oracle import c_oracle
from oracle import historian_oracle as ho
from tests import tree_ref as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden", "reference_data") + os.sep
M = os.path.join(ROOT, "tests", "golden", "models") + os.sep
NEAR_TIE = 1e-9
F_BOUND = 1e-13


class Model:
    """what tree_ref and capi need of a rate model"""

    def __init__(self, alphabet, sub_rate, cpt_weight):
        self.alphabet = alphabet
        self.sub_rate = [np.asarray(r, dtype=np.float64) for r in sub_rate]
        self.cpt_weight = [float(w) for w in cpt_weight]

    def components(self):
        return len(self.sub_rate)

    @staticmethod
    def of(path, scale=1.):
        m = ho.RateModel.from_file(path)
        return Model(m.alphabet, [np.asarray(r) * scale for r in m.sub_rate], m.cpt_weight)


def random_reversible(a, seed):
    """a reversible rate matrix over `a` symbols: symmetric exchangeabilities times a random equilibrium"""
    rng = np.random.RandomState(seed)
    s = rng.gamma(1., 1., (a, a))
    s = s + s.T
    pi = rng.dirichlet(np.full(a, 5.))
    r = s * pi[None, :]
    np.fill_diagonal(r, 0.)
    np.fill_diagonal(r, -r.sum(axis=1))
    return Model("".join(chr(48 + k) for k in range(a)), [r], [1.])


@pytest.fixture(scope="module", autouse=True)
def engine():
    capi.init(0, c_oracle.table())
    yield
    capi.shutdown()


@pytest.fixture(scope="module")
def jc():
    return Model.of(G + "testnj.jukescantor.json")


@pytest.fixture(scope="module")
def amino():
    return Model.of(G + "testamino.json")


@pytest.fixture(scope="module")
def prot4():
    return Model.of(M + "prot4.json")


def device_matrix(model, esr, tok, max_iterations=100, stream=None):
    return capi.distance_matrix(np.stack(model.sub_rate), model.cpt_weight, esr, tok, max_iterations, stream=stream)


_searches = {}


def reference(model, esr, tok, max_iterations=100):
    """tree_ref's distances, evaluations and flags for a token matrix; one search per distinct count table"""
    n = tok.shape[0]
    dist, infos = np.zeros((n, n)), {}
    for i in range(n - 1):
        for j in range(i + 1, n):
            counts = T.counts_from_tokens(tok[i], tok[j])
            key = (id(model), esr, max_iterations, tuple(sorted(counts.items())))
            if key not in _searches:
                s = T.Search(model, counts, esr)
                _searches[key] = (s.t_ml(max_iterations), dict(evaluations=s.evaluations, min_gap=s.min_gap, t_lower=s.t_lower, t_upper=s.t_upper))
            dist[i, j] = dist[j, i] = _searches[key][0]
            infos[(i, j)] = _searches[key][1]
    return dist, infos


def assert_rule_2(got, evals, want, infos, what, searched=True):
    """bit for bit except flagged pairs; a flagged pair finite and inside its bracket; at most 2 % flagged"""
    n = got.shape[0]
    assert np.array_equal(got, got.T) and not got.diagonal().any(), what + ": not symmetric with a zero diagonal"
    pairs = sorted(infos)
    flagged = [ij for ij in pairs if infos[ij]["min_gap"] < NEAR_TIE]
    print("%s: %d pairs, %d flagged %s" % (what, len(pairs), len(flagged), flagged))
    assert len(flagged) <= .02 * len(pairs), what + ": more than 2 %% of the pairs are near ties: %s" % flagged
    for p, (i, j) in enumerate(pairs):
        if (i, j) in flagged:
            assert np.isfinite(got[i, j]) and infos[(i, j)]["t_lower"] <= got[i, j] <= infos[(i, j)]["t_upper"], (what, i, j, got[i, j])
        else:
            assert float(got[i, j]).hex() == float(want[i][j]).hex(), (what, i, j)
            assert evals[p] == infos[(i, j)]["evaluations"], (what, i, j)
        if searched:
            assert evals[p] > 0, (what, i, j)
    return flagged


def draw_rows(rng, a, n, cols, base_diff=.3, gap=.1):
    """n token rows descended from one random row: a fraction of the columns redrawn, some gapped"""
    base = rng.randint(0, a, cols)
    rows = np.empty((n, cols), dtype=np.int8)
    for r in range(n):
        row = base.copy()
        redo = rng.rand(cols) < base_diff * rng.rand()
        row[redo] = rng.randint(0, a, redo.sum())
        row[rng.rand(cols) < gap] = -1
        rows[r] = row
    return rows


# ---- 1. the likelihood evaluation ---------------------------------------------------------------------------------------
# t from 1e-9 to 20: with the largest |rate| of testamino.json (12.8) that is every row of the series' table - sup-norms below
# .01, .1, 1, 10, 100 and 1000 - and with the rates times eight the squarings added beyond the table (norm 2044).
T_GRID = [1e-9, 1e-6, 5e-4, 5e-3, .05, .5, 3., 9.99, 20.]


def nll_case(model, seed, ts):
    rng = np.random.RandomState(seed)
    a = len(model.alphabet)
    counts = (rng.randint(0, 6, (len(ts), a, a)) * (rng.rand(len(ts), a, a) < .5)).astype(np.int32)
    counts[0] = 0                                   # no counted column: f = 0
    counts[1][np.arange(a), np.arange(a)] += 3      # every diagonal pair present
    got = capi.distance_neg_log_like(np.stack(model.sub_rate), model.cpt_weight, counts, np.array(ts))
    worst = 0.
    for k, t in enumerate(ts):
        c = {(i, j): int(counts[k, i, j]) for i in range(a) for j in range(a) if counts[k, i, j]}
        want = T.Search(model, c, 1.).neg_log_like(t)
        rel = abs(got[k] - want) / abs(want) if want else abs(got[k])
        worst = max(worst, rel)
    return worst


@pytest.mark.parametrize("name", ["jc", "amino", "prot4", "amino x 8"])
def test_neg_log_like_against_tree_ref(name, jc, amino, prot4):
    model = {"jc": jc, "amino": amino, "prot4": prot4}.get(name) or Model.of(G + "testamino.json", scale=8.)
    shapes = {T.series_shape(float(np.max(np.abs(r * t)))) for r in model.sub_rate for t in T_GRID}
    if name == "amino":
        assert {(5, 1), (5, 4), (7, 5), (9, 7), (10, 10), (8, 14)} <= shapes
    if name == "amino x 8":
        assert (8, 16) in shapes
    worst = nll_case(model, 11, T_GRID)
    print("neg_log_like %s: largest relative difference %.3g" % (name, worst))
    assert worst <= F_BOUND


# ---- 2, 3. the reference's families: distances, then trees ----------------------------------------------------------------
@pytest.fixture(scope="module")
def testnj_family(jc):
    model, names, rows, esr, dist, infos = T.family("testnj.jukescantor.json", "testnj.fa")
    tok = T.tokens(model, rows)
    return dict(model=jc, names=names, esr=esr, tok=tok, dist=dist, infos=infos, device=device_matrix(jc, esr, tok),
                nj="testnj.out.nh", upgma="testupgma.out.nh")


@pytest.fixture(scope="module")
def pf16593_family(amino):
    model, names, rows, esr, dist, infos = T.recorded_family("testamino.json", "PF16593.testspan.fa")
    tok = T.tokens(model, rows)
    return dict(model=amino, names=names, esr=esr, tok=tok, dist=dist, infos=infos, device=device_matrix(amino, esr, tok),
                nj="PF16593.testspan.testnj.nh", upgma="PF16593.testspan.testupgma.nh")


@pytest.fixture(params=["testnj", "PF16593"])
def family(request, testnj_family, pf16593_family):
    return {"testnj": testnj_family, "PF16593": pf16593_family}[request.param]


def test_family_distances_are_tree_refs(family):
    got, evals = family["device"]
    assert_rule_2(got, evals, family["dist"], family["infos"], family["nj"])


def test_family_trees_from_the_device_matrix_are_the_references(family):
    got, _ = family["device"]
    dist = got.tolist()
    assert T.to_newick(T.neighbor_joining(family["names"], dist)) + "\n" == open(G + family["nj"]).read()
    assert T.to_newick(T.upgma(family["names"], dist)) + "\n" == open(G + family["upgma"]).read()


def test_two_calls_give_the_same_bits(pf16593_family):
    f = pf16593_family
    again, evals = device_matrix(f["model"], f["esr"], f["tok"])
    assert again.tobytes() == f["device"][0].tobytes() and np.array_equal(evals, f["device"][1])


def test_on_a_delayed_stream(pf16593_family):
    # the call returns when its work is done, so "still busy" is checked immediately before it (tests/test_gpu_streams.py)
    f = pf16593_family
    SH.one_hip_runtime()
    s = SH.Streams()
    try:
        a = s.new()
        s.busy(a)
        SH.assert_busy(a, "distance_matrix")
        got, evals = device_matrix(f["model"], f["esr"], f["tok"], stream=SH.handle(a))
        assert a.query() is True, "distance_matrix returned before its stream had drained"
    finally:
        s.release()
    assert got.tobytes() == f["device"][0].tobytes() and np.array_equal(evals, f["device"][1])


# ---- 4. the smallest shapes that can still go wrong ----------------------------------------------------------------------
def check_shape(model, tok, what, max_iterations=100):
    esr = T.expected_sub_rate(model)
    got, evals = device_matrix(model, esr, tok, max_iterations)
    want, infos = reference(model, esr, tok, max_iterations)
    return got, assert_rule_2(got, evals, want, infos, what, searched=max_iterations > 0)


def test_two_sequences(jc):
    rng = np.random.RandomState(2)
    check_shape(jc, draw_rows(rng, 4, 2, 30), "n_seqs = 2")


def test_more_pairs_than_wavefronts_at_once(jc):
    # 65 rows, 2080 pairs and as many wavefronts; the rows are 13 distinct ones, so tree_ref runs 91 searches at most
    rng = np.random.RandomState(3)
    base = draw_rows(rng, 4, 13, 40)
    tok = base[rng.permutation(np.arange(65) % 13)]
    got, _ = check_shape(jc, tok, "65 x 40")
    assert len({got[i, j] for i in range(65) for j in range(65)}) > 40


@pytest.mark.parametrize("cols", [1, 5000])
def test_one_column_and_five_thousand(cols, amino):
    rng = np.random.RandomState(cols)
    check_shape(amino, draw_rows(rng, 20, 3, cols, gap=.05), "n_cols = %d" % cols)


def test_rows_without_common_columns_identical_rows_and_a_saturated_pair(jc):
    # Rows 0-8 hold residues in columns 12-39 only: a family, rows 0 and 1 identical.  Rows 9 and 10 hold residues in columns
    # 0-11 only, so they share no column with the family (18 pairs), and differ from one another everywhere: pDiff = 1.  f of
    # a saturated pair flattens towards t = 20, so its comparisons are near ties by nature and tree_ref flags it: it is the
    # one flagged pair of 55 (1.8 %) and must come back finite and inside [1e-9, 20].
    rng = np.random.RandomState(4)
    tok = np.full((11, 40), -1, dtype=np.int8)
    tok[:9, 12:] = draw_rows(rng, 4, 9, 28, gap=0.)
    tok[1] = tok[0]
    tok[9, :12] = np.arange(12) % 4
    tok[10, :12] = (np.arange(12) + 1 + np.arange(12) // 4) % 4
    got, flagged = check_shape(jc, tok, "disjoint / identical / saturated")
    assert flagged == [(9, 10)] and 1e-9 <= got[9, 10] <= 20.
    assert (got[:9, 9:] == 10.).all() and got[0, 1] == 5e-10


@pytest.mark.parametrize("iterations", [0, 3])
def test_no_iterations_and_three(iterations, amino):
    rng = np.random.RandomState(7)
    tok = draw_rows(rng, 20, 4, 60)
    got, _ = check_shape(amino, tok, "max_iterations = %d" % iterations, iterations)
    assert (got[np.triu_indices(4, 1)] > 1e-9).all()


def test_tokens_that_are_all_uncounted(jc):
    got, _ = check_shape(jc, np.full((3, 10), -1, dtype=np.int8), "all -1")
    assert (got[np.triu_indices(3, 1)] == 10.).all()


def test_a_mixture(prot4):
    rng = np.random.RandomState(8)
    check_shape(prot4, draw_rows(rng, 20, 3, 80), "prot4, four components")


def test_thirty_two_symbols():
    model = random_reversible(32, 5)
    rng = np.random.RandomState(9)
    check_shape(model, draw_rows(rng, 32, 3, 200), "A = 32")


def test_rejected_input(jc):
    with pytest.raises(capi.HxError) as e:
        m = random_reversible(33, 1)
        device_matrix(m, 1., np.zeros((3, 5), dtype=np.int8))
    assert e.value.code == capi.HX_ERR_RANGE and "33" in str(e.value)
    with pytest.raises(capi.HxError) as e:
        device_matrix(jc, 1., np.zeros((1, 5), dtype=np.int8))
    assert e.value.code == capi.HX_ERR_INVALID_ARG
    with pytest.raises(capi.HxError) as e:
        device_matrix(jc, 1., np.full((2, 5), 4, dtype=np.int8))          # a token outside the alphabet
    assert e.value.code == capi.HX_ERR_RANGE
