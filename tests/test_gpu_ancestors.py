"""Ancestral sequence prediction on the device: hx_sumprod_ancestors (node posteriors of every column, the most probable
residue of every wildcard) against the sum-product oracle's log_node_post_prob, node by node.

The reference's own reconstruction of PF16593 first (85 nodes: the upper nodes pass through the 1e-30 rescaling), then
seeded reconstruction-shaped columns - internal nodes wildcards, child subtrees dropped independently, so that a kept child
next to a gap occurs as a real deletion produces it - on the 4-component protein mixture and on a cyclic DNA model, whole
and in chunks; the Jukes-Cantor fixture whose exact tie rounding decides; alphabets without a kernel of their own; edge
columns; agreement with hx_sumprod_columns at the column's root; the stream contract.

Bounds: exp(node_post) within 1e-8 relative of the oracle's (the bound of tests/test_gpu_sumprod.py for root posteriors:
the device's log() and the order of the sums in the matrix-vector products differ from libm's and numpy's), column
likelihoods within 1e-12 relative, `best` equal wherever the oracle's top-two gap is at least 1e-6."""
import functools
import json
import math
import os

import numpy as np
import pytest

from historian_amd import capi, counts, hostmodel
from oracle import c_oracle
from oracle import historian_oracle as ho
from oracle import sumprod_oracle as so
from oracle.ref_mains import read_fasta
from tests import ancestors_ref as AR
from tests import stream_helpers as SH
from tests.recon_helpers import parse_newick
from tests.test_gpu_sumprod import _fixture, _random_model, _random_tree

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden", "reference_data") + os.sep
PROT4 = os.path.join(ROOT, "tests", "golden", "models", "prot4.json")
CYCLIC = {"alphabet": "acgt", "insrate": .01, "delrate": .01, "insextprob": .5, "delextprob": .5,
          "rootprob": {"a": .1, "c": .2, "g": .3, "t": .4},
          "subrate": {"a": {"c": 1., "g": .1}, "c": {"g": 1.2, "t": .05}, "g": {"t": .9, "a": .02}, "t": {"a": 1.1, "c": .3}}}


@pytest.fixture(scope="module", autouse=True)
def engine():
    capi.init(0, c_oracle.table())
    yield
    capi.shutdown()


def _recon_columns(rng, parent, alphabet, n_cols):
    """Columns shaped like a reconstruction's: the column's root is the tree's or, with probability .3, any node; every
    child subtree is kept with probability .85 on its own (a kept child beside a gap: a deletion); internal nodes are
    '*', leaves a residue or, with probability .03, 'x'."""
    n = len(parent)
    child = [[] for _ in range(n)]
    for r, p in enumerate(parent):
        if p >= 0:
            child[p].append(r)
    rows = [[] for _ in range(n)]
    for _ in range(n_cols):
        col = ["-"] * n
        root = int(rng.integers(0, n)) if rng.random() < .3 else n - 1
        stack = [root]
        while stack:
            r = stack.pop()
            if child[r]:
                col[r] = "*"
                stack.extend(c for c in child[r] if rng.random() < .85)
            else:
                col[r] = "x" if rng.random() < .03 else alphabet[int(rng.integers(0, len(alphabet)))]
        for r in range(n):
            rows[r].append(col[r])
    return ["".join(r) for r in rows]


class Case:
    """A model, a tree, columns; the device's inputs and, computed once and never changed, the oracle's posteriors."""

    def __init__(self, js, parent, length, rows, every=1):
        self.omodel, self.model = ho.RateModel(js), hostmodel.RateModel(js)
        self.parent, self.length, self.rows = parent, length, rows
        self.tree = so.Tree(parent, length, ["n%d" % k for k in range(len(parent))])
        self.sp = so.SumProduct(self.omodel, self.tree)
        n, c, a = len(parent), self.sp.C, self.sp.A
        # the device gets the oracle's exp(R t) so that the comparison is of the passes, not of two matrix exponentials
        self.branch_sub = [[self.sp.branch_sub[cpt][r] if parent[r] >= 0 else np.zeros((a, a)) for cpt in range(c)] for r in range(n)]
        self.tokens = counts.tokenize_columns(self.model.alphabet, rows)
        self.want = {}                     # column -> (col_log_like, {node: [A] log posteriors} of the ungapped nodes)
        for col, seq in enumerate(so.columns_of(self.tree, dict(enumerate(rows)))):
            if col % every:
                continue
            self.sp.init_column(seq)
            self.sp.fill_up()
            self.sp.fill_down()
            self.want[col] = (self.sp.col_log_like, {r: self.sp.log_node_post_prob(r) for r in self.sp.ungapped})

    def predictor(self):
        return counts.AncestorPredictor(self.model, self.parent, self.length, branch_sub=self.branch_sub)

    def check(self, got):
        """every node of every checked column; -> (wildcard cells seen, worst relative deviation of a posterior)"""
        cll, best, post = got["col_log_like"], got["best"], got["node_post"]
        a = len(self.model.alphabet)
        cells, worst, min_gap = 0, 0., math.inf
        for col, (want_ll, lpp) in self.want.items():
            # 1e-12 relative; an all-wildcard column's likelihood is 1 and its logarithm what the table log_sum_exp leaves of
            # log(1/C)'s (3.5e-7 in the oracle too): the floor of tests/test_gpu_sumprod.py for that column
            # (the floor only there: every other column keeps the purely relative bound)
            assert abs(cll[col] - want_ll) <= 1e-12 * abs(want_ll) + (1e-13 if abs(want_ll) < 1e-6 else 0.), col
            for r in range(len(self.parent)):
                tk = int(self.tokens[col, r])
                if tk == counts.GAP:
                    assert best[col, r] == -2 and np.all(np.isneginf(post[col, r])), (col, r)
                elif tk >= 0:
                    want_row = np.full(a, -np.inf)
                    want_row[tk] = 0.
                    assert best[col, r] == tk and np.array_equal(post[col, r], want_row), (col, r)
                else:
                    w = np.exp(lpp[r])
                    np.testing.assert_allclose(np.exp(post[col, r]), w, rtol=1e-8, atol=1e-300, err_msg="column %d node %d" % (col, r))
                    worst = max(worst, float(np.max(np.abs(np.exp(post[col, r]) - w) / w)))
                    assert np.all(post[col, r] <= 0.)
                    min_gap = min(min_gap, AR.top_two_gap(lpp[r]))
                    assert best[col, r] == AR.max_post_state(lpp[r]), (col, r)
                    cells += 1
        print("wildcard cells %d, smallest top-two gap of the oracle %.3g, worst relative deviation of a posterior %.3g" % (cells, min_gap, worst))
        # the oracle itself: no near tie among these cells, so `best` was compared without exceptions
        assert min_gap >= AR.NEAR_TIE
        return cells, worst


@functools.lru_cache(maxsize=None)
def case(name):
    if name.startswith("prot4"):
        with open(PROT4) as f:
            js = json.load(f)
        seed, leaves, n_cols = (9, 9, 300) if name == "prot4 9 leaves" else (11, 16, 333)
        rng = np.random.default_rng(seed)
        parent, length = _random_tree(rng, leaves)
        return Case(js, parent, length, _recon_columns(rng, parent, js["alphabet"], n_cols))
    if name == "cyclic acgt":
        rng = np.random.default_rng(4)
        parent, length = _random_tree(rng, 6)
        return Case(CYCLIC, parent, length, _recon_columns(rng, parent, "acgt", 700))
    alphabet = name
    rng = np.random.default_rng(len(alphabet))
    js = _random_model(rng, alphabet, True)
    parent, length = _random_tree(rng, 7)
    return Case(js, parent, length, _recon_columns(rng, parent, alphabet, 65), every=5)


def test_the_references_own_reconstruction():
    """PF16593.testspan.testnj.historian.fa: 85 nodes, 38 columns, one component of 20 residues, 1 400 '*' cells"""
    with open(G + "PF16593.testspan.testnj.nh") as f:
        rt = parse_newick(f.read())
    tree = so.Tree(rt.parent, rt.branch_length, rt.name)
    records = list(read_fasta(G + "PF16593.testspan.testnj.historian.fa"))
    assert len(records) == tree.nodes() == 85
    rows = []
    for n, (name, row) in enumerate(records):          # rows in tree-node order; an internal row's name is a Newick string
        assert name == tree.name[n] or (tree.child[n] and name.startswith("("))
        rows.append(row)
    omodel, model = ho.RateModel.from_file(G + "testamino.json"), hostmodel.RateModel.load(G + "testamino.json")
    sp = so.SumProduct(omodel, tree)
    want = AR.predict(omodel, tree, rows, min_prob=.01, sp=sp)
    assert len(want.lp) == sum(r.count("*") for r in rows) == 1400 and len(rows[0]) == 38
    print("oracle: smallest top-two gap %.3g, nearest posterior to log .01 at %.3g" % (want.min_gap(), want.threshold_margin(.01)))
    assert want.min_gap() >= AR.NEAR_TIE and want.threshold_margin(.01) >= 1e-6
    sub = [[sp.branch_sub[0][r]] if tree.parent[r] >= 0 else [np.zeros((20, 20))] for r in range(tree.nodes())]
    got_rows, got_pp = counts.predict_ancestors(model, tree.parent, tree.branch_length, rows, min_prob=.01, branch_sub=sub)
    assert got_rows == want.rows
    AR.compare_pp(want, got_pp, rtol=1e-8)


@pytest.mark.parametrize("name", ["prot4 9 leaves", "prot4 16 leaves"])
def test_seeded_reconstruction_columns_of_the_protein_mixture(name):
    c = case(name)
    assert c.sp.C == 4 and c.sp.A == 20
    cells, _ = c.check(c.predictor().run(c.tokens, want_post=True))
    assert cells > 1000
    assert capi.sumprod_kernel_ms() > 0


def test_seeded_columns_of_a_cyclic_dna_model_whole_and_in_chunks(monkeypatch):
    c = case("cyclic acgt")
    ap = c.predictor()
    whole = ap.run(c.tokens, want_post=True)
    cells, _ = c.check(whole)
    assert cells > 1000
    # the launcher's columns per chunk: the budget over the scratch of a column (3 C N A' + 3 C N doubles), in whole blocks
    # of 64 columns and at least one.  1 MB holds all 700 columns of this case (1 320 bytes each: 768 fit), so that run
    # is one chunk; a budget of 0 gives chunks of 64 columns: eleven, the last one partly filled.
    n_cols, n, a, cpts = c.tokens.shape[0], len(c.parent), 4, 1
    per_col = 8 * (3 * cpts * n * a + 3 * cpts * n)

    def chunk_of(mb):
        return min(n_cols, max(64, ((mb << 20) // per_col) & ~63))
    assert (n_cols, n, c.sp.C, c.sp.A) == (700, 11, cpts, a) and chunk_of(1) == 700 and chunk_of(0) == 64
    for mb in (1, 0):
        monkeypatch.setenv("HX_SUMPROD_SCRATCH_MB", str(mb))
        chunks = ap.run(c.tokens, want_post=True)
        for k in ("col_log_like", "best", "node_post"):
            assert whole[k].tobytes() == chunks[k].tobytes(), (mb, k)
    lean = ap.run(c.tokens)                                  # without node_post: the same picks
    assert lean["node_post"] is None and np.array_equal(lean["best"], whole["best"])


def test_a_tie_that_rounding_decides():
    """testcount.historian.fa under Jukes-Cantor: 12 '*' cells, one of them an exact tie in the oracle"""
    omodel, model, tree, gapped = _fixture("testcount.jukescantor.json", "testcount.historian.fa", "testcount.nh")
    rows = [gapped[n] for n in range(tree.nodes())]
    want = AR.predict(omodel, tree, rows)
    assert len(want.lp) == 12 and len(want.near_ties()) == 1 and want.min_gap() == 0.
    got_rows, _ = counts.predict_ancestors(model, tree.parent, tree.branch_length, rows)
    assert AR.compare_rows(want, got_rows, rows, omodel.alphabet, tie_rtol=1e-9) <= 1


@pytest.mark.parametrize("alphabet", ["acgtu", "abcdefghijklmnopqrstu", "ab"])
def test_alphabets_without_a_kernel_of_their_own(alphabet):
    c = case(alphabet)
    cells, _ = c.check(c.predictor().run(c.tokens, want_post=True))
    assert cells > 20


def _three_nodes():
    omodel, model = ho.RateModel.from_file(G + "testnj.jukescantor.json"), hostmodel.RateModel.load(G + "testnj.jukescantor.json")
    return omodel, model, counts.AncestorPredictor(model, [2, 2, -1], [.1, .2, 0.])


def test_edge_columns_on_a_three_node_tree():
    omodel, model, ap = _three_nodes()
    inf = -np.inf
    # one ungapped leaf: no wildcard; n_cols = 1
    got = ap.run(np.array([[3, -2, -2]], dtype=np.int8), want_post=True)
    assert got["best"].tolist() == [[3, -2, -2]]
    assert np.array_equal(got["node_post"][0], [[inf, inf, inf, 0.], [inf] * 4, [inf] * 4])
    assert abs(got["col_log_like"][0] - math.log(model.root[0][3])) <= 1e-12 * abs(math.log(model.root[0][3]))
    # an all-gap column beside others: what hx_sumprod_columns gives
    tok = np.array([[-2, -2, -2], [-1, -1, -1], [1, 2, -1]], dtype=np.int8)
    cc = counts.ColumnCounter(model, [2, 2, -1], [.1, .2, 0.])
    old = cc.run(tok)
    # (the same exp(R t) for both: the counter takes its own from the eigen decomposition)
    got = counts.AncestorPredictor(model, [2, 2, -1], [.1, .2, 0.], branch_sub=[[cc.branch_sub[0, r]] for r in range(3)]).run(tok, want_post=True)
    assert got["best"][0].tolist() == [-2, -2, -2] and np.all(np.isneginf(got["node_post"][0]))
    assert got["col_log_like"].tobytes() == old["col_log_like"].tobytes()
    # two 'x' leaves under a '*' root: the oracle's posterior at every node
    tree = so.Tree([2, 2, -1], [.1, .2, 0.], ["l", "r", "root"])
    sp = so.SumProduct(omodel, tree)
    sub = [[sp.branch_sub[0][r]] if r < 2 else [np.zeros((4, 4))] for r in range(3)]
    got = counts.AncestorPredictor(model, [2, 2, -1], [.1, .2, 0.], branch_sub=sub).run(tok, want_post=True)
    sp.init_column({0: "x", 1: "x", 2: "*"})
    sp.fill_up()
    sp.fill_down()
    for r in range(3):
        np.testing.assert_allclose(np.exp(got["node_post"][1, r]), np.exp(sp.log_node_post_prob(r)), rtol=1e-8)
    assert got["best"][1, 2] == AR.max_post_state(sp.log_node_post_prob(2))
    sp.init_column({0: "c", 1: "g", 2: "*"})
    sp.fill_up()
    sp.fill_down()
    np.testing.assert_allclose(np.exp(got["node_post"][2, 2]), np.exp(sp.log_node_post_prob(2)), rtol=1e-8)
    assert got["best"][2].tolist() == [1, 2, AR.max_post_state(sp.log_node_post_prob(2))]


def test_refused_arguments_and_a_model_without_an_eigen_basis():
    _, model, ap = _three_nodes()
    tok = np.zeros((4, 3), dtype=np.int8)
    ap.run(tok)                                                # (capi.sumprod_ancestors leaves the eigen pointers NULL)
    bad = counts.AncestorPredictor(model, [2, 2, -1], [.1, .2, 0.])
    bad.parent = np.array([-1, 0, 0], dtype=np.int32)          # a parent before its children
    with pytest.raises(capi.HxError) as e:
        bad.run(tok)
    assert e.value.code == -5
    bad_tok = tok.copy()
    bad_tok[2, 1] = 4                                          # not a token of a four-letter alphabet
    with pytest.raises(capi.HxError) as e:
        ap.run(bad_tok)
    assert e.value.code == -8
    three = counts.AncestorPredictor(model, [3, 3, 3, -1], [.1, .2, .3, 0.])
    with pytest.raises(capi.HxError) as e:
        three.run(np.zeros((4, 4), dtype=np.int8))
    assert e.value.code == -1


def test_agreement_with_the_column_counter_at_the_root_and_between_runs():
    c = case("prot4 9 leaves")
    ap = c.predictor()
    got = ap.run(c.tokens, want_post=True)
    again = ap.run(c.tokens, want_post=True)
    for k in ("col_log_like", "best", "node_post"):
        assert got[k].tobytes() == again[k].tobytes(), k          # no atomics: the same bits
    old = counts.ColumnCounter(c.model, c.parent, c.length, branch_sub=c.branch_sub).run(c.tokens, want_root_post=True)
    np.testing.assert_allclose(got["col_log_like"], old["col_log_like"], rtol=1e-12, atol=0)
    for col in range(c.tokens.shape[0]):
        present = [r for r in range(len(c.parent)) if c.tokens[col, r] != counts.GAP]
        root = max(present)                                    # (children before parents: the column's root is its last node)
        new_row, old_row = got["node_post"][col, root], old["root_post"][col]
        if c.tokens[col, root] == counts.WILD:
            np.testing.assert_allclose(new_row, old_row, rtol=1e-12, atol=0, err_msg="column %d" % col)
        else:
            # a residue at the root: exactly 0 / -inf here by definition; hx_sumprod_columns computes the 0 (rounding: ~1e-16)
            assert np.array_equal(np.isneginf(new_row), np.isneginf(old_row)) and abs(old_row[c.tokens[col, root]]) <= 1e-12


def test_ancestors_on_a_delayed_stream():
    # the smallest fixture: the reference's testaligncount alignment.  The call returns when its kernels are done, so
    # "still busy" is checked immediately before it.
    SH.one_hip_runtime()
    SH.cycles_per_ms()
    _, model, tree, gapped = _fixture("testnj.jukescantor.json", "testaligncount.fa", "testaligncount.nh")
    ap = counts.AncestorPredictor(model, tree.parent, tree.branch_length)
    tok = counts.tokenize_columns(model.alphabet, [gapped[n] for n in range(tree.nodes())])
    args = (ap.parent, ap.ins_prob, ap.log_cpt_weight, ap.branch_sub, tok)
    want = capi.sumprod_ancestors(*args, want_post=True)
    streams = SH.Streams()
    try:
        a = streams.new()
        streams.busy(a)
        SH.assert_busy(a, "sumprod_ancestors")
        got = capi.sumprod_ancestors(*args, want_post=True, stream=SH.handle(a))
    finally:
        streams.release()
    for w, g in zip(want, got):
        assert w.tobytes() == g.tobytes()
