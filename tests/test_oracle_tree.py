"""The restatement of the reference's tree estimation (tests/tree_ref.py) against what the reference holds: its four Newick
fixtures (`testnj`, `testupgma`; reference Makefile:270-276), byte for byte, and hand-worked edge cases of
DistanceMatrixParams::tML's control flow (reference src/model.cpp:584-655)."""
import math
import os

import numpy as np
import pytest

from oracle import historian_oracle as ho
from tests import tree_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden", "reference_data") + os.sep
FAMILIES = {"testnj": ("testnj.jukescantor.json", "testnj.fa", "testnj.out.nh", "testupgma.out.nh"),
            "PF16593": ("testamino.json", "PF16593.testspan.fa", "PF16593.testspan.testnj.nh", "PF16593.testspan.testupgma.nh")}


@pytest.fixture(scope="module")
def jc():
    return ho.RateModel.from_file(G + "testnj.jukescantor.json")


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_tree_ref_prints_the_references_trees(family):
    model_file, fasta, nj, upgma = FAMILIES[family]
    model, names, rows, esr, dist, infos = T.family(model_file, fasta)
    assert T.to_newick(T.neighbor_joining(names, dist)) + "\n" == open(G + nj).read()
    assert T.to_newick(T.upgma(names, dist)) + "\n" == open(G + upgma).read()
    # the node numbering of the reference's parse(toString()): post-order, root last, leaves as named
    text, tree = T.build_tree(model, names, rows, distance=dist)
    assert text + "\n" == open(G + nj).read()
    assert tree.nodes() == 2 * len(names) - 1 and sorted(tree.name[n] for n in range(tree.nodes()) if tree.is_leaf(n)) == sorted(names)
    assert all(tree.branch_length[n] >= T.MIN_BRANCH_LENGTH for n in range(tree.nodes() - 1))


def test_the_recorded_distances_are_what_tree_ref_computes():
    # tests/golden/tree_ref/PF16593.testspan.distances.json spares the GPU tests twenty seconds; it holds nothing else
    model_file, fasta = FAMILIES["PF16593"][:2]
    _, _, _, esr, dist, infos = T.family(model_file, fasta)
    _, _, _, r_esr, r_dist, r_infos = T.recorded_family(model_file, fasta)
    assert esr.hex() == r_esr.hex()
    assert [[v.hex() for v in row] for row in dist] == [[v.hex() for v in row] for row in r_dist]
    assert infos == r_infos
    flagged = [ij for ij, info in infos.items() if info["min_gap"] < 1e-9]
    assert len(flagged) == 4 and len(infos) == 903          # with the restated series, as with scipy's expm: 4 near ties


@pytest.mark.parametrize("t", [1e-9, 5e-4, .003, .05, .5, 3., 20., 90.])
def test_the_vectorised_series_has_the_bits_of_the_oracles(t):
    for name in ("testamino.json", "testnj.jukescantor.json"):
        model = ho.RateModel.from_file(G + name)
        for sr in model.sub_rate:
            want = np.array(ho.sub_prob_matrix_ss(np.asarray(sr).tolist(), t))
            assert np.array_equal(want.view(np.int64), T._sub_prob(sr, t).view(np.int64))


def test_a_pair_without_a_counted_column(jc):
    # tJC = 0/0 = NaN; std::max(tMin, NaN) = tMin, so tjc = 1e-9, the bracket is [5e-10, 10]; f = 0 everywhere, nothing is
    # ever strictly below both ends, the scan runs dry and `llLower < llUpper` is false: tUpper
    info = {}
    assert T.ml_distance(jc, "AC--", "--GT", info=info) == 10.
    assert (info["t_lower"], info["t_upper"]) == (5e-10, 10.)
    assert T.ml_distance(jc, "*CNx", "A*GT", info=info) == 10.      # a wildcard or a character outside the alphabet in every column
    assert T.ml_distance(jc, "ACGT", "....", max_iterations=0) == 1e-9                                       # ... and the clamped tJC


def test_a_saturated_pair_searches_up_to_twenty(jc):
    # pDiff = 3/4 >= (A - 1) / A: tJC = inf, clamped to 10; tLower = min(1e-9, 5) = 1e-9, tUpper = max(10, 20) = 20
    info = {}
    t = T.ml_distance(jc, "AAAACCCC", "CGTAAGTC", info=info)      # 6 of 8 differ
    assert (info["t_lower"], info["t_upper"]) == (1e-9, 20.)
    assert 1e-9 <= t <= 20.
    assert T.ml_distance(jc, "AAAACCCC", "CGTAAGTC", max_iterations=0) == 10.


def test_no_iterations_give_the_clamped_jukes_cantor_distance(jc):
    esr = T.expected_sub_rate(jc)
    x, y = "ACGTACGTAC", "ACGTACGTCA"                            # 2 of 10 differ
    want = -(3 / 4) * math.log(1 - (4 / 3) * (2 / 10)) / esr
    assert T.ml_distance(jc, x, y, max_iterations=0) == want
    assert T.ml_distance(jc, x, y, max_iterations=-5) == want
    assert T.ml_distance(jc, x, x, max_iterations=0) == 1e-9     # pDiff = 0: tJC = -0.0, raised to tMin
    # three iterations exhaust the loop: the three bracket evaluations and one per iteration, no more
    info = {}
    t3 = T.ml_distance(jc, x, y, max_iterations=3, info=info)
    assert info["evaluations"] == 6 and 1e-9 <= t3 <= 10.


def test_identical_sequences(jc):
    # tjc = 1e-9, bracket [5e-10, 10]; f rises with t, so no point is below f(tLower): every scan fails, llLower < llUpper
    # halves the window from above until it is no wider than tLower, and tLower comes back
    info = {}
    assert T.ml_distance(jc, "ACGTACGT", "ACGTACGT", info=info) == 5e-10
    assert info["evaluations"] >= 3 + 4 * 35                     # 35 halvings of [5e-10, 10] until the width is <= 5e-10


def test_two_sequences_make_only_the_root(jc):
    d = T.ml_distance(jc, "ACGTACGTAC", "ACGTACGTCA")
    dist = [[0., d], [d, 0.]]
    want = "(a:%g,b:%g);" % (d / 2, d / 2)
    assert T.to_newick(T.neighbor_joining(["a", "b"], dist)) == want
    assert T.to_newick(T.upgma(["a", "b"], dist)) == want
    tree = T.parse_tree(want)
    assert tree.parent == [2, 2, -1] and tree.name[:2] == ["a", "b"]


def test_hostmodel_expected_sub_rate_is_tree_refs():
    from historian_amd import hostmodel
    for path in (G + "testamino.json", G + "testnj.jukescantor.json", os.path.join(ROOT, "tests", "golden", "models", "prot4.json")):
        want = T.expected_sub_rate(ho.RateModel.from_file(path))
        assert abs(hostmodel.expected_sub_rate(hostmodel.RateModel.load(path)) - want) <= 1e-14 * want
