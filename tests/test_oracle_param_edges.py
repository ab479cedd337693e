"""The yardstick of tests/test_gpu_param_edges.py, pinned before the kernels are held to it: the C oracle's three
arithmetics (the reference's table, libm, libm with the reference's truncation) on the extreme models and sequences of
tests/param_edge_cases.py - leaf pairs, banded leaf pairs and profile pairs, Forward and Backward.

Bounds: table against truncated libm as tests/test_gpu_trunc.py holds the device to (cells 1e-6, likelihoods 1e-9 relative;
measured worst on these cases 3.3e-8 and 1.1e-10), lpStart against lpEnd 1e-4 relative in the truncated arithmetic (measured
worst 1.7e-5, on `beyond`).  Structure that needs no second implementation: where a model leaves only the diagonal, only the
diagonal is finite; the closed form of the likelihood of an ungapped alignment."""
import math

import numpy as np
import pytest

from oracle import c_oracle
from tests import param_edge_cases as P

ALL = P.case_names("leaf", "multi", "banded", "dag")
LEAF = P.case_names("leaf", "multi")


def by_name(names):
    """one test per case; the case is built (once per process) when its first test runs"""
    return pytest.mark.parametrize("case", names, indirect=True)


@pytest.fixture
def case(request):
    return P.case(request.param)


@by_name(ALL)
def test_three_arithmetics_agree(case):
    for which in (0, 1):
        what = "%s (%s)" % (case["name"], "FB"[which])
        table, libm, trunc = (P.oracle(case, which, tm) for tm in (0, 1, 2))
        for r in (table, libm, trunc):
            assert not np.isnan(r["cells"]).any(), what
            assert not np.isnan(P.lp_of(r, which)), what
        assert np.array_equal(np.isneginf(table["cells"]), np.isneginf(libm["cells"])), what
        assert np.array_equal(np.isneginf(table["cells"]), np.isneginf(trunc["cells"])), what
        P.assert_cells_close(trunc["cells"], table["cells"], 1e-6, what)
        P.assert_lp_close(P.lp_of(trunc, which), P.lp_of(table, which), 1e-9, what)
        P.assert_lp_close(P.lp_of(libm, which), P.lp_of(table, which), 1e-4, what)       # (north_star's bound: no truncation here)
    lp_end, lp_start = P.oracle(case, 0, 2)["lp_end"], P.oracle(case, 1, 2)["lp_start"]
    P.assert_lp_close(lp_start, lp_end, 1e-4, case["name"] + ": lpStart vs lpEnd")


@by_name(ALL)
def test_in_cell_spread_stays_on_its_side_of_the_fp64_range(case):
    # the scaled-probability fills keep a cell under one exponent: `beyond` alone may leave fp64's range (e^-708), and must
    spread = max(P.in_cell_spread(P.oracle(case, which)["cells"]).max() for which in (0, 1))
    if case["model"] == "beyond":
        assert spread > 800, spread
    else:
        assert spread < 600, spread


@by_name([n for n in LEAF if P.model_of_case(n) in ("t0", "indel0")])
def test_only_the_diagonal_is_finite_without_indels(case):
    sx, sy = case["sx"], case["sy"]
    # Forward: every state, on the diagonal from the start.  Backward: the match state (a gap state, which no path enters, may
    # still be left by extension), on the diagonal into the end
    i, j, _ = np.nonzero(np.isfinite(P.oracle(case, 0)["cells"]))
    assert len(i) and np.all(i == j), case["name"]
    i, j = np.nonzero(np.isfinite(P.oracle(case, 1)["cells"][:, :, 0]))
    assert len(i) and np.all(len(sx) - i == len(sy) - j), case["name"]
    assert np.isfinite(P.oracle(case, 0)["cells"][0, 0, 0])
    possible = len(sx) == len(sy) and (case["model"] != "t0" or sx == sy)
    assert np.isfinite(P.oracle(case, 0)["lp_end"]) == possible, case["name"]
    assert np.isfinite(P.oracle(case, 1)["lp_start"]) == possible, case["name"]


@by_name([n for n in ALL if P.model_of_case(n) == "ins0"])
def test_no_insertion_state_is_ever_entered_at_rate_zero(case):
    cells = P.oracle(case, 0)["cells"]
    assert np.all(np.isneginf(cells[:, :, 3])) and np.all(np.isneginf(cells[:, :, 4])), case["name"]      # IMI, IIW
    assert np.isfinite(cells[:, :, :3]).any()


def test_ungapped_likelihood_in_closed_form():
    # indel0, y = x, 64 residues: the only path is 64 matches - the start cell (log 1), 64 match-to-match transitions, the
    # end transition, and the 64 emissions sum over a of root(a) P_l(a -> x) P_r(a -> x)
    case = P.leaf_case("indel0", "same", 64, 64)
    hmm, sx = case["f"].hmm, case["sx"]
    T = hmm.trans_matrix()
    tok = [hmm.l.alphabet.index(ch) for ch in sx]
    # the emissions as every arithmetic of the oracle forms them (the reference's table operator over the prepared vectors,
    # src/forward.h:112-124; the arithmetics differ in the cell recursion alone): the sum itself is then exact
    lse = c_oracle.load().orc_log_sum_exp
    fwd = P.oracle(case, 0)
    log_root = np.array(hmm.log_root).reshape(-1)
    emit = []
    for k in range(1, 65):
        lp = P.NEG_INF
        for a in range(len(log_root)):
            lp = lse(lp, float(log_root[a]) + (float(fwd["subx"][k][a]) + float(fwd["suby"][k][a])))
        emit.append(lp)
    want = math.fsum([T[0][0]] * 64 + [T[0][5]] + emit)
    for tm in (0, 1, 2):
        assert abs(P.oracle(case, 0, tm)["lp_end"] - want) <= 1e-12 * abs(want), tm
        assert abs(P.oracle(case, 1, tm)["lp_start"] - want) <= 1e-12 * abs(want), tm
    # ... and against the emissions in plain arithmetic: the table interpolates, < 3e-10 per operation, four operations per
    # emission (measured over the 64: 1.8e-9)
    root = np.exp(log_root)
    sl, sr = np.array(hmm.l.sub_mat)[0], np.array(hmm.r.sub_mat)[0]
    plain = math.fsum([T[0][0]] * 64 + [T[0][5]] + [math.log(math.fsum(root[a] * sl[a][k] * sr[a][k] for a in range(4))) for k in tok])
    assert abs(want - plain) <= 64 * 4 * 3e-10


def test_the_full_precision_depth_follows_from_the_model():
    # D of tests/param_edge_cases.py: every case but `beyond` stays inside it, `beyond` leaves it
    for case in map(P.case, ALL):
        if case["kind"] == "dag" or min(P.per_step_floor(case["f"].hmm)) == 0.:
            continue            # (derived for leaf fills under models in which every state can move in every direction)
        depth = P.full_precision_depth(case["f"].hmm)
        spread = max(P.in_cell_spread(P.oracle(case, which)["cells"]).max() for which in (0, 1))
        assert depth < 1001 * P.LN2
        assert (spread > depth) == (case["model"] == "beyond"), (case["name"], spread, depth)
