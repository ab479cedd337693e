"""The yardstick on the envelopes real guide alignments produce (tests/band_geometry_cases.py): the guides are alignments,
the likelihoods finite, the row spans as irregular as the family's name says, and oracle_fill.c the Python oracle's bits."""
import numpy as np
import pytest

from oracle import c_oracle
from oracle import historian_oracle as ho
from tests import band_geometry_cases as G
from tests import helpers as H


@pytest.mark.parametrize("name", list(G.FAMILIES))
def test_family_is_a_valid_irregular_envelope_with_finite_likelihoods(name):
    f, (x, y, hmm, md) = G.leaf(name)
    lx, events, band, _ = G.FAMILIES[name]
    assert H.valid_guide(f.guide, f.seqs)
    assert len(f.seqs[1]) == lx and x.n_states - 1 <= 330 and y.n_states - 1 <= 330
    assert x.n_states - 1 > 64
    assert md == band
    wf, wb = c_oracle.forward(x, y, hmm, md), c_oracle.backward(x, y, hmm, md)
    assert np.isfinite(wf["lp_end"]) and np.isfinite(wb["lp_start"])
    assert abs(wf["lp_end"] - wb["lp_start"]) < .01 * abs(wf["lp_end"])       # (the reference's own FWD_BACK_ERROR_TOLERANCE)
    # every in-envelope cell of the mask is where the fill put a cell: (0, 0) holds 0, the rest of the oracle's -inf
    # pattern lies inside the mask
    assert not np.isfinite(wf["cells"][~G.mask(name)]).any()
    # irregular: a row far wider than the band's diagonal width, or at least 64 rows sharing one span
    bm = G.band_mask(f)
    spans = [(int(np.argmax(r)), int(r.sum())) for r in bm]
    assert all(n >= 1 for _, n in spans)
    widest = max(n for _, n in spans)
    shared = max(spans.count(s) for s in set(spans))
    assert widest >= 3 * (2 * band + 1) or shared >= 64, (widest, shared)
    if name in G.WHOLE:
        assert G.mask(name).all()
        job = (x, y, hmm, -1)
        H.assert_same_bits(wf["cells"], c_oracle.forward(*job)["cells"], "banded vs unbanded Forward cells")
        H.assert_same_bits(wb["cells"], c_oracle.backward(*job)["cells"], "banded vs unbanded Backward cells")
    else:
        assert not G.mask(name).all()


def test_the_issue_table_figures():
    # lpEnd of the six families first tabulated (seed 7, Jukes-Cantor), and the shapes
    want = {"long_y_run": ((151, 241), -472.248), "long_x_run": ((201, 101), -389.580), "staircase": ((261, 291), -748.529),
            "leading_y_run": ((141, 221), -440.309), "band0_runs": ((131, 126), -308.402), "no_match": ((71, 62), -200.867)}
    for name, (shape, lp) in want.items():
        f, (x, y, hmm, md) = G.leaf(name)
        assert G.mask(name).shape == shape
        assert "%.3f" % c_oracle.forward(x, y, hmm, md)["lp_end"] == "%.3f" % lp


@pytest.mark.parametrize("name", G.SMALL)
def test_c_oracle_matches_the_python_oracle_bit_for_bit(name):
    lx, events, band, kw = G.FAMILIES[name]
    f = H.guided_leaf_case(G.SEED, lx, events, band, **kw)      # (a matrix of its own: filling modifies it)
    x, y, hmm, md = H.job_images(f)
    f.fill()
    wf = c_oracle.forward(x, y, hmm, md)
    H.assert_same_bits(wf["cells"], H.oracle_dense(f), "Forward cells")
    H.assert_same_bits([wf["lp_end"]], [f.lp_end], "lpEnd")
    b = ho.BackwardMatrix(f)
    wb = c_oracle.backward(x, y, hmm, md)
    H.assert_same_bits(wb["cells"], H.oracle_dense(b), "Backward cells")
    H.assert_same_bits([wb["lp_start"]], [b.lp_start()], "lpStart")


@pytest.mark.parametrize("name,band,samples,keep_all", [("dag_one_strip", 0, 0, False), ("dag_one_strip", 2, 4, False),
                                                        ("dag_one_strip", 6, 0, True), ("dag_three_strips", 6, 4, False),
                                                        ("dag_three_strips", 2, 0, False), ("dag_three_strips", 0, 0, True)])
def test_profile_pairs_over_a_four_leaf_history(name, band, samples, keep_all):
    f, (x, y, hmm, md) = G.dag(name, band, samples, keep_all)
    assert H.valid_guide(f.guide, f.seqs)
    strips = (x.n_states - 1 + 63) // 64
    assert strips == 1 if name == "dag_one_strip" else strips >= 3, x.n_states
    wf, wb = c_oracle.forward(x, y, hmm, md), c_oracle.backward(x, y, hmm, md)
    assert np.isfinite(wf["lp_end"]) and np.isfinite(wb["lp_start"])
    assert not np.isnan(wf["cells"]).any() and not np.isnan(wb["cells"]).any()
    env = H.envelope_mask(f)
    assert not env.all() and not np.isfinite(wf["cells"][~env]).any()
    if name == "dag_one_strip":
        g = H.guided_dag_case(G.SEED, *G.DAG_FAMILIES[name], band, samples, keep_all=keep_all)
        g.fill()
        H.assert_same_bits(wf["cells"], H.oracle_dense(g), "Forward cells")
        H.assert_same_bits(wb["cells"], H.oracle_dense(ho.BackwardMatrix(g)), "Backward cells")
