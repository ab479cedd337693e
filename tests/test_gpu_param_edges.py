"""Every fill policy at the edges of the model's parameter space (the cases of tests/param_edge_cases.py; the yardstick
is pinned on them by tests/test_oracle_param_edges.py): zero and tiny rates, zero and saturated branches, extension
probabilities of 0 and nearly 1, in-cell spreads of hundreds of nats; identical, unrelated and low-complexity sequences.

Tolerances are those the suite already holds each policy to:
  exact   every cell, lpEnd and lpStart the table oracle's bits (tests/test_gpu_parity.py);
  fast    the -inf pattern of the exact fill, cells within 1e-7, lpEnd and lpStart within 1e-9 relative
          (test_fast_mode_stays_within_tolerance_of_exact);
  trunc / linear   the libm oracle with / without the reference's truncation: the same -inf pattern, cells within 1e-9,
          lpEnd (and lpStart) within 1e-12 relative; the untruncated lpStart within 1e-11 of lpEnd, the truncating one's
          within 1e-4; trunc also against the table oracle, cells 1e-6 and likelihoods 1e-9 (tests/test_gpu_linear_shapes.py,
          tests/test_gpu_trunc.py).
A zero likelihood is -inf, never NaN, in lpEnd and lpStart, and has no best path.  The best path of every other pair is the
path through the table oracle's matrix under exact, fast and trunc; under linear a path may differ only where the device
itself reports a near-tie.

One case, `beyond`, spreads the states of a cell over more than fp64's range (1305 nats; the range is 708).  The scaled
policies keep a cell under one exponent, so there - and only there - the narrowed contract of include/historian_hip.h
applies: a state more than D nats below the largest state of its own cell may come out as -inf or with reduced precision,
every other value and both likelihoods meet the full contract (D and its derivation: tests/param_edge_cases.py).

What the cases reach that the benign models of the other files do not:
  t0, indel0, ins0   cells (or two state planes) of probability zero in the interior of the pipeline: the exponent of an
                     all-zero cell at renormalisation, -inf through every table log-sum-exp, from_logs of an all -inf cell
                     on the wrap-around link (HX_LINEAR_WAVES=1) and between workgroups (HX_CHAIN_MULTI=2), lpEnd = -inf
  tiny_indel         terms 27 nats apart: the truncating sum drops nearly every second term
  tiny_t, saturated  emissions of 1e-10 (a mantissa loses 60 decimal digits between two renormalisations), gap probabilities near 1
  ext0, ext_near_1   -inf and nearly-zero extension transitions; lpEnd near -690
  wide               518 nats inside one cell: shifts of 750 bits, exp(-518) on the wrap-around link
  same, homo, rep    ties and near-ties between best paths"""
import pytest

from historian_amd import capi
from tests import helpers as H
from tests import param_edge_cases as P

pytestmark = pytest.mark.gpu

POLICY = {"exact": (capi.HX_LSE_EXACT, 0), "fast": (capi.HX_LSE_FAST, 0), "trunc": (capi.HX_LSE_TRUNC, 2), "linear": (capi.HX_LSE_LINEAR, 1)}


@pytest.fixture(scope="module", autouse=True)
def engine():
    capi.init(0, P.c_oracle.table())      # host-libm table
    yield
    capi.shutdown()


def images(cases):
    return [c["img"] for c in cases]


def run(cases, flags, backward=True):
    b = capi.Batch(images(cases), flags | (capi.HX_KEEP_BACKWARD if backward else 0))
    b.forward()
    if backward:
        b.backward()
    return b


def check_scaled(b, cases, policy, backward=True, inside_only=False):
    """a trunc / linear batch against its yardsticks; -> {case name: (deviating states, smallest depth among them)} of the
    cases under the narrowed contract"""
    tm = POLICY[policy][1]
    lp_end = b.lp_end()
    lp_start = b.lp_start() if backward else None
    worst = {"cells": 0., "table": 0.}
    narrowed = {}
    for k, c in enumerate(cases):
        sel = H.envelope_mask(c["f"]) if inside_only else None
        for which in ((0, 1) if backward else (0,)):
            what = "%s, %s (%s)" % (c["name"], policy, "FB"[which])
            got = b.read_matrix(k, which)
            yards = [(P.oracle(c, which, tm)["cells"], 1e-9, "cells")] + ([(P.oracle(c, which)["cells"], 1e-6, "table")] if policy == "trunc" else [])
            for want, tol, key in yards:
                if c["model"] == "beyond":
                    n, d = P.assert_cells_close_within_depth(got, want, tol, P.full_precision_depth(c["f"].hmm), what, sel)
                    if key == "cells":
                        narrowed[what] = (n, d)
                else:
                    worst[key] = max(worst[key], P.assert_cells_close(got, want, tol, what, sel))
        what = "%s, %s" % (c["name"], policy)
        P.assert_lp_close(lp_end[k], P.oracle(c, 0, tm)["lp_end"], 1e-12, what + ": lpEnd")
        if policy == "trunc":
            P.assert_lp_close(lp_end[k], P.oracle(c, 0)["lp_end"], 1e-9, what + ": lpEnd vs the table arithmetic")
        if backward:
            P.assert_lp_close(lp_start[k], P.oracle(c, 1, tm)["lp_start"], 1e-12, what + ": lpStart")
            if policy == "trunc":
                P.assert_lp_close(lp_start[k], P.oracle(c, 1)["lp_start"], 1e-9, what + ": lpStart vs the table arithmetic")
            P.assert_lp_close(lp_start[k], lp_end[k], 1e-11 if policy == "linear" else 1e-4, what + ": lpStart vs lpEnd")
    print("%s: worst cell error %.3g (bound 1e-9)%s; narrowed contract: %s" % (
        policy, worst["cells"], ", vs the table arithmetic %.3g (bound 1e-6)" % worst["table"] if policy == "trunc" else "", narrowed))
    return narrowed


def check_paths(b, cases, policy):
    """the best path of every pair with a likelihood, none (n_cells = -1) for the others"""
    want = [P.reference_path(c) for c in cases]
    _, n_cells = b.best_trace(raw=True)
    got = b.best_trace()
    ties = b.best_trace_ties()
    differ = []
    for k, c in enumerate(cases):
        if want[k] is None:
            assert n_cells[k] == -1 and got[k] is None, "%s, %s: a best path without a likelihood" % (c["name"], policy)
        elif got[k] != want[k]:
            differ.append(c["name"])
            assert policy == "linear", "%s, %s: best path differs from the reference's" % (c["name"], policy)
            assert ties[k] == 1, "%s, linear: best path differs without a reported near-tie" % c["name"]
    print("%s: %d of %d best paths differ %s" % (policy, len(differ), len(cases), differ))


# ---------------------------------------------------------------------------------------------------------------------------
# leaf pairs, one batch per policy
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("generic", [False, True])
def test_exact_policy_is_the_table_oracle_bit_for_bit(generic):
    # (HX_FORCE_GENERIC takes the leaf pairs through the first general kernels of hx_dag.hip)
    cases = P.leaf_cases()
    b = run(cases, capi.HX_LSE_EXACT | (capi.HX_FORCE_GENERIC if generic else 0))
    assert all(b.job_kernel(k)[0] == (9 if generic else 0) for k in range(len(cases)))
    lp_end, lp_start = b.lp_end(), b.lp_start()
    for k, c in enumerate(cases):
        wf, wb = P.oracle(c, 0), P.oracle(c, 1)
        H.assert_same_bits(b.read_matrix(k, 0), wf["cells"], c["name"] + " Forward cells")
        H.assert_same_bits(b.read_matrix(k, 1), wb["cells"], c["name"] + " Backward cells")
        H.assert_same_bits([lp_end[k], lp_start[k]], [wf["lp_end"], wb["lp_start"]], c["name"] + " lpEnd, lpStart")
    check_paths(b, cases, "exact")
    b.close()


def test_fast_policy_stays_within_its_tolerance():
    cases = P.leaf_cases()
    b = run(cases, capi.HX_LSE_FAST)
    assert all(b.job_kernel(k)[0] == 0 for k in range(len(cases)))
    lp_end, lp_start = b.lp_end(), b.lp_start()
    worst = 0.
    for k, c in enumerate(cases):
        for which in (0, 1):
            worst = max(worst, P.assert_cells_close(b.read_matrix(k, which), P.oracle(c, which)["cells"], 1e-7,
                                                    "%s, fast (%s)" % (c["name"], "FB"[which])))
        P.assert_lp_close(lp_end[k], P.oracle(c, 0)["lp_end"], 1e-9, c["name"] + ", fast: lpEnd")
        P.assert_lp_close(lp_start[k], P.oracle(c, 1)["lp_start"], 1e-9, c["name"] + ", fast: lpStart")
    print("fast: worst cell error %.3g (bound 1e-7)" % worst)
    check_paths(b, cases, "fast")
    b.close()


@pytest.mark.parametrize("launch", ["default", "HX_CHAIN_MULTI=0", "HX_LINEAR_WAVES=1"])
@pytest.mark.parametrize("policy", ["trunc", "linear"])
def test_scaled_policies_on_unbanded_leaf_pairs(policy, launch, monkeypatch):
    # HX_LINEAR_WAVES=1: one wave per pair, so that every strip boundary is the wrap-around link and the row above comes
    # back from its stored logarithms (from_logs) - whole-zero cells, zero planes and 500-nat spreads included
    if launch != "default":
        monkeypatch.setenv("HX_CHAIN_MULTI", "0")
    if launch == "HX_LINEAR_WAVES=1":
        monkeypatch.setenv("HX_LINEAR_WAVES", "1")
    cases = P.leaf_cases()
    b = run(cases, POLICY[policy][0])
    assert all(b.job_kernel(k)[0] == 0 for k in range(len(cases)))
    narrowed = check_scaled(b, cases, policy)
    assert len(narrowed) == 2 * sum(c["model"] == "beyond" for c in cases)
    check_paths(b, cases, policy)
    b.close()


@pytest.mark.parametrize("groups", ["2", "0"])
@pytest.mark.parametrize("policy", ["trunc", "linear"])
def test_long_pairs_and_rows_handed_between_workgroups_as_logarithms(policy, groups, monkeypatch):
    # two workgroups per pair: the wrap-around link crosses workgroups (k_fill_leaf_linear MULTI); 0: the ordinary launch
    monkeypatch.setenv("HX_CHAIN_MULTI", groups)
    cases = P.multi_cases()
    b = run(cases, POLICY[policy][0])
    assert all(b.job_kernel(k)[0] == 0 for k in range(len(cases)))
    check_scaled(b, cases, policy)
    assert b.relaunches() == 0
    check_paths(b, cases, policy)
    b.close()


# ---------------------------------------------------------------------------------------------------------------------------
# banded leaf pairs
# ---------------------------------------------------------------------------------------------------------------------------
def admitted_to_shared_wavefronts(cases, monkeypatch):
    monkeypatch.setenv("HX_BAND2", "1")
    out = []
    for c in cases:
        b = capi.Batch([c["img"]], capi.HX_LSE_TRUNC)
        if b.shared_wavefront_pairs() == 1:
            out.append(c)
        b.close()
    monkeypatch.delenv("HX_BAND2")
    return out


@pytest.mark.parametrize("policy", ["exact", "fast"])
def test_table_policies_on_banded_leaf_pairs(policy):
    cases = P.banded_cases()
    b = run(cases, POLICY[policy][0])
    assert all(b.job_kernel(k)[0] in (1, 2) for k in range(len(cases)))
    lp_end, lp_start = b.lp_end(), b.lp_start()
    for k, c in enumerate(cases):
        for which in (0, 1):
            what = "%s, %s (%s)" % (c["name"], policy, "FB"[which])
            if policy == "exact":
                H.assert_same_bits(b.read_matrix(k, which), P.oracle(c, which)["cells"], what)
            else:
                P.assert_cells_close(b.read_matrix(k, which), P.oracle(c, which)["cells"], 1e-7, what)
        P.assert_lp_close(lp_end[k], P.oracle(c, 0)["lp_end"], 0. if policy == "exact" else 1e-9, c["name"] + ": lpEnd")
        P.assert_lp_close(lp_start[k], P.oracle(c, 1)["lp_start"], 0. if policy == "exact" else 1e-9, c["name"] + ": lpStart")
    check_paths(b, cases, policy)
    b.close()


@pytest.mark.parametrize("hook", ["default", "HX_BAND2=0", "HX_BAND2=1", "HX_BAND_PPW=-3"])
@pytest.mark.parametrize("policy", ["trunc", "linear"])
def test_scaled_policies_on_banded_leaf_pairs(policy, hook, monkeypatch):
    # the rotating-row sweep (hx_band.hip), two pairs per wavefront (hx_band2.hip), the lean kernel (HX_BAND_PPW=-3); row 0
    # beyond the sweep's reach is the prefix sum of hx_bandedge.h.  Dense planes, then band-compressed ones (Forward only,
    # compared inside the envelope: a cell that is not stored reads as -inf)
    cases = P.banded_cases()
    if hook == "HX_BAND2=1":
        cases = admitted_to_shared_wavefronts(cases, monkeypatch)
        assert {c["model"] for c in cases} >= {"t0_one_side", "tiny_indel", "ext0", "wide", "beyond"}, [c["name"] for c in cases]
    if hook != "default":
        monkeypatch.setenv(*hook.split("="))
    for storage in (0, capi.HX_BAND_COMPRESSED):
        b = run(cases, POLICY[policy][0] | storage, backward=not storage)
        assert all(b.job_kernel(k)[0] in (1, 2) for k in range(len(cases)))
        assert any(b.job_kernel(k)[0] == 2 for k in range(len(cases)))
        assert b.shared_wavefront_pairs() == (len(cases) if hook == "HX_BAND2=1" else 0)
        check_scaled(b, cases, policy, backward=not storage, inside_only=bool(storage))
        check_paths(b, cases, policy)
        b.close()


# ---------------------------------------------------------------------------------------------------------------------------
# profile pairs (state DAGs)
# ---------------------------------------------------------------------------------------------------------------------------
def test_general_profiles_under_every_policy():
    cases = P.dag_cases()
    assert max(c["f"].x_size for c in cases) > 65         # more than one strip of 64 rows
    be = run(cases, capi.HX_LSE_EXACT)
    assert all(be.job_kernel(k)[0] == 7 for k in range(len(cases)))
    for k, c in enumerate(cases):
        wf, wb = P.oracle(c, 0), P.oracle(c, 1)
        H.assert_same_bits(be.read_matrix(k, 0), wf["cells"], c["name"] + " Forward cells")
        H.assert_same_bits(be.read_matrix(k, 1), wb["cells"], c["name"] + " Backward cells")
        H.assert_same_bits([be.lp_end()[k], be.lp_start()[k]], [wf["lp_end"], wb["lp_start"]], c["name"] + " lpEnd, lpStart")
    check_paths(be, cases, "exact")
    be.close()
    bf = run(cases, capi.HX_LSE_FAST)
    for k, c in enumerate(cases):
        for which in (0, 1):
            P.assert_cells_close(bf.read_matrix(k, which), P.oracle(c, which)["cells"], 1e-7, "%s, fast (%s)" % (c["name"], "FB"[which]))
        P.assert_lp_close(bf.lp_end()[k], P.oracle(c, 0)["lp_end"], 1e-9, c["name"] + ", fast: lpEnd")
        P.assert_lp_close(bf.lp_start()[k], P.oracle(c, 1)["lp_start"], 1e-9, c["name"] + ", fast: lpStart")
    check_paths(bf, cases, "fast")
    # no truncating kernel for state DAGs: HX_LSE_TRUNC takes the fast table policy there, bit for bit
    bt = run(cases, capi.HX_LSE_TRUNC)
    for k, c in enumerate(cases):
        for which in (0, 1):
            H.assert_same_bits(bt.read_matrix(k, which), bf.read_matrix(k, which), c["name"] + " under HX_LSE_TRUNC")
    H.assert_same_bits(bt.lp_end(), bf.lp_end(), "lpEnd under HX_LSE_TRUNC")
    H.assert_same_bits(bt.lp_start(), bf.lp_start(), "lpStart under HX_LSE_TRUNC")
    bt.close()
    # HX_LSE_LINEAR: the scaled-probability Forward fill of hx_daglin.hip (the libm oracle: pattern, 1e-9, lpEnd 1e-12, and
    # 1e-5 of the table arithmetic); its Backward fill is the fast policy's, bit for bit
    bl = run(cases, capi.HX_LSE_LINEAR)
    for k, c in enumerate(cases):
        want = P.oracle(c, 0, 1)
        P.assert_cells_close(bl.read_matrix(k, 0), want["cells"], 1e-9, c["name"] + ", linear")
        P.assert_lp_close(bl.lp_end()[k], want["lp_end"], 1e-12, c["name"] + ", linear: lpEnd")
        P.assert_lp_close(bl.lp_end()[k], P.oracle(c, 0)["lp_end"], 1e-5, c["name"] + ", linear: lpEnd vs the table arithmetic")
        H.assert_same_bits(bl.read_matrix(k, 1), bf.read_matrix(k, 1), c["name"] + " Backward cells, linear-mode batch vs fast batch")
    H.assert_same_bits(bl.lp_start(), bf.lp_start(), "lpStart, linear-mode batch vs fast batch")
    bl.close()
    bf.close()
