"""Indel counts carried through profiles (tests/indel_carry_ref.py: makeProfile under CountIndelEvents, the carried terms of
transitionEigenCounts and getCounts) against exhaustive enumeration of whole histories.

Each child profile is built KeepAll from every cell of its lattice with a finite posterior, so each of its transitions is one
lower-level cell transition and carries exactly that transition's events: a root path then fixes the whole history, and the
expectation over root paths of the events along the path plus the carried counts is the exact expectation over histories.
The fills use libm log-sum-exps here (indel_carry_ref.exact_log_sum_exp), so the comparison holds to rounding."""
import pytest

from oracle import counts_dp_oracle as cd
from oracle import historian_oracle as ho
from tests import indel_carry_ref as R

M = "tests/golden/models/"
KEEP_ALL = ho.DPMatrix.CountIndelEvents
COLLAPSE = ho.DPMatrix.CountIndelEvents | ho.DPMatrix.CollapseChains
TIMES = (.1, .2, .15, .3)


def _close(a, b, tol=1e-12):
    return abs(a - b) <= tol * max(1., abs(b))


def _root(model_file, seqs, strategy):
    """((a,b),c) for three sequences, ((a,b),(c,d)) for four: the root's CarryForwardMatrix, filled"""
    root = R.root_pair(ho.RateModel.from_file(M + model_file), seqs, TIMES, strategy)
    root.fill()
    return root


CASES = [("jc.json", ["acg", "ag", "ct"]), ("jc.json", ["acg", "ag", "ct", "g"]), ("jc.json", ["acg", "t", "tca", "gg"]),
         ("jc.json", ["a", "c", "gt"]), ("wag.json", ["ar", "n", "dr"]), ("wag.json", ["arn", "an", "dr", "r"])]


@pytest.mark.parametrize("model_file,seqs", CASES)
def test_root_counts_are_the_expectation_over_whole_histories(model_file, seqs):
    with R.exact_log_sum_exp():
        root = _root(model_file, seqs, KEEP_ALL)
        got, x_post, y_post = R.get_indel_counts(ho.BackwardMatrix(root), root.tm)
        want = R.brute_force_indel_counts(root, root.tm)
        plain = cd.get_indel_counts(ho.BackwardMatrix(root), root.tm)
    assert _close(got["lp"], want["lp"])
    for k in R.KEYS:
        assert _close(got[k], want[k]), (k, got[k], want[k])
    # the carried counts are what this adds: without them the internal node's events are missing
    assert got["insTime"] > plain["insTime"] + .1 and got["delTime"] > plain["delTime"] + .1
    # every path leaves START of each profile along one transition
    for prof, post in ((root.x, x_post), (root.y, y_post)):
        assert _close(sum(post[t] for t in prof.state[0].null_out + prof.state[0].absorb_out), 1., 1e-12)


@pytest.mark.parametrize("model_file,seqs", CASES)
def test_collapsed_chains_carry_the_same_counts(model_file, seqs):
    with R.exact_log_sum_exp():
        keep = _root(model_file, seqs, KEEP_ALL)
        coll = _root(model_file, seqs, COLLAPSE)
        a, _, _ = R.get_indel_counts(ho.BackwardMatrix(keep), keep.tm)
        b, _, _ = R.get_indel_counts(ho.BackwardMatrix(coll), coll.tm)
    assert len(coll.x.state) <= len(keep.x.state)
    assert _close(coll.lp_end, keep.lp_end)
    for k in R.KEYS:
        assert _close(b[k], a[k]), (k, b[k], a[k])


@pytest.mark.parametrize("seqs", [["acgtac", "agtac", "cgta", "acta"], ["aacgtt", "acgt", "ttacg", "tacg"]])
@pytest.mark.parametrize("kind", ["sampled", "posterior"])
def test_collapsing_mixes_the_counts_of_paths_that_meet(seqs, kind):
    # (((a,b),c),d): the ((a,b),c) profile is made over the posterior profile of (a,b), whose null states give several routes
    # through eliminated cells between the same two retained cells - makeProfile's mixing (counts *= 1 - pp;
    # counts += (src + dest) * pp) then runs with pp < 1.  The same cells kept whole (KeepAll) are the yardstick.
    model = ho.RateModel.from_file(M + "jc.json")
    env = ho.GuideAlignmentEnvelope()

    def hmm(tl, tr):
        return ho.PairHMM(ho.ProbModel(model, tl), ho.ProbModel(model, tr), model.ins_prob)
    got = []
    with R.exact_log_sum_exp():
        leaves = [ho.Profile.from_seq(1, model.alphabet, s, k, "n%d" % k) for k, s in enumerate(seqs)]
        f1 = R.CarryForwardMatrix(leaves[0], leaves[1], hmm(.3, .4), 10, env, model)
        p1 = ho.BackwardMatrix(f1).post_prob_profile(.001, 0, COLLAPSE | ho.DPMatrix.IncludeBestTrace)
        f2 = R.CarryForwardMatrix(p1, leaves[2], hmm(.35, .3), 11, env, model)
        for strategy in (KEEP_ALL | ho.DPMatrix.IncludeBestTrace, COLLAPSE | ho.DPMatrix.IncludeBestTrace):
            R.CarryForwardMatrix.partial_mixes = 0
            p2 = (f2.sample_profile(ho.MT19937(3), 20, 0, strategy) if kind == "sampled"
                  else ho.BackwardMatrix(f2).post_prob_profile(.001, 0, strategy))
            mixes = R.CarryForwardMatrix.partial_mixes
            root = R.CarryForwardMatrix(p2, leaves[3], hmm(.2, .3), 12, env, model)
            got.append((R.get_indel_counts(ho.BackwardMatrix(root), root.tm)[0], mixes))
    (keep, keep_mixes), (coll, coll_mixes) = got
    assert keep_mixes == 0 and coll_mixes > 0
    for k in R.KEYS + ("lp",):
        assert _close(coll[k], keep[k]), (k, coll[k], keep[k])


@pytest.mark.parametrize("xs,ys,t_l,t_r", [("ac", "ag", .1, .2), ("acg", "ag", .3, .1), ("a", "cgt", .2, .2), ("acgt", "act", .05, .4)])
def test_leaf_pairs_are_the_plain_restatement(xs, ys, t_l, t_r):
    model = ho.RateModel.from_file(M + "jc.json")
    hmm = ho.PairHMM(ho.ProbModel(model, t_l), ho.ProbModel(model, t_r), model.ins_prob)
    x = ho.Profile.from_seq(1, model.alphabet, xs, 1, "x")
    y = ho.Profile.from_seq(1, model.alphabet, ys, 2, "y")
    fwd = R.CarryForwardMatrix(x, y, hmm, 0, ho.GuideAlignmentEnvelope(), model)
    bwd = ho.BackwardMatrix(fwd)
    got, _, _ = R.get_indel_counts(bwd, fwd.tm)
    want = cd.get_indel_counts(bwd, fwd.tm)
    for k in R.KEYS + ("lp",):
        assert _close(got[k], want[k]), (k, got[k], want[k])


def test_ready_states_carry_nothing_and_keep_the_counts_of_what_they_copy():
    import random
    from tests import helpers as H
    model = ho.RateModel.from_file(M + "jc.json")
    rng = random.Random(0)
    anc = H.random_seq(rng, "acgt", 14)
    leaves = [ho.Profile.from_seq(1, model.alphabet, H.mutate(rng, anc, "acgt", .15, .06), k, "n%d" % k) for k in range(2)]
    hmm = ho.PairHMM(ho.ProbModel(model, .1), ho.ProbModel(model, .2), model.ins_prob)
    f = R.CarryForwardMatrix(leaves[0], leaves[1], hmm, 10, ho.GuideAlignmentEnvelope(), model)
    prof = ho.BackwardMatrix(f).post_prob_profile(.01, 0, COLLAPSE | ho.DPMatrix.IncludeBestTrace)
    assert len(prof.trans_counts) == len(prof.trans)
    ready = [t for t, tr in enumerate(prof.trans) if prof.state[tr.dest].name.endswith(".")]
    assert ready and all(prof.trans_counts[t] == R.ZERO for t in ready)
    # the absorbing transitions moved onto the ready state keep their counts
    moved = [t for t, tr in enumerate(prof.trans) if prof.state[tr.src].name.endswith(".")]
    assert moved and all(sum(prof.trans_counts[t]) > 0 for t in moved)
    # without CountIndelEvents nothing is carried
    assert not hasattr(f.make_profile(R.all_cells(f, ho.BackwardMatrix(f)), ho.DPMatrix.CollapseChains), "trans_counts")
