"""The yardstick of the resident history's edge tests (tests/history_edge_cases.py), with the oracle alone: every case
takes the launch plan it names; no column likelihood of the oracle is non-finite; the two deep cases pass the reference's
1e-30 rescaling - at wildcards in one, at residues in the other - and go on doing so on the branch lengths of the deep
proposals, which would otherwise not test rescaling; the seeded random walk covers what it is there for; the restated sum
of tests/history_ref.py adds what it says it adds."""
import math

import numpy as np
import pytest

from tests import history_edge_cases as HE
from tests import history_ref as HR


@pytest.mark.parametrize("name", list(HE.HISTORY))
def test_the_launch_plan_of_every_case_and_a_finite_oracle(name):
    c = HE.case(name)
    plan = HE.history_plan(c.a, c.c)
    assert {k: plan[k] for k in c.plan} == c.plan, plan
    assert plan["lds"] <= 96 * 1024 and (c.c > 8 or plan["waves"] < c.c) == (plan["turns"] > 1)
    assert len(c.want) % 64 != 0 and np.all(np.isfinite(c.want))
    # `on`, which evaluates the proposals' trees, is the oracle's fill_up: on the case's own lengths, the case's own bits
    same = c.on(c.length)
    assert same.want == c.want and (same.wild_rescales, same.residue_rescales) == (c.wild_rescales, c.residue_rescales)
    assert np.array_equal(same.branch_sub, c.branch_sub)
    print("%s: A %d, C %d, N %d, %d columns, plan %s; the oracle rescaled %d wildcard vectors and %d residue entries"
          % (name, c.a, c.c, c.n, len(c.want), plan, c.wild_rescales, c.residue_rescales))


def test_the_plans_shed_waves_where_the_issue_says():
    assert HE.history_plan(64, 3)["waves"] == 2 and HE.history_plan(46, 6)["waves"] == 5
    assert HE.history_plan(64, 128) == dict(ta=0, waves=1, turns=128, lds=96 * 1024)
    assert HE.history_plan(64, 2)["waves"] == 2 and HE.history_plan(44, 6)["waves"] == 6         # (the last that keep theirs)
    assert HE.sum_plan(len(HE.case("many columns").want)) == dict(per_thread=(4, 5), blocks=66)


def test_the_deep_cases_rescale_before_and_after_the_deep_proposals():
    wild, residue = HE.case("anc cat64 mix12"), HE.case("cat40 mix12")
    assert wild.wild_rescales >= 1 and residue.residue_rescales >= 1
    for name, counted in (("anc cat64 mix12", "wild_rescales"), ("cat40 mix12", "residue_rescales")):
        c = HE.case(name)
        states = HE.deep_states(name)
        assert [accepted for _, _, accepted in states] == [True, False, True]
        for nodes, new, _ in states:
            print("%s after %s: %d wildcard vectors, %d residue entries rescaled" % (name, nodes, new.wild_rescales, new.residue_rescales))
            assert getattr(new, counted) >= 1 and np.all(np.isfinite(new.want))
            assert any(a != b for a, b in zip(new.want, c.want))
        # what each proposal walks: the whole spine; the top leaf and the root; a leaf, a stretch of the spine
        leaves = (c.n + 1) // 2
        assert HE.walked_nodes(c.parent, states[0][0]) == [0] + list(range(leaves, c.n))
        assert HE.walked_nodes(c.parent, states[1][0]) == [leaves - 1, c.n - 1]
        third = HE.walked_nodes(c.parent, states[2][0])
        assert third[0] == leaves // 2 and third[1:] == list(range(c.parent[leaves // 2], c.n))
        # there are columns that each of them leaves alone
        roots = HE.column_roots(c)
        for nodes, _, _ in states:
            assert sum(r not in HE.walked_nodes(c.parent, nodes) for r in roots) >= 3


@pytest.mark.parametrize("name", HE.TWO_LEAVES)
def test_the_two_leaf_proposals_name_unrelated_leaves(name):
    c = HE.case(name)
    (nodes, first), (every, second) = HE.two_leaf_states(name)
    assert len(nodes) == 2 and all(r not in c.parent for r in nodes) and every == list(range(c.n - 1))
    assert np.all(np.isfinite(first.want)) and np.all(np.isfinite(second.want))
    assert first.want != c.want and second.want != first.want


def test_the_random_walk_covers_what_it_is_there_for():
    c = HE.case(HE.WALK)
    steps = HE.walk_steps(c.n)
    cover = HE.walk_coverage(c.parent, steps)
    print(cover)
    assert (c.n, len(c.want), len(steps)) == (13, 70, 60)
    assert all(0 < len(set(nodes)) == len(nodes) and 0 <= min(nodes) and max(nodes) <= c.n - 2 for nodes, _, _ in steps)
    assert all(.01 < t < .8 for _, ts, _ in steps for t in ts)
    assert cover["accepts"] >= 10 and cover["rejects"] >= 10
    assert cover["root_child"] >= 1 and cover["far_ancestor"] >= 1
    assert {1, 2, c.n - 1} <= cover["sizes"]
    assert min(cover["drift"]) >= 2


def test_the_restated_sum_on_sums_it_can_be_checked_on():
    # integers below 2^53 add exactly in any order; one column per thread and a ragged tail
    for n in (1, 2, 70, 1023, 1024, 1025, 4200):
        v = np.arange(1, n + 1, dtype=float)
        assert HR.history_sum(v) == n * (n + 1) / 2
    # the order is the kernel's: thread 0 adds columns 0 and 1024 first, and only then its neighbour's 2^-53
    v = np.zeros(1025)
    v[0], v[1], v[1024] = 1., 2. ** -53, -1.
    assert HR.history_sum(v) == 2. ** -53 and math.fsum(v) == 2. ** -53
    v[0], v[1], v[1024] = 1., -1., 2. ** -53
    assert HR.history_sum(v) == 0.                                 # ((1 + 2^-53) - 1: rounded away in thread 0)
