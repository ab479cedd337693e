"""The yardstick of the sum-product edge tests (tests/sumprod_edge_cases.py), with the oracle alone: every column has one
root and a finite likelihood; in the deep-tree cases the reference's 1e-30 rescaling does fire, at wildcards and at
residues; no outside message G comes near the underflow of a double (the reference never rescales G: below about 1e-200
the oracle would be the one that is wrong); and the restated launch plans give every case the plan it is there for."""
import numpy as np
import pytest

from tests import sumprod_edge_cases as EC

ALL = list(EC.COUNTS) + list(EC.ANCESTORS)


@pytest.mark.parametrize("name", ALL)
def test_columns_have_one_root_and_the_oracle_stays_in_range(name):
    ref = EC.reference(name)
    assert np.all(ref.roots == 1)
    assert np.all(np.isfinite(ref.col_log_like))
    shared = np.mean(ref.rescaled_wild + ref.rescaled_residue > 0)
    print("%s: columns with a rescaled node %.0f %% (at a wildcard: %d nodes, at a residue: %d), smallest positive G %.3g, E %.3g"
          % (name, 100 * shared, ref.rescaled_wild.sum(), ref.rescaled_residue.sum(), ref.min_g, ref.min_e))
    assert ref.min_g > 1e-200


@pytest.mark.parametrize("name", EC.DEEP)
def test_deep_trees_rescale_at_wildcards_and_at_residues(name):
    ref = EC.reference(name)
    assert np.mean(ref.rescaled_wild + ref.rescaled_residue > 0) >= .1
    assert ref.rescaled_wild.sum() > 0 and ref.rescaled_residue.sum() > 0


@pytest.mark.parametrize("name", ["anc bal64 prot4", "anc cat64 mix12"])
def test_deep_reconstructions_rescale_at_their_wildcards(name):
    ref = EC.reference(name)
    assert np.mean(ref.rescaled_wild > 0) >= .1


@pytest.mark.parametrize("name", ALL)
def test_the_launch_plan_of_every_case(name):
    s = EC.spec(name)
    if name in EC.COUNTS:
        plan = EC.counts_plan(s.a, s.c, s.n, s.n_cols, s.reversible)
    else:
        plan = EC.ancestors_plan(s.a, s.c)
    assert {k: plan[k] for k in s.plan} == s.plan, plan
    assert all(len(row) == s.n_cols for row in s.rows) and s.n_cols % 64 != 0


def test_the_plans_of_the_forced_slices():
    """what HX_SUMPROD_SLICES makes of the steady-state cases: odd and even numbers of blocks per workgroup, more than
    one tile per workgroup; the chunk size of the rescaled case"""
    s = EC.spec("bal64 prot4")
    assert [EC.counts_plan(s.a, s.c, s.n, s.n_cols, True, slices=k)["blocks_per_group"] for k in (None, 1, 2)] == [[1], [2], [1]]
    s = EC.spec("alphabet 33")
    assert [EC.counts_plan(s.a, s.c, s.n, s.n_cols, True, slices=k)["blocks_per_group"] for k in (None, 1, 2)] == [[1], [3], [1, 2]]
    s = EC.spec("many columns")
    assert [EC.counts_plan(s.a, s.c, s.n, s.n_cols, True, slices=k)["blocks_per_group"] for k in (None, 3, 4)] == [[1], [22], [16, 17]]
    for name, real in (("cat40 cyclic", False), ("cyclic 21", False), ("prot x 9", True)):
        s = EC.spec(name)
        plans = [EC.counts_plan(s.a, s.c, s.n, s.n_cols, real, slices=k, no_mfma=True) for k in (None, 1, 2)]
        assert all(p["outer"].startswith("vector units") for p in plans)
        assert [p["tiles_per_group"] for p in plans] == [[1], [5], [2, 3]]
    s = EC.spec("bal64 prot4")
    assert EC.counts_chunk(s.a, s.c, s.n, s.n_cols, True, EC.counts_chunk_mb(s.a, s.c, s.n, True, 64)) == 64 < s.n_cols
    assert EC.counts_chunk(s.a, s.c, s.n, s.n_cols, True, 16 << 10) == s.n_cols
