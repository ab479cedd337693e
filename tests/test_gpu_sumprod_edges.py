"""hx_sumprod_columns where its launcher takes another path than on the shapes of tests/test_gpu_sumprod.py: the cases of
tests/sumprod_edge_cases.py (pinned by tests/test_oracle_sumprod_edges.py) against the sum-product oracle, accumulated
column by column with the same weights - trees deep enough for the 1e-30 rescaling, more than eight components (a wave
takes a second component and stages its eigenvectors again), matrices through the scalar cache instead of LDS, alphabet
sizes at the edges of the outer-product kernels' plans, a second slice of the row sums - and the steady state of the two
outer-product kernels (HX_SUMPROD_SLICES: several blocks, or tiles, of columns per workgroup), chunks of a rescaled case.

Bounds are those of tests/test_gpu_sumprod.py.  A = 4 and 20 (kernels of their own): column likelihoods 1e-12 relative (an
all-wildcard column's likelihood is 1: there the 1e-13 floor of tests/test_gpu_ancestors.py), root counts 1e-10 relative,
eigen counts and counts 1e-10 of the largest entry, root posteriors 1e-8 relative.  Any other alphabet
(test_alphabets_without_a_kernel_of_their_own): 1e-11 relative + 1e-13, 1e-9, 1e-9, 1e-8 of the largest entry."""
import functools

import numpy as np
import pytest

from historian_amd import capi, counts, hostmodel
from oracle import c_oracle
from tests import sumprod_edge_cases as EC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def engine():
    capi.init(0, c_oracle.table())
    yield
    capi.shutdown()


@functools.lru_cache(maxsize=None)
def counter(name):
    s, ref = EC.spec(name), EC.reference(name)
    model = hostmodel.RateModel(s.js)
    # the device gets the oracle's exp(R t) so that the comparison is of the passes, not of two matrix exponentials
    cc = counts.ColumnCounter(model, s.parent, s.length, branch_sub=ref.branch_sub)
    assert (np.abs(np.asarray(cc.eigen.evec).imag).max() > 1e-6) == (not s.reversible)
    return cc, counts.tokenize_columns(model.alphabet, s.rows)


def run(name):
    s = EC.spec(name)
    cc, tok = counter(name)
    assert (tok == counts.WILD).sum() == sum(row.count("x") for row in s.rows)         # every symbol of the alphabet is a token
    return cc.run(tok, s.weight, want_root_post=s.root_post)


@functools.lru_cache(maxsize=None)
def default_run(name):
    """the launcher's own plan (called before a test sets a variable); computed once, never modified"""
    return run(name)


def check(name, got, what="the launcher's plan"):
    """-> the worst deviations, printed"""
    s, ref = EC.spec(name), EC.reference(name)
    own = s.a in (4, 20)
    want = ref.col_log_like
    err = np.abs(got["col_log_like"] - want)
    if own:
        tol = 1e-12 * np.abs(want) + np.where(np.abs(want) < 1e-6, 1e-13, 0.)
    else:
        tol = 1e-11 * np.abs(want) + 1e-13
    far = np.abs(want) >= 1e-6
    worst = dict(ll=float(np.max(err[far] / np.abs(want[far]))), root=0., eigen=0., counts=0., post=0.)
    for cpt in range(s.c):
        r, e, c = ref.root[cpt], ref.eig[cpt], ref.counts[cpt]
        with np.errstate(invalid="ignore", divide="ignore"):
            worst["root"] = max(worst["root"], float(np.nanmax(np.where(r > 0, np.abs(got["root_counts"][cpt] - r) / r, 0.))))
        worst["eigen"] = max(worst["eigen"], float(np.abs(got["eigen_counts"][cpt] - e).max() / np.abs(e).max()))
        worst["counts"] = max(worst["counts"], float(np.abs(got["counts"][cpt] - c).max() / np.abs(c).max()))
    for col, lpp in ref.root_post.items():
        w = np.exp(lpp)
        worst["post"] = max(worst["post"], float(np.max(np.where(w > 0, np.abs(np.exp(got["root_post"][col]) - w) / np.where(w > 0, w, 1.), 0.))))
    print("%s, %s: worst deviation of a column likelihood %.3g (relative), root count %.3g (relative), eigen count %.3g, count %.3g "
          "(of the largest entry), root posterior %.3g (relative)" % (name, what, worst["ll"], worst["root"], worst["eigen"], worst["counts"], worst["post"]))
    assert np.all(err <= tol), int(np.argmax(err - tol))
    for cpt in range(s.c):
        r, e, c = ref.root[cpt], ref.eig[cpt], ref.counts[cpt]
        if own:
            np.testing.assert_allclose(got["root_counts"][cpt], r, rtol=1e-10, atol=1e-12 * r.max())
        else:
            np.testing.assert_allclose(got["root_counts"][cpt], r, rtol=1e-9)
        np.testing.assert_allclose(got["eigen_counts"][cpt], e, rtol=0, atol=(1e-10 if own else 1e-9) * np.abs(e).max())
        np.testing.assert_allclose(got["counts"][cpt], c, rtol=0, atol=(1e-10 if own else 1e-8) * np.abs(c).max())
    assert (got["root_post"] is not None) == s.root_post
    for col, lpp in ref.root_post.items():
        np.testing.assert_allclose(np.exp(got["root_post"][col]), np.exp(lpp), rtol=1e-8, atol=1e-300, err_msg="column %d" % col)
    return worst


@pytest.mark.parametrize("name", list(EC.COUNTS))
def test_edge_cases_against_the_oracle(name):
    check(name, default_run(name))
    assert capi.sumprod_kernel_ms() > 0


@pytest.mark.parametrize("name,slices", [("bal64 prot4", 1), ("bal64 prot4", 2), ("alphabet 33", 1), ("alphabet 33", 2),
                                         ("many columns", 3), ("many columns", 4)])
def test_several_blocks_per_workgroup_of_the_matrix_core_outer_product(name, slices, monkeypatch):
    """2, 3, 22 and 16 | 17 blocks of 64 columns per workgroup: both register buffers, the refetch two blocks ahead, the
    loop left after an odd and after an even number of blocks (tests/test_oracle_sumprod_edges.py has the numbers)"""
    whole = default_run(name)
    monkeypatch.setenv("HX_SUMPROD_SLICES", str(slices))
    got = run(name)
    check(name, got, "%d slices" % slices)
    assert got["col_log_like"].tobytes() == whole["col_log_like"].tobytes()        # (they do not depend on the slices)


@pytest.mark.parametrize("slices", [1, 2])
@pytest.mark.parametrize("name", ["cat40 cyclic", "cyclic 21", "prot x 9"])
def test_several_tiles_per_workgroup_of_the_vector_unit_outer_products(name, slices, monkeypatch):
    """5, and 3 | 2, tiles of 32 columns per workgroup of k_outer_counts<false> (the cyclic models) and <true> (HX_SUMPROD_NO_MFMA)"""
    whole = default_run(name)
    monkeypatch.setenv("HX_SUMPROD_NO_MFMA", "1")
    monkeypatch.setenv("HX_SUMPROD_SLICES", str(slices))
    got = run(name)
    check(name, got, "vector units, %d slices" % slices)
    assert got["col_log_like"].tobytes() == whole["col_log_like"].tobytes()


def test_chunks_of_a_rescaled_case(monkeypatch):
    """bal64 prot4 in chunks of 64 columns (the smallest budget that holds 64: the launcher's formula, restated in
    EC.counts_chunk): the same column likelihoods to the bit, counts within the bound"""
    name = "bal64 prot4"
    s = EC.spec(name)
    whole = default_run(name)
    mb = EC.counts_chunk_mb(s.a, s.c, s.n, True, 64)
    assert EC.counts_chunk(s.a, s.c, s.n, s.n_cols, True, mb) == 64 < s.n_cols
    monkeypatch.setenv("HX_SUMPROD_SCRATCH_MB", str(mb))
    got = run(name)
    check(name, got, "chunks of 64 columns")
    assert got["col_log_like"].tobytes() == whole["col_log_like"].tobytes()
