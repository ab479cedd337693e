"""hx_sumprod_ancestors where its launcher takes another path than on the shapes of tests/test_gpu_ancestors.py: the
reconstruction-shaped cases of tests/sumprod_edge_cases.py (pinned by tests/test_oracle_sumprod_edges.py) - exp(R t)
through the scalar cache instead of LDS (64 symbols x 3 components, 46 x 6), more than eight components on either side of
the combining kernel's switch from four waves to one (20 and 21 symbols), a balanced 64-leaf tree of the protein mixture
and 40- and 64-leaf caterpillars of a 12-component DNA mixture, internal nodes '*' (the upper nodes of the 64-leaf trees pass
through the 1e-30 rescaling) - against the oracle's log_node_post_prob at every node of every column.

Bounds: those of tests/test_gpu_ancestors.py (Case.check) - posteriors 1e-8 relative, column likelihoods 1e-12 relative, `best`
equal everywhere: the seeds are such that the oracle has no top-two gap below 1e-6 among these cells, which Case.check asserts."""
import functools

import numpy as np
import pytest

from historian_amd import capi
from oracle import c_oracle
from tests import sumprod_edge_cases as EC
from tests.test_gpu_ancestors import Case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def engine():
    capi.init(0, c_oracle.table())
    yield
    capi.shutdown()


@functools.lru_cache(maxsize=None)
def case(name):
    s = EC.spec(name)
    return Case(s.js, s.parent, s.length, s.rows)


@pytest.mark.parametrize("name", list(EC.ANCESTORS))
def test_edge_cases_against_the_oracle_with_and_without_posteriors(name):
    s, c = EC.spec(name), case(name)
    assert (c.sp.A, c.sp.C, len(c.want)) == (s.a, s.c, s.n_cols) and s.n_cols >= 20
    ap = c.predictor()
    got = ap.run(c.tokens, want_post=True)
    print(name, end=": ")
    cells, _ = c.check(got)
    assert cells > 200
    assert capi.sumprod_kernel_ms() > 0
    lean = ap.run(c.tokens)                                  # k_ancestor_combine<false>: the same picks, checked above
    assert lean["node_post"] is None
    assert lean["best"].tobytes() == got["best"].tobytes() and lean["col_log_like"].tobytes() == got["col_log_like"].tobytes()
