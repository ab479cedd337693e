"""k_quickalign (hx_quick.hip, through the C ABI) on the cases of tests/quickalign_edge_cases.py: every cell of every pair, the
score and the end cell against oracle/oracle_quickalign.c, bit for bit and without a tolerance (the kernel only adds and takes
maxima).  What the cases are and why: that module's docstrings; that they hold what they claim: tests/test_oracle_quickalign_edges.py.

The envelope `[]` goes through capi.QuickBatch like the others: numpy hands over a non-null pointer for an empty array (asserted
below), so the job is a sparse one without a diagonal and not a full one."""
import numpy as np
import pytest

from historian_amd import capi
from oracle import c_oracle
from tests import quickalign_edge_cases as E
from tests.quickalign_helpers import check_jobs

pytestmark = pytest.mark.gpu
WAVES = (0, 1, 2, 4, 8)     # HX_QA_WAVES; 0 leaves the hook unset (the launch's own choice)


@pytest.fixture(scope="module", autouse=True)
def engine():
    capi.init(0, c_oracle.table())
    yield
    capi.shutdown()


def force_waves(monkeypatch, waves):
    if waves:
        monkeypatch.setenv("HX_QA_WAVES", str(waves))       # read at every launch
    else:
        monkeypatch.delenv("HX_QA_WAVES", raising=False)


def check_cases(cases):
    """one batch of the cases, compared with their (cached) oracle results; -> {name: (cells, score, x_end, y_end)} of the device"""
    got = check_jobs([c[1:] for c in cases], [E.oracle(c) for c in cases], [c[0] for c in cases])
    return {c[0]: g for c, g in zip(cases, got)}


@pytest.mark.parametrize("waves", WAVES)
def test_end_cell_ties(monkeypatch, waves):
    """One wave handing every strip to itself, two to eight waves with several rounds of strips, and the default launch, on pairs
    whose maximum is reached in several cells: the smaller j, then the smaller i wins, as in the reference's column-major scan."""
    force_waves(monkeypatch, waves)
    got = check_cases(E.tie_cases())
    for c in E.repeat_tie_cases():
        # the reference's traceback over the device matrix, from the device's end cell
        want = E.oracle(c)
        mine = E.align_path_over(c, *got[c[0]])
        assert mine == E.align_path_over(c, want["cells"], want["score"], want["x_end"], want["y_end"]), c[0]


@pytest.mark.parametrize("waves", WAVES)
def test_shape_grid(monkeypatch, waves):
    force_waves(monkeypatch, waves)
    cases = E.shape_grid_cases()
    assert len(cases) == 92
    check_cases(cases)


def test_alphabets_and_foreign_tokens():
    check_cases(E.alphabet_cases())


@pytest.mark.parametrize("waves", (0, 1))
def test_degenerate_envelopes(monkeypatch, waves):
    """Envelopes without a cell (score -inf, end cell (0, 0)), with one corner cell, without neighbouring diagonals, and two
    full-envelope pairs in the same batch (the membership-testing kernel with a null bitmap)."""
    force_waves(monkeypatch, waves)
    cases = E.envelope_cases()
    b = capi.QuickBatch([c[1:] for c in cases if c[0].endswith("_empty")])
    try:
        assert all(b._jobs[k].n_diagonals == 0 and bool(b._jobs[k].diagonals) for k in range(b.n))
    finally:
        b.close()
    got = check_cases(cases)
    for c in cases:
        if c[0].split("_", 2)[2] in E.NO_CELL:
            cells, score, xe, ye = got[c[0]]
            assert score == E.NEG_INF and (xe, ye) == (0, 0) and not np.isfinite(cells).any()


def test_column_tables_at_the_lds_limit():
    for batch in E.column_table_batches():
        check_cases(batch)


@pytest.mark.parametrize("n_pairs", E.LARGE_BATCHES)
def test_large_batches_take_the_narrow_launches(monkeypatch, n_pairs):
    """From 128 pairs the launch takes at most 8 waves a pair, from 384 at most 4: 641 rows are 11 strips on either."""
    monkeypatch.delenv("HX_QA_WAVES", raising=False)
    check_cases(E.large_batch(n_pairs))


@pytest.mark.parametrize("set_name", E.SCORE_SETS)
def test_score_sets(set_name):
    check_cases(E.score_set_cases(set_name))


def test_rerun_and_refusals():
    cases = E.score_set_cases("integer") + E.envelope_cases()[:4]
    jobs = [c[1:] for c in cases]

    def everything(b):
        score, xe, ye = b.results()
        lay = [b.layout(k) for k in range(b.n)]
        raw = []
        for k in range(b.n):
            buf = np.empty(lay[k].matrix_doubles)
            capi._check(capi.load().hx_quick_batch_read_matrix(b._h, k, capi._p(buf, capi._f64p)))
            raw.append(buf.tobytes())             # every slot of the device matrix, padding included
        return (score.tobytes(), xe.tobytes(), ye.tobytes(), [b.read_matrix(k).tobytes() for k in range(b.n)]), raw

    b1, b2 = capi.QuickBatch(jobs), capi.QuickBatch(jobs)
    try:
        with pytest.raises(capi.HxError):
            b1.results()                          # before run()
        with pytest.raises(capi.HxError):
            b1.read_matrix(0)
        b1.run()
        first = everything(b1)
        b1.run()
        assert everything(b1) == first            # (slots that no lane writes keep what the allocation held)
        b2.run()
        assert everything(b2)[0] == first[0]
    finally:
        b1.close()
        b2.close()

    name, x, y, a, sm, sv, d = E.score_set_cases("integer")[0]
    too_high = x.copy()
    too_high[5] = a
    none = np.zeros(0, dtype=np.int32)
    refused = {
        "alph 0": (x, y, 0, sm, sv, None),
        "alph 32": (x, y, 32, np.zeros((32, 32)), sv, None),
        "token equal to alph (x)": (too_high, y, a, sm, sv, None),
        "token equal to alph (y)": (x, too_high[:len(y)], a, sm, sv, None),
        "empty x": (none, y, a, sm, sv, None),
        "empty y": (x, none, a, sm, sv, None),
        "diagonal x_len + 1": (x, y, a, sm, sv, [0, len(x) + 1]),
        "diagonal -y_len - 1": (x, y, a, sm, sv, [-len(y) - 1, 0]),
    }
    for what, job in refused.items():
        with pytest.raises(capi.HxError):
            capi.QuickBatch([job])
            pytest.fail("accepted: " + what)
    # ... and the neighbouring legal values are taken
    check_cases([E.case("legal_outermost_diagonals", x, y, "integer", [-len(y), 0, len(x)])])
