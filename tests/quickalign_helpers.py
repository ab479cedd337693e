"""What the guide-alignment GPU tests share (tests/test_gpu_quickalign.py, tests/test_gpu_quickalign_edges.py): one batch
through the C ABI, every pair compared with oracle/oracle_quickalign.c bit for bit."""
from historian_amd import capi
from oracle import c_oracle
from oracle import quickalign_oracle as q
from tests import helpers as H


def score_vector(sc):
    return [getattr(sc, n) for n in capi.QuickBatch.SCORE_NAMES]


def check_jobs(jobs, wants, names=None):
    """jobs: the tuples of capi.QuickBatch; wants: per job the dict of c_oracle.quickalign.  One batch, one launch; every cell,
    the score and the end cell of every pair must equal the oracle's.  Returns per job (cells, score, x_end, y_end) of the device."""
    b = capi.QuickBatch(jobs)
    try:
        b.run()
        score, xe, ye = b.results()
        got = []
        for k, want in enumerate(wants):
            what = "pair %d" % k if names is None else names[k]
            cells = b.read_matrix(k)
            H.assert_same_bits(cells, want["cells"], "%s cells" % what)
            H.assert_same_bits([score[k]], [want["score"]], "%s score" % what)
            assert (int(xe[k]), int(ye[k])) == (want["x_end"], want["y_end"]), what
            got.append((cells, float(score[k]), int(xe[k]), int(ye[k])))
    finally:
        b.close()
    return got


def run_and_check(pairs, A, sc):
    """pairs: list of (x, y, diagonals or None)"""
    jobs = [(q.tokens(x, A), q.tokens(y, A), len(A), sc.submat, score_vector(sc), d) for x, y, d in pairs]
    check_jobs(jobs, [c_oracle.quickalign(xt, yt, a, sm, sc, d) for xt, yt, a, sm, sv, d in jobs])
