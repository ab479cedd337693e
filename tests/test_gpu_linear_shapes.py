"""Shapes of the scaled-probability leaf fill (hx_linear.hip k_fill_leaf_linear), truncating and untruncated, Forward and Backward.

The step loop handles two anti-diagonals per iteration, hands the strip above's last row from wave to wave through LDS
rings and, with more strips than waves, from the last wave to the first through the matrix.  The sizes below hit every
branch of that: matrices of 2, 63, 64, 65, 129 and 2001 rows (a single partial strip, one short of a strip, exactly one,
one row into a second, a third, and the headline's 32) against 2, 3, 63, 64, 65 and 2001 columns (odd and even: the second
cell of the last step pair is outside the lattice for one of them), every pairing, with 8, 4, 2 and 1 waves per pair
(HX_LINEAR_WAVES; one workgroup per pair) and in the default launch, which deals the pairs of such a small batch to several
workgroups each.

Yardsticks and tolerances are those of tests/test_gpu_trunc.py and tests/test_gpu_parity.py: the oracle's recursion in libm
arithmetic with the reference's truncation (true_math=2) resp. without it (true_math=True) - the same -inf pattern, finite
cells within 1e-9, lpEnd within 1e-12 relative; the untruncated Backward fill's lpStart within 1e-12 relative of the
oracle's and 1e-11 of lpEnd, the truncating one's within 1e-4 of lpEnd (Forward and Backward drop different terms)."""
import numpy as np
import pytest

from historian_amd import capi
from oracle import c_oracle
from tests import helpers as H

pytestmark = pytest.mark.gpu

ROWS = (2, 63, 64, 65, 129, 2001)
COLS = (2, 3, 63, 64, 65, 2001)
AA = "arndcqeghilkmfpstwyv"


@pytest.fixture(scope="module", autouse=True)
def engine():
    capi.init(0, c_oracle.table())      # host-libm table
    yield
    capi.shutdown()


@pytest.fixture(scope="module")
def pairs():
    cases = []
    for a, rows in enumerate(ROWS):
        for b, cols in enumerate(COLS):
            k = a * len(COLS) + b
            # (a sequence of n residues is a profile of n + 1 states; every third pair a protein model)
            cases.append(H.leaf_case(900 + k, rows - 1, cols - 1, alphabet=AA, jc=False, tl=.2, tr=.3) if k % 3 == 0
                         else H.leaf_case(900 + k, rows - 1, cols - 1))
    return [H.job_images(f) for f in cases], {}      # (and the oracle's results, computed once per pair and yardstick)


def oracle(pairs, k, which, tm):
    imgs, cache = pairs
    if (k, which, tm) not in cache:
        fn = c_oracle.backward if which else c_oracle.forward
        cache[(k, which, tm)] = fn(*imgs[k], true_math=tm)
    return cache[(k, which, tm)]


@pytest.mark.parametrize("policy", ["trunc", "linear"])
@pytest.mark.parametrize("waves", [8, 4, 2, 1, 0])
def test_every_shape_forward_and_backward(waves, policy, pairs, monkeypatch):
    if waves:
        monkeypatch.setenv("HX_LINEAR_WAVES", str(waves))
        monkeypatch.setenv("HX_CHAIN_MULTI", "0")        # one workgroup per pair: the launch HX_LINEAR_WAVES shapes
    imgs = pairs[0]
    flag, tm = (capi.HX_LSE_TRUNC, 2) if policy == "trunc" else (capi.HX_LSE_LINEAR, True)
    b = capi.Batch(imgs, flag | capi.HX_KEEP_BACKWARD)
    b.forward()
    b.backward()
    lp_end, lp_start = b.lp_end(), b.lp_start()
    for k in range(len(imgs)):
        rows, cols = ROWS[k // len(COLS)], COLS[k % len(COLS)]
        what = "%d x %d, %s, %d waves" % (rows, cols, policy, waves)
        for which in (0, 1):
            want = oracle(pairs, k, which, tm)
            got = b.read_matrix(k, which)
            assert got.shape[:2] == (rows, cols), what
            assert not np.isnan(got).any(), what
            assert np.array_equal(np.isneginf(want["cells"]), np.isneginf(got)), "%s: -inf pattern (%s)" % (what, "FB"[which])
            fin = np.isfinite(got)
            assert np.max(np.abs(want["cells"][fin] - got[fin]), initial=0.) < 1e-9, "%s (%s)" % (what, "FB"[which])
        want_end = oracle(pairs, k, 0, tm)["lp_end"]
        assert np.isfinite(want_end), what
        assert abs(want_end - lp_end[k]) <= 1e-12 * abs(lp_end[k]), what
        if policy == "linear":
            assert abs(oracle(pairs, k, 1, tm)["lp_start"] - lp_start[k]) <= 1e-12 * abs(lp_start[k]), what
            assert abs(lp_start[k] - lp_end[k]) <= 1e-11 * abs(lp_end[k]), what
        else:
            assert abs(lp_start[k] - lp_end[k]) <= 1e-4 * abs(lp_end[k]), what
    b.close()
