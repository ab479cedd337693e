"""What the unbanded scaled-probability Forward fill (hx_linear.hip k_fill_leaf_linear) writes, and what it leaves alone.

A strip of the strip-skewed layout is a parallelogram inside a rectangle: lane l of a step pair t holds columns t - l and
t + 1 - l, so the rectangle's two skew triangles, and the rows past the matrix's last in its last strip, hold no lattice
cell.  The fill stores only the lanes of a step pair that hold one.  HX_POISON_MATRIX=1 fills the Forward block with the
byte 0xFF in front of the fill, which makes "not written" observable:

 1. every lattice cell against the yardsticks and tolerances of tests/test_gpu_linear_shapes.py (the oracle's recursion in
    libm arithmetic with the reference's truncation, true_math=2, resp. without it, true_math=True: the same -inf pattern,
    finite cells within 1e-9, lpEnd within 1e-12 relative, no NaN - a store masked away by mistake is the poison's NaN);
 2. every other slot of the raw block still holds the poison, unless it shares a 128-byte line of the matrix with a lattice
    cell (matrices are 1 KiB-aligned) - a rule that holds for lane-exact and for line-wide store masks alike;
 3. in every pair of at least 64 columns the number of poison slots left is exactly what the shipped mask - the lane range
    widened to whole 128-byte lines, groups of eight lanes - leaves: stored_slots below.  A fill that writes its padding
    fails this.

Sizes: 2, 17, 63, 64, 65 and 129 rows (a last strip of 2, 17, 63, 64, 1 and 1 live rows; one, two and three strips) against
2, 3, 63, 64, 65 and 130 columns (odd and even; shorter than, equal to and longer than a strip's skew), every pairing, both
policies, with 8, 4, 2 and 1 waves per pair (HX_LINEAR_WAVES, one workgroup per pair) and in the default launch.

The same fill writes the five chains of a cell relative to their first transitions (FOLD) when every pair of the launch has
its transitions within e^+-6.93 of one another; any other model runs the unfolded code.  test_fold_admission pins both sides:
the protein pairs above fold, tests/param_edge_cases.py's tiny_indel (gap transitions 27 nats below the others) does not,
HX_LINEAR_FOLD=0 turns the fold off, and all three meet the same yardsticks."""
import ctypes as C

import numpy as np
import pytest

from historian_amd import capi
from oracle import c_oracle
from tests import helpers as H
from tests import param_edge_cases as P

pytestmark = pytest.mark.gpu

ROWS = (2, 17, 63, 64, 65, 129)
COLS = (2, 3, 63, 64, 65, 130)
AA = "arndcqeghilkmfpstwyv"
POISON = np.uint64(0xFFFFFFFFFFFFFFFF)
LINE = 16       # doubles per 128-byte line


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


def oracle(pairs, k, tm):
    imgs, cache = pairs
    if (k, tm) not in cache:
        cache[(k, tm)] = c_oracle.forward(*imgs[k], true_math=tm)
    return cache[(k, tm)]


def stored_slots(rows, cols):
    """Slots the line-wide mask writes.  In the step pair of the skewed columns t, t + 1 (t even) lane l of a strip holds the
    columns t - l and t + 1 - l: a lattice cell iff t + 1 - cols <= l <= t + 1 and l is one of the strip's live rows.  That
    range of lanes, widened to whole groups of eight, stores: two slots per lane in each of five states."""
    n = 0
    for row0 in range(0, rows, 64):
        last = min(64, rows - row0) - 1
        for t in range(0, cols + last, 2):
            lo, hi = max(t + 1 - cols, 0), min(t + 1, last)
            assert lo <= hi
            n += (hi | 7) - (lo & ~7) + 1
    return 10 * n


def raw_block(b, k):
    l = b.layout(k, 0)
    buf = np.empty(l.matrix_doubles)
    rc = capi.load().hx_batch_read_matrix(b._h, k, 0, buf.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == 0
    return l, buf.view(np.uint64)


@pytest.mark.parametrize("policy", ["trunc", "linear"])
@pytest.mark.parametrize("waves", [8, 4, 2, 1, 0])
def test_forward_fill_writes_the_lattice_and_only_its_lines(waves, policy, pairs, monkeypatch):
    if waves:
        monkeypatch.setenv("HX_LINEAR_WAVES", str(waves))
        monkeypatch.setenv("HX_CHAIN_MULTI", "0")        # one workgroup per pair: the launch HX_LINEAR_WAVES shapes
    monkeypatch.setenv("HX_POISON_MATRIX", "1")
    imgs = pairs[0]
    flag, tm = (capi.HX_LSE_TRUNC, 2) if policy == "trunc" else (capi.HX_LSE_LINEAR, True)
    b = capi.Batch(imgs, flag)
    b.forward()
    lp_end = b.lp_end()
    for k in range(len(imgs)):
        rows, cols = ROWS[k // len(COLS)], COLS[k % len(COLS)]
        what = "%d x %d, %s, %d waves" % (rows, cols, policy, waves)
        # 1. the lattice
        want = oracle(pairs, k, tm)
        got = b.read_matrix(k, 0)
        assert got.shape[:2] == (rows, cols), what
        assert not np.isnan(got).any(), "%s: %d lattice values are NaN" % (what, int(np.isnan(got).sum()))
        assert np.array_equal(np.isneginf(want["cells"]), np.isneginf(got)), "%s: -inf pattern" % what
        fin = np.isfinite(got)
        assert np.max(np.abs(want["cells"][fin] - got[fin]), initial=0.) < 1e-9, what
        assert np.isfinite(want["lp_end"]), what
        assert abs(want["lp_end"] - lp_end[k]) <= 1e-12 * abs(lp_end[k]), what
        # 2. the padding
        l, raw = raw_block(b, k)
        assert (l.n_rows, l.n_cols, l.compressed) == (rows, cols, 0), what
        ii, jj = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
        slot = capi.slot_index(l, ii, jj).ravel()
        lattice = np.concatenate([s * l.plane_stride + slot for s in range(5)])
        assert len(np.unique(lattice)) == 5 * rows * cols and lattice.max() < l.matrix_doubles, what
        in_lattice = np.zeros(l.matrix_doubles, dtype=bool)
        in_lattice[lattice] = True
        line_live = np.zeros((l.matrix_doubles + LINE - 1) // LINE, dtype=bool)
        line_live[lattice // LINE] = True
        written = raw != POISON
        stray = written & ~in_lattice & ~line_live[np.arange(l.matrix_doubles) // LINE]
        print("%s: %d slots, %d lattice, %d written, %d poison, %d stray" %
              (what, l.matrix_doubles, len(lattice), int(written.sum()), int((~written).sum()), int(stray.sum())))
        assert not stray.any(), "%s: %d slots written in lines without a lattice cell, first at %d" % (what, int(stray.sum()), int(np.argmax(stray)))
        # 3. the mask acts
        if cols >= 64:
            assert int((~written).sum()) == l.matrix_doubles - stored_slots(rows, cols), what
    b.close()


@pytest.mark.parametrize("policy", ["trunc", "linear"])
@pytest.mark.parametrize("which", ["folds", "beyond the bound", "switched off"])
def test_fold_admission(which, policy, pairs, monkeypatch):
    monkeypatch.setenv("HX_CHAIN_MULTI", "0")            # one workgroup per pair: the launches that can fold
    flag, tm = (capi.HX_LSE_TRUNC, 2) if policy == "trunc" else (capi.HX_LSE_LINEAR, True)
    if which == "beyond the bound":
        cases = [P.leaf_case("tiny_indel", "unrel", 65, 130), P.leaf_case("tiny_indel", "mut", 70, 66)]
        imgs = [c["img"] for c in cases]
        wants = [P.oracle(c, 0, tm) for c in cases]
    else:
        if which == "switched off":
            monkeypatch.setenv("HX_LINEAR_FOLD", "0")
        ks = [k for k in range(len(pairs[0])) if k % 3 == 0 and COLS[k % len(COLS)] >= 63]      # the protein pairs
        imgs = [pairs[0][k] for k in ks]
        wants = [oracle(pairs, k, tm) for k in ks]
    b = capi.Batch(imgs, flag)
    b.forward()
    assert b.forward_folded() == (which == "folds"), which
    lp_end = b.lp_end()
    for k, want in enumerate(wants):
        what = "%s, pair %d, %s" % (which, k, policy)
        got = b.read_matrix(k, 0)
        assert not np.isnan(got).any(), what
        assert np.array_equal(np.isneginf(want["cells"]), np.isneginf(got)), "%s: -inf pattern" % what
        fin = np.isfinite(got)
        print("%s: max |cell - oracle| %.3g, lpEnd rel. %.3g" % (what, np.max(np.abs(want["cells"][fin] - got[fin]), initial=0.),
                                                                 abs(want["lp_end"] - lp_end[k]) / abs(lp_end[k])))
        assert np.max(np.abs(want["cells"][fin] - got[fin]), initial=0.) < 1e-9, what
        assert abs(want["lp_end"] - lp_end[k]) <= 1e-12 * abs(lp_end[k]), what
    b.close()
