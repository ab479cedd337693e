"""Row N4's eleven-state lattice on the device: the sibling-pair parent-proposal DP (hx_sibling.hip, C ABI hx_sibling_batch_*)
against tests/sibling_ref.py - Sampler::SiblingMatrix, reference src/sampler.cpp:1185-1342.  Every cell of every state plane
and lpEnd compared as uint64: the kernel applies the reference's table log_sum_exp in the reference's order.  The restatement
is pinned by enumeration (tests/test_oracle_sibling.py), not by a reference fixture."""
import random
import time

import numpy as np
import pytest

from historian_amd import capi
from oracle import c_oracle
from tests import helpers as H
from tests import sibling_ref as sr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def engine():
    capi.init(0, c_oracle.table())
    yield
    capi.shutdown()


def as_job(case, m):
    C, A = len(case["log_root"]), len(case["log_root"][0])
    return (np.array(case["l_sub"], dtype=float).reshape(-1, C, A), np.array(case["r_sub"], dtype=float).reshape(-1, C, A),
            np.array(case["log_root"], dtype=float), np.array(case["l_emit"], dtype=float), np.array(case["r_emit"], dtype=float),
            m.T, case["l_env"], case["r_env"], case["max_dist"])


def dense(m):
    out = np.full((m.x_size, m.y_size, sr.N_STATES), -np.inf)
    for (i, j), c in m.cells.items():
        out[i, j] = c
    return out


# (seed, left, right, components, alphabet, band, one-hot columns, envelope coordinates non-decreasing)
CASES = [(11, 5, 7, 1, 4, None, False, True), (12, 70, 66, 1, 4, None, False, True), (13, 150, 70, 4, 4, None, False, True),
         (14, 64, 65, 1, 20, None, True, True), (15, 65, 200, 1, 4, 3, False, False), (16, 90, 140, 1, 4, 0, False, True),
         (17, 1, 1, 1, 4, None, False, True), (18, 0, 3, 1, 4, None, False, True), (19, 3, 0, 4, 20, 0, True, True),
         (20, 0, 0, 1, 4, None, False, True), (21, 150, 150, 1, 20, 20, True, False), (22, 63, 129, 4, 4, 3, True, True),
         (23, 200, 130, 1, 4, 20, False, True),
         # envelope coordinates with long plateaus (H.with_plateaus): 100 rows, 90 columns, 70 rows directly followed by 80 columns
         (24, 200, 110, 1, 4, 4, False, True, ("x", 50, 100)), (25, 120, 200, 1, 4, 3, True, True, ("y", 70, 90)),
         (26, 190, 200, 1, 4, 5, False, True, ("xy", 60, 70, 80))]


def build(c, fill=True):
    seed, nx, ny, C, A, band, one_hot, sorted_env = c[:8]
    case = sr.random_case(seed, nx, ny, C=C, A=A, band=band, one_hot=one_hot, sorted_env=sorted_env)
    if len(c) > 8:
        case["l_env"], case["r_env"] = [[int(v) for v in e] for e in H.with_plateaus(case["l_env"], case["r_env"], c[8])]
    return case, sr.SiblingMatrix(fill=fill, **case)


@pytest.fixture(scope="module")
def mixed():
    built = [build(c) for c in CASES]
    b = capi.SiblingBatch([as_job(case, m) for case, m in built])
    b.run()
    yield built, b
    b.close()


def test_sibling_matrices_bit_for_bit(mixed):
    built, b = mixed
    lp = b.lp_end()
    for k, (case, want) in enumerate(built):
        got = b.read_matrix(k)
        for s, name in enumerate(capi.SiblingBatch.STATES):
            H.assert_same_bits(got[:, :, s], dense(want)[:, :, s], "job %d plane %s" % (k, name))
        H.assert_same_bits([lp[k]], [want.lp_end], "job %d lpEnd" % k)
    assert b.total_cells() == sum((c[1] + 1) * (c[2] + 1) for c in CASES)
    fill_ms, step_ms = b.kernel_ms()
    assert 0 < fill_ms <= step_ms


def test_outside_the_envelope_is_minus_infinity_and_runs_repeat(mixed):
    built, b = mixed
    first = [b.read_matrix(k) for k in range(b.n)]
    lp_first = b.lp_end().copy()
    cut = 0
    for (case, m), got in zip(built, first):
        for i in range(m.x_size):
            for j in range(m.y_size):
                if not m.in_envelope(i, j):
                    cut += 1
                    assert np.all(np.isneginf(got[i, j])), (i, j)
    assert cut > 1000
    b.run()
    H.assert_same_bits(b.lp_end(), lp_first, "lpEnd of a second run")
    for k in range(b.n):
        H.assert_same_bits(b.read_matrix(k), first[k], "job %d of a second run" % k)


@pytest.mark.parametrize("waves", [1, 3, 16])
def test_strips_dealt_to_any_number_of_wavefronts(monkeypatch, waves):
    monkeypatch.setenv("HX_SIBLING_WAVES", str(waves))
    built = [build(c) for c in [(31, 300, 130, 1, 4, 5, False, False), (32, 257, 90, 1, 4, None, True, True), (33, 129, 64, 4, 4, 0, True, True)] + CASES[-3:]]
    b = capi.SiblingBatch([as_job(case, m) for case, m in built])
    b.run()
    lp = b.lp_end()
    for k, (case, want) in enumerate(built):
        H.assert_same_bits(b.read_matrix(k), dense(want), "job %d cells, %d wavefronts" % (k, waves))
        H.assert_same_bits([lp[k]], [want.lp_end], "job %d lpEnd" % k)
    b.close()


@pytest.fixture(scope="module")
def thousand():
    # the Python restatement of a million cells: 11 s of wall time on the GPU host (about 30 s on a slow one), once per module
    out = {}
    for band in (None, 20):
        t0 = time.time()
        case, m = build((41, 1000, 1000, 1, 4, band, False, True))
        print("restatement of 1000 x 1000, band %s: %.0f s" % (band, time.time() - t0))
        out[band] = (case, m)
    return out


@pytest.mark.parametrize("band", [None, 20])
def test_a_thousand_by_a_thousand(thousand, band):
    case, want = thousand[band]
    b = capi.SiblingBatch([as_job(case, want)])
    b.run()
    H.assert_same_bits(b.lp_end(), [want.lp_end], "lpEnd")
    got = b.read_matrix(0)
    rng = random.Random(5)
    inside = sorted(want.cells)
    picks = [inside[rng.randrange(len(inside))] for _ in range(12000)] + [(0, 0), (1000, 1000), (0, 1000), (1000, 0), (64, 64), (63, 1000)]
    for i, j in picks:
        H.assert_same_bits(got[i, j], np.array(want.cells[(i, j)]), "cell (%d, %d)" % (i, j))
    assert len(set(picks)) >= 10000
    if band is not None:
        for _ in range(2000):
            i, j = rng.randrange(1001), rng.randrange(1001)
            if not want.in_envelope(i, j):
                assert np.all(np.isneginf(got[i, j]))
    b.close()


def test_a_right_child_too_long_for_lds():
    # above 8192 columns the right child's side of a step (rEmit, envelope coordinate) is read from memory inside the step:
    # k_pair_fill<SiblingCell, false>, and k_pair_fill<BranchCell<*>, false> of the three-state lattice that shares the sweep
    built = [build((61, 70, 8300, 1, 4, None, False, True)), build((62, 70, 8250, 1, 4, 5, False, True))]
    b = capi.SiblingBatch([as_job(case, m) for case, m in built])
    b.run()
    lp = b.lp_end()
    for k, (case, want) in enumerate(built):
        H.assert_same_bits(b.read_matrix(k), dense(want), "job %d cells" % k)
        H.assert_same_bits([lp[k]], [want.lp_end], "job %d lpEnd" % k)
    b.close()
    from oracle import branch_oracle as bo
    from tests.test_gpu_branch import as_job as branch_job, dense as branch_dense, random_branch
    case = random_branch(63, 70, 8300, 1, 4, 4, False)
    x, ysub, yemit, T, xe, ye, md = case
    bb = capi.BranchBatch([branch_job(case)])
    for viterbi in (True, False):
        bb.run(viterbi=viterbi)
        want = bo.BranchMatrix(x, ysub, yemit, T, list(xe), list(ye), md, viterbi=viterbi)
        H.assert_same_bits(bb.read_matrix(0), branch_dense(want), "branch cells (%s)" % ("viterbi" if viterbi else "forward"))
        H.assert_same_bits(bb.lp_end(), [want.lp_end], "branch lpEnd")
    bb.close()


def test_refused_arguments():
    case, m = build((51, 4, 4, 1, 4, None, False, True))
    job = as_job(case, m)
    lib = capi.load()
    import ctypes as C
    h = C.c_void_p()
    assert lib.hx_sibling_batch_create(None, 1, C.byref(h)) == -1                 # HX_ERR_INVALID_ARG, as hx_branch_batch_create
    with pytest.raises(capi.HxError) as e:
        capi.SiblingBatch([])
    assert e.value.code == -1
    b = capi.SiblingBatch([job])
    arr = b._jobs
    b.close()
    for field, value in (("l_len", -1), ("components", 0)):
        bad = type(arr[0])()
        C.memmove(C.byref(bad), C.byref(arr[0]), C.sizeof(bad))
        setattr(bad, field, value)
        assert lib.hx_sibling_batch_create(C.byref(bad), 1, C.byref(h)) == -1, field
    with pytest.raises(capi.HxError) as e:
        capi.SiblingBatch([job[:6] + (None, None, 3)])                             # a band without envelope coordinates
    assert e.value.code == -1
    b = capi.SiblingBatch([job])
    with pytest.raises(capi.HxError):
        b.lp_end()                                                                 # before run
    b.run()
    for k in (-1, 1):
        with pytest.raises(capi.HxError) as e:
            b.read_matrix(k)
        assert e.value.code == -8                                                  # HX_ERR_RANGE
    b.close()
