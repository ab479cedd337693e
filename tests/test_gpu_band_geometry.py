"""Banded fills on the envelopes real guide alignments produce (tests/band_geometry_cases.py): every planner branch and
every kernel that consumes its plans, on long gap runs, leading and trailing runs, blocks without a match, runs across rows
63 | 64 and 127 | 128, y runs after rows = 0 .. 3 (mod 4), a band wider than both sequences, protein and mixture models.
The yardsticks are the ones of tests/test_gpu_parity.py and tests/test_gpu_trunc.py, unchanged: bit for bit against
oracle_fill.c in the exact policy; 1e-9 on cells and 1e-12 on lpEnd against its libm arithmetic for the scaled-probability
policies; 1e-7 / 1e-9 of the exact fill for the fast table.

Dispatch observed on an MI355X (test_dispatch_reaches_every_path asserts the four paths, this is the whole table):
class = Forward kernel class of hx_batch_job_kernel, sweep = Backward in the rotating-row sweep, w32 = admitted to two pairs
per wavefront (a one-pair HX_LSE_TRUNC batch under HX_BAND2=1 reports shared_wavefront_pairs() == 1).

    family                 lx, events, band                                   class  sweep  w32
    long_y_run             150, {40: +90}, 4                                    2     yes   yes
    long_x_run             200, {60: -100}, 4                                   2     yes   yes
    staircase              260, {30: +40, 80: -50, 150: +70, 200: -30}, 6       2     yes   yes
    leading_y_run          140, {0: +80}, 3                                     2     yes   yes
    band0_runs             130, {50: +20, 90: -25}, 0                           2     yes   yes
    no_match               70, {0: +60, 1: -69}, 5                              1     no    no
    trailing_x_run         180, {100: -80}, 4                                   2     yes   yes
    trailing_y_run         120, {120: +85}, 3                                   2     yes   yes
    unaligned_70_80        200, {60: -70, 130: +80}, 5                          1     no    no
    unaligned_40_40        200, {80: -40, 120: +40}, 5                          2     yes   no
    x_runs_across_64_128   260, {30: -70, 120: -70}, 4                          2     yes   yes
    y_runs_at_64_128       170, {63: +40, 127: +35}, 3                          2     yes   yes
    y_runs_mod4            200, eight runs of 8 to 14, 2                        2     yes   yes
    band_over_both         80, {20: +10, 40: -8}, 400                           1     no    no
    protein                150, {40: +50, 100: -40}, 5                          2     yes   yes
    two_components         140, {30: -45, 90: +60}, 4                           2     yes   yes

Class 1 is the strip pipeline (hx_chain.hip / hx_linear.hip, BANDED): rows i and i + 63 of those three pairs are alive together
(62 or more columns shared by 63 rows and more), which the rotating-row sweep's 64-lane ring cannot hold.  The 40 + 40 block
passes that ring and fails the 32-row one of hx_band2.hip, so a class that holds it runs one pair per wavefront.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from historian_amd import capi
from oracle import c_oracle, trace_oracle
from tests import band_geometry_cases as G
from tests import helpers as H
from tests.test_gpu_parity import run_and_check
from tests.test_gpu_trunc import check_forward

pytestmark = pytest.mark.gpu

NAMES = list(G.FAMILIES)
STORAGE = (0, capi.HX_SPARSE_ENVELOPE, capi.HX_BAND_COMPRESSED)


@pytest.fixture(scope="module", autouse=True)
def engine():
    capi.init(0, c_oracle.table())
    yield
    capi.shutdown()


def cases(names=NAMES):
    return [G.leaf(n)[0] for n in names]


def images(names=NAMES):
    return [G.leaf(n)[1] for n in names]


@functools.lru_cache(maxsize=None)
def want(name, which, true_math=0):
    """the oracle's fill of a family (which: 0 Forward, 1 Backward), computed once and left unchanged"""
    x, y, hmm, md = G.leaf(name)[1]
    w = (c_oracle.backward if which else c_oracle.forward)(x, y, hmm, md, true_math=true_math)
    w["cells"].setflags(write=False)
    return w


# ---------------------------------------------------------------------------------------------------------------------------
# exact policy
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hook", ["default", "HX_BAND_PPW=-3", "HX_BAND_PPW=2", "HX_BAND_BWD_OLD=1", "HX_BAND_NO_LINE_GROUPS=1",
                                  "HX_FORCE_GENERIC"])
def test_exact_policy_bit_for_bit_under_every_dispatch(hook, monkeypatch):
    flags = 0
    if hook == "HX_FORCE_GENERIC":
        flags = capi.HX_FORCE_GENERIC
    elif hook != "default":
        monkeypatch.setenv(*hook.split("="))
    run_and_check(cases(), backward=True, flags=flags)      # Forward and Backward cells, lpEnd, lpStart: the oracle's bits
    if hook in ("default", "HX_BAND_NO_LINE_GROUPS=1"):
        # said once more in words: dense planes are -inf outside the envelope, in both matrices
        b = capi.Batch(images(), capi.HX_KEEP_BACKWARD)
        b.forward()
        b.backward()
        for k, name in enumerate(NAMES):
            for which in (0, 1):
                assert np.all(np.isneginf(b.read_matrix(k, which)[~G.mask(name)])), (name, which)
        b.close()


@pytest.mark.parametrize("hook", ["default", "HX_BAND_PPW=-3", "HX_BAND_PPW=2", "HX_BAND_BWD_OLD=1", "HX_BAND_NO_LINE_GROUPS=1"])
@pytest.mark.parametrize("storage", [capi.HX_SPARSE_ENVELOPE, capi.HX_BAND_COMPRESSED])
def test_exact_policy_sparse_and_compressed_planes_inside_the_envelope(storage, hook, monkeypatch):
    if hook != "default":
        monkeypatch.setenv(*hook.split("="))
    backward = storage != capi.HX_BAND_COMPRESSED          # (compressed batches are Forward only)
    b = capi.Batch(images(), storage | (capi.HX_KEEP_BACKWARD if backward else 0))
    b.forward()
    if backward:
        b.backward()
    for k, name in enumerate(NAMES):
        env = G.mask(name)
        H.assert_same_bits(b.read_matrix(k, 0)[env], want(name, 0)["cells"][env], "%s: Forward, in-envelope cells" % name)
        H.assert_same_bits([b.lp_end()[k]], [want(name, 0)["lp_end"]], "%s: lpEnd" % name)
        if backward:
            H.assert_same_bits(b.read_matrix(k, 1)[env], want(name, 1)["cells"][env], "%s: Backward, in-envelope cells" % name)
            H.assert_same_bits([b.lp_start()[k]], [want(name, 1)["lp_start"]], "%s: lpStart" % name)
    b.close()


# ---------------------------------------------------------------------------------------------------------------------------
# fast, truncating and scaled-probability policies, three storage modes
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGE)
def test_fast_policy_stays_within_tolerance_of_exact(storage):
    # the yardstick of test_fast_mode_stays_within_tolerance_of_exact (sparse / compressed planes: inside the envelope)
    backward = storage != capi.HX_BAND_COMPRESSED
    imgs = images()
    be = capi.Batch(imgs, capi.HX_KEEP_BACKWARD)
    bf = capi.Batch(imgs, capi.HX_LSE_FAST | storage | (capi.HX_KEEP_BACKWARD if backward else 0))
    be.forward()
    be.backward()
    bf.forward()
    if backward:
        bf.backward()
    le, lf, se = be.lp_end(), bf.lp_end(), be.lp_start()
    sf = bf.lp_start() if backward else None
    for k, name in enumerate(NAMES):
        sel = G.mask(name) if storage else np.ones(G.mask(name).shape, dtype=bool)
        for which in ((0, 1) if backward else (0,)):
            me, mf = be.read_matrix(k, which)[sel], bf.read_matrix(k, which)[sel]
            assert np.array_equal(np.isneginf(me), np.isneginf(mf)), (name, which)
            fin = np.isfinite(me)
            assert np.max(np.abs(me[fin] - mf[fin]), initial=0.) < 1e-7, (name, which)
        assert abs(le[k] - lf[k]) <= 1e-9 * abs(le[k]), name
        if backward:
            assert abs(se[k] - sf[k]) <= 1e-9 * abs(se[k]), name
    be.close()
    bf.close()


@pytest.mark.parametrize("ppw", [0, -3, 2])
def test_truncating_policy(ppw, monkeypatch):
    # check_forward and the Backward block of tests/test_gpu_trunc.py::test_banded_leaf_pairs_in_the_rotating_row_sweep
    if ppw:
        monkeypatch.setenv("HX_BAND_PPW", str(ppw))
    cs = cases()
    for flags in STORAGE:
        bt, imgs = check_forward(cs, flags, env_only=flags != 0)
        be = capi.Batch(imgs, flags & ~capi.HX_BAND_COMPRESSED)
        be.forward()
        assert bt.best_trace() == be.best_trace()
        if flags != capi.HX_BAND_COMPRESSED:
            bt.backward()
            st = bt.lp_start()
            for k, name in enumerate(NAMES):
                w = want(name, 1, 2)
                got = bt.read_matrix(k, 1)
                inside = np.isfinite(w["cells"])
                assert np.max(np.abs(w["cells"][inside] - got[inside]), initial=0.) < 1e-9, "%s backward" % name
                if not flags:
                    assert np.array_equal(np.isneginf(w["cells"]), np.isneginf(got)), name
                assert abs(w["lp_start"] - st[k]) <= 1e-12 * abs(st[k]), name
        be.close()
        bt.close()


@pytest.mark.parametrize("ppw", [0, 6])
def test_scaled_probability_policy(ppw, monkeypatch):
    # the assertions of tests/test_gpu_parity.py::test_linear_mode_on_banded_leaf_pairs
    if ppw:
        monkeypatch.setenv("HX_LINEAR_PPW", str(ppw))
    imgs = images()
    for flags in STORAGE:
        be = capi.Batch(imgs, flags & ~capi.HX_BAND_COMPRESSED)
        bf = capi.Batch(imgs, capi.HX_LSE_LINEAR | flags)
        be.forward()
        bf.forward()
        le, lf = be.lp_end(), bf.lp_end()
        for k, name in enumerate(NAMES):
            w = want(name, 0, 1)
            mf = bf.read_matrix(k, 0)
            inside = np.isfinite(w["cells"])
            sel = G.mask(name) if flags else np.ones(mf.shape[:2], dtype=bool)
            assert not np.isnan(mf[sel]).any(), name
            assert np.array_equal(np.isneginf(w["cells"][sel]), np.isneginf(mf[sel])), "%s: -inf pattern" % name
            assert np.max(np.abs(w["cells"][inside] - mf[inside]), initial=0.) < 1e-9, name
            assert abs(w["lp_end"] - lf[k]) <= 1e-12 * abs(lf[k]), name
            assert abs(le[k] - lf[k]) <= 1e-5 * abs(le[k]), name
        if flags != capi.HX_BAND_COMPRESSED:
            be.backward()
            bf.backward()
            se, sf = be.lp_start(), bf.lp_start()
            for k, name in enumerate(NAMES):
                w = want(name, 1, 1)
                mb = bf.read_matrix(k, 1)
                inside = np.isfinite(w["cells"])
                if not flags:
                    assert np.array_equal(np.isneginf(w["cells"]), np.isneginf(mb)), "%s: backward -inf pattern" % name
                assert np.max(np.abs(w["cells"][inside] - mb[inside]), initial=0.) < 1e-9, "%s backward" % name
                assert abs(w["lp_start"] - sf[k]) <= 1e-12 * abs(sf[k]), name
                assert abs(se[k] - sf[k]) <= 1e-5 * abs(se[k]), name
                assert abs(sf[k] - lf[k]) <= 1e-11 * abs(lf[k]), name      # Forward == Backward to rounding
        else:
            bd = capi.Batch(imgs, capi.HX_LSE_LINEAR)
            bd.forward()
            assert bf.best_trace() == bd.best_trace()
            bd.close()
        be.close()
        bf.close()


# ---------------------------------------------------------------------------------------------------------------------------
# dispatch
# ---------------------------------------------------------------------------------------------------------------------------
def dispatch_table(monkeypatch):
    """name -> (Forward class, Backward in the sweep, admitted to two pairs per wavefront)"""
    b = capi.Batch(images(), capi.HX_KEEP_BACKWARD)
    kern = [b.job_kernel(k) for k in range(len(NAMES))]
    b.close()
    monkeypatch.setenv("HX_BAND2", "1")
    table = {}
    for name, (cls, sweep) in zip(NAMES, kern):
        b = capi.Batch([G.leaf(name)[1]], capi.HX_LSE_TRUNC | capi.HX_KEEP_BACKWARD)
        assert b.job_kernel(0) == (cls, sweep), name           # (the class is the pair's own, whatever the policy)
        table[name] = (cls, sweep, b.shared_wavefront_pairs() == 1)
        b.close()
    monkeypatch.delenv("HX_BAND2")
    return table


def test_dispatch_reaches_every_path(monkeypatch):
    table = dispatch_table(monkeypatch)
    print("\n".join("%-22s class %d  sweep %d  w32 %d" % ((n,) + tuple(int(v) for v in t)) for n, t in table.items()))
    assert all(cls in (1, 2) for cls, _, _ in table.values()), table
    assert any(cls == 2 and sweep for cls, sweep, _ in table.values()), table         # the rotating-row sweep, both fills
    assert any(cls == 1 for cls, _, _ in table.values()), table                       # refused: the strip pipeline
    assert all(not sweep and not w32 for cls, sweep, w32 in table.values() if cls == 1), table
    assert any(cls == 2 and w32 for cls, _, w32 in table.values()), table             # two pairs per wavefront
    assert any(cls == 2 and not w32 for cls, _, w32 in table.values()), table         # the 64-row ring but not the 32-row one
    # what the planner's conditions say about the two blocks without a match
    assert table["unaligned_70_80"][0] == 1
    assert table["unaligned_40_40"] == (2, True, False)


@pytest.mark.parametrize("nw", [1, 2, 4])
def test_two_pairs_per_wavefront(nw, monkeypatch):
    # the assertions of tests/test_gpu_trunc.py::test_two_banded_pairs_per_wavefront.  A class shares wavefronts only when
    # every pair of it is admitted: the batch of all families holds refused geometries and must not, the batch of the
    # admitted ones must - and gives the bits of one pair per wavefront either way.
    table = dispatch_table(monkeypatch)
    admitted = [n for n in NAMES if table[n][2]]
    monkeypatch.setenv("HX_BAND2_NW", str(nw))
    for names in (NAMES, admitted):
        imgs = images(names)
        in_class = sum(1 for n in names if table[n][0] == 2)
        for policy, tm in ((capi.HX_LSE_TRUNC, 2), (capi.HX_LSE_LINEAR, 1)):
            for flags in STORAGE:
                monkeypatch.setenv("HX_BAND2", "1")
                bt = capi.Batch(imgs, policy | flags)
                assert bt.shared_wavefront_pairs() == (len(names) if names is admitted else 0), (in_class, names)
                bt.forward()
                lt = bt.lp_end()
                for k, name in enumerate(names):
                    w = want(name, 0, tm)
                    got = bt.read_matrix(k, 0)
                    sel = G.mask(name) if flags else np.ones(got.shape[:2], dtype=bool)
                    assert not np.isnan(got[sel]).any(), name
                    assert np.array_equal(np.isneginf(w["cells"][sel]), np.isneginf(got[sel])), "%s: -inf pattern" % name
                    fin = np.isfinite(w["cells"]) & sel[:, :, None]
                    assert np.max(np.abs(w["cells"][fin] - got[fin]), initial=0.) < 1e-9, name
                    assert abs(w["lp_end"] - lt[k]) <= 1e-12 * abs(lt[k]), name
                if flags != capi.HX_BAND_COMPRESSED:
                    bt.backward()
                    st = bt.lp_start()
                    for k, name in enumerate(names):
                        w = want(name, 1, tm)
                        got = bt.read_matrix(k, 1)
                        inside = np.isfinite(w["cells"])
                        assert np.max(np.abs(w["cells"][inside] - got[inside]), initial=0.) < 1e-9, "%s backward" % name
                        if not flags:
                            assert np.array_equal(np.isneginf(w["cells"]), np.isneginf(got)), "%s backward -inf pattern" % name
                        assert abs(w["lp_start"] - st[k]) <= 1e-12 * abs(st[k]), name
                monkeypatch.setenv("HX_BAND2", "0")
                b1 = capi.Batch(imgs, policy | flags)
                assert b1.shared_wavefront_pairs() == 0
                b1.forward()
                for k, name in enumerate(names):
                    sel = G.mask(name) if flags else np.ones(G.mask(name).shape, dtype=bool)
                    H.assert_same_bits(bt.read_matrix(k, 0)[sel], b1.read_matrix(k, 0)[sel], "two pairs per wavefront vs one, %s" % name)
                assert bt.best_trace() == b1.best_trace()
                b1.close()
                bt.close()


# ---------------------------------------------------------------------------------------------------------------------------
# readers
# ---------------------------------------------------------------------------------------------------------------------------
def test_best_paths_on_every_geometry():
    imgs = images()
    be = capi.Batch(imgs)
    be.forward()
    paths = be.best_trace()
    be.close()
    for name in ("staircase", "unaligned_70_80"):
        k = NAMES.index(name)
        x, y, hmm, md = imgs[k]
        assert paths[k] == trace_oracle.best_trace(x, y, hmm, md, want(name, 0)), name
    for flags in (capi.HX_SPARSE_ENVELOPE, capi.HX_BAND_COMPRESSED, capi.HX_FORCE_GENERIC, capi.HX_LSE_TRUNC,
                  capi.HX_LSE_TRUNC | capi.HX_SPARSE_ENVELOPE, capi.HX_LSE_TRUNC | capi.HX_BAND_COMPRESSED):
        b = capi.Batch(imgs, flags)
        b.forward()
        assert b.best_trace() == paths, flags
        b.close()


@pytest.mark.parametrize("storage", STORAGE)
def test_gathered_cells_at_the_corners_of_every_run(storage):
    backward = storage != capi.HX_BAND_COMPRESSED
    b = capi.Batch(images(), storage | (capi.HX_KEEP_BACKWARD if backward else 0))
    b.forward()
    if backward:
        b.backward()
    for k, name in enumerate(NAMES):
        ij = G.run_corners(name)
        inside = G.mask(name)[ij[:, 0], ij[:, 1]]
        if name not in G.WHOLE:
            assert inside.any() and (~inside).any(), name
        for which in ((0, 1) if backward else (0,)):
            got = b.read_cells(k, ij, which)
            assert np.all(np.isneginf(got[~inside])), (name, which)
            H.assert_same_bits(got[inside], b.read_matrix(k, which)[ij[inside, 0], ij[inside, 1]], "%s: gathered cells of matrix %d" % (name, which))
            if which == 0:
                H.assert_same_bits(got[inside], want(name, 0)["cells"][ij[inside, 0], ij[inside, 1]], "%s: gathered cells vs the oracle" % name)
    b.close()


_CELL = np.dtype([("x", "<i4"), ("y", "<i4"), ("s", "<i4"), ("pad", "<i4"), ("lpp", "<f8")])


def scan(b, job, p, cap):
    """hx_batch_posterior_scan -> (n_out, the cap entries of the output buffer as a record array; it starts as all -1 bytes)"""
    out = (capi.HxCell * max(cap, 1))()
    C.memset(out, 0xFF, C.sizeof(out))
    n = C.c_int64(-1)
    capi._check(capi.load().hx_batch_posterior_scan(b._h, job, p, out if cap else None, cap, C.byref(n)))
    return n.value, np.frombuffer(out, dtype=_CELL)[:cap].copy()


def expected_scan(b, job, env, p):
    """(b + f) - lpEnd >= log(p) over the in-envelope cells, from the matrices as read back: records sorted by (x, y, s)"""
    f, bw, lp = b.read_matrix(job, 0), b.read_matrix(job, 1), b.lp_end()[job]
    with np.errstate(invalid="ignore"):
        lpp = (bw + f) - lp
    keep = (lpp >= (-np.inf if p == 0 else math.log(p))) & env[:, :, None]
    i, j, s = np.nonzero(keep)
    rec = np.zeros(len(i), dtype=_CELL)
    rec["x"], rec["y"], rec["s"], rec["lpp"] = i, j, s, lpp[keep]
    return rec


def check_scan(b, job, env, what):
    for p in (.5, 1e-3, 0.):
        exp = expected_scan(b, job, env, p)
        n, got = scan(b, job, p, len(exp) + 8)
        assert n == len(exp), (what, p, n, len(exp))
        got, spare = got[:n], got[n:]
        assert np.all(spare["x"] == -1), (what, p)                       # nothing written past the count
        got = got[np.lexsort((got["s"], got["y"], got["x"]))]
        assert np.array_equal(got[["x", "y", "s"]], exp[["x", "y", "s"]]), (what, p)
        assert np.all(got["pad"] == 0)
        H.assert_same_bits(got["lpp"], exp["lpp"], "%s, p = %g: log_post_prob" % (what, p))
        if p == 0.:
            assert n == 5 * int(env.sum()), what
        # count only, and a buffer smaller than the count: n_out is still the total, exactly cap entries are written
        assert scan(b, job, p, 0)[0] == n
        if n >= 2:
            cap = n // 2
            out = (capi.HxCell * (cap + 3))()       # (room for three more than the call is told of)
            C.memset(out, 0xFF, C.sizeof(out))
            nn = C.c_int64(-1)
            capi._check(capi.load().hx_batch_posterior_scan(b._h, job, p, out, cap, C.byref(nn)))
            part = np.frombuffer(out, dtype=_CELL)
            assert nn.value == n, (what, p)
            assert np.all(part["x"][cap:] == -1) and np.all(part["x"][:cap] >= 0), (what, p)
            # ... distinct entries of the expected set, with their values
            part = part[:cap][np.lexsort((part["s"][:cap], part["y"][:cap], part["x"][:cap]))]
            key = lambda r: (r["x"].astype(np.int64) * 1024 + r["y"]) * 8 + r["s"]
            assert len(np.unique(key(part))) == cap, (what, p)
            at = np.searchsorted(key(exp), key(part))
            assert np.all(at < len(exp)) and np.array_equal(key(exp)[np.minimum(at, len(exp) - 1)], key(part)), (what, p)
            H.assert_same_bits(part["lpp"], exp["lpp"][at], "%s, p = %g: log_post_prob of a truncated scan" % (what, p))


def test_posterior_scan_on_every_geometry():
    b = capi.Batch(images(), capi.HX_KEEP_BACKWARD)
    b.forward()
    b.backward()
    for k, name in enumerate(NAMES):
        check_scan(b, k, G.mask(name), name)
    b.close()


def test_posterior_scan_beyond_one_round_of_the_grid_in_a_mixed_batch():
    # 521 x 511 cells > 262 144 threads: the grid-stride loop takes a second round; the pair is job 2 of a batch that mixes
    # kernel classes (a profile pair, an unbanded and two banded leaf pairs)
    big = H.leaf_case(81, 520, 510)
    d = G.dag("dag_three_strips", 6, 4)[0]
    fs = [G.leaf("long_y_run")[0], d, big, G.leaf("staircase")[0]]
    b = capi.Batch([H.job_images(f) for f in fs], capi.HX_KEEP_BACKWARD)
    assert b.layout(2).n_rows * b.layout(2).n_cols > 262144
    b.forward()
    b.backward()
    for k in (2, 1, 3):
        check_scan(b, k, H.envelope_mask(fs[k]) if k != 2 else np.ones((521, 511), dtype=bool), "job %d" % k)
    b.close()


def test_posterior_scan_in_the_interleaved_layout_of_the_truncating_policy():
    # unbanded leaf pairs of the scaled-probability policies keep the five states of a step pair adjacent (hx_layout.block_stride)
    fs = [G.leaf("band0_runs")[0], H.leaf_case(306, 100, 130), H.leaf_case(305, 63, 64, alphabet=G.AA, jc=False, tl=.3, tr=.2)]
    b = capi.Batch([H.job_images(f) for f in fs], capi.HX_LSE_TRUNC | capi.HX_KEEP_BACKWARD)
    assert b.layout(1).block_stride != b.layout(0).block_stride
    b.forward()
    b.backward()
    for k, f in enumerate(fs):
        check_scan(b, k, H.envelope_mask(f), "job %d" % k)
    b.close()


# ---------------------------------------------------------------------------------------------------------------------------
# chain and general profiles
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", list(G.DAG_FAMILIES))
def test_profile_pairs_banded_round_a_four_leaf_history(size):
    # the best paths alone with their null states: chains (class 6); without: leaf-like chains whose transitions carry
    # probabilities (class 4); four sampled paths: general profiles (class 8) - all banded
    kinds = ((0, True), (0, False), (4, False))
    fs = [G.dag(size, band, samples, keep_all)[0] for samples, keep_all in kinds for band in (0, 2, 6)]
    imgs = [H.job_images(f) for f in fs]
    be = capi.Batch(imgs, capi.HX_KEEP_BACKWARD)
    classes = [be.job_kernel(k)[0] for k in range(len(fs))]
    assert classes == [6] * 3 + [4] * 3 + [8] * 3, classes
    be.close()
    run_and_check(fs, backward=True)                       # exact: Forward and Backward bit for bit
    # fast: the tolerances of test_fast_mode_stays_within_tolerance_of_exact
    be = capi.Batch(imgs)
    bf = capi.Batch(imgs, capi.HX_LSE_FAST)
    for b in (be, bf):
        b.forward()
        b.backward()
    le, lf, se, sf = be.lp_end(), bf.lp_end(), be.lp_start(), bf.lp_start()
    for k in range(len(fs)):
        for which in (0, 1):
            me, mf = be.read_matrix(k, which), bf.read_matrix(k, which)
            assert np.array_equal(np.isneginf(me), np.isneginf(mf))
            fin = np.isfinite(me)
            assert np.max(np.abs(me[fin] - mf[fin]), initial=0.) < 1e-7
        assert np.isfinite(le[k]) and np.isfinite(se[k])
        assert abs(le[k] - lf[k]) <= 1e-9 * abs(le[k])
        assert abs(se[k] - sf[k]) <= 1e-9 * abs(se[k])
    be.close()
    bf.close()
