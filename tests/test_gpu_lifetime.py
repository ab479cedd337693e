"""Who frees what: every object of the C ABI gives back, at its destroy call, the device and page-locked allocations its
create call and its calls in between took (csrc/hx_devmem.h).  hx_live_allocations counts them; the tests
read it as differences within a test, because fixtures of other modules may hold objects of their own.

Every assertion is an equality or a strict inequality of two counts.  Every object is destroyed by close() on its wrapper,
never by garbage collection.  Nothing is compared with an oracle here: what the calls compute is the other modules' business.

The shapes are the smallest with two strips (70 x 70).  The progress counters of a launch that deals a pair to several
workgroups (hx_batch::d_multi) are not allocated at this size and no hook of DESIGN 14 changes that for leaf pairs:
HX_CHAIN_MULTI is capped at a quarter of the strips, HX_DAG_MULTI_MIN_STRIPS concerns general profiles only, and HX_FORCE_DAG
is read once per process."""
import ctypes as C

import numpy as np
import pytest

from historian_amd import capi, counts
from oracle import c_oracle
from tests import helpers as H
from tests import sibling_ref as sr
from tests.test_gpu_branch import as_job as branch_job, random_branch
from tests.test_gpu_sibling import as_job as sibling_job
from tests.test_gpu_sumprod import _fixture

pytestmark = pytest.mark.gpu

live = capi.live_allocations


@pytest.fixture(scope="module", autouse=True)
def engine():
    capi.init(0, c_oracle.table())
    yield
    capi.shutdown()


JC_RATE = np.full((1, 4, 4), 1. / 3)        # Jukes-Cantor, one substitution per unit of time
JC_RATE[0][np.arange(4), np.arange(4)] = -1.


def unchanged(call):
    """runs call(); the count afterwards must be the count before"""
    before = live()
    out = call()
    assert live() == before
    return out


def test_pair_fill_batch():
    """two unbanded leaf pairs of two strips and a banded one (so the batch owns step windows), HX_KEEP_BACKWARD"""
    imgs = [H.job_images(f) for f in (H.leaf_case(7, 70, 70), H.leaf_case(8, 70, 70), H.leaf_case(11, 70, 70, band=6))]
    base = live()
    b = capi.Batch(imgs, capi.HX_KEEP_BACKWARD)
    created = live()
    assert created > base

    def fills():
        b.forward()
        b.backward()
        return b.lp_end(), b.lp_start()
    unchanged(fills)                       # (Backward matrices came with the batch; no several-workgroups launch at this size)
    rows_cols = b.layout(0).n_rows + b.layout(0).n_cols
    b.best_trace(cap=rows_cols + 4)
    traced = live()
    assert traced > created                # the path buffers are kept with the batch ...
    unchanged(lambda: b.best_trace(cap=rows_cols + 4))
    unchanged(lambda: b.best_trace(cap=3 * rows_cols))      # ... and a larger cap replaces them
    assert live() == traced
    times = [.1, .2, 1.5, 2.5, 1.2, 2.2]
    u = np.random.default_rng(1).random(4 * (rows_cols + 4))
    unchanged(lambda: b.sample_traces(0, 2, u))
    b.event_counts(0, times)
    counted = live()
    assert counted > traced                # the scratch of the event counts is kept as well
    unchanged(lambda: b.event_counts(2, times))
    unchanged(lambda: b.indel_counts(1, times))
    unchanged(lambda: b.posterior_scan(0, .01, cap=256))
    unchanged(lambda: b.posterior_scan(2, .5, cap=0))
    unchanged(lambda: b.read_cells(0, [(0, 0), (69, 69), (64, 3)], which=1))
    unchanged(lambda: b.read_cells(2, [(5, 5)]))
    unchanged(lambda: b.read_matrix(2, 1))
    lib = capi.load()
    lib.hx_host_alloc.argtypes = [C.c_size_t, C.POINTER(C.c_void_p)]
    lib.hx_host_free.argtypes = [C.c_void_p]
    p = C.c_void_p()
    assert lib.hx_host_alloc(b.layout(1).matrix_doubles * 8, C.byref(p)) == 0      # (the caller's: not counted)

    def async_read():
        assert lib.hx_batch_read_matrix_async(b._h, 1, 0, p) == 0
        assert lib.hx_batch_wait_read(b._h, 1, 0) == 0
    unchanged(async_read)                  # (its event is no allocation)
    assert lib.hx_host_free(p) == 0
    assert live() == counted
    b.close()
    assert live() == base


def test_backward_matrices_allocated_late():
    """without HX_KEEP_BACKWARD the Backward matrices come with the first Backward fill, and go with the batch"""
    base = live()
    b = capi.Batch([H.job_images(H.leaf_case(7, 70, 70))])
    b.forward()
    created = live()
    b.backward()
    assert live() > created
    unchanged(b.backward)
    b.close()
    assert live() == base


def quick_pairs():
    rng = np.random.default_rng(3)
    submat = rng.normal(size=(4, 4))
    scores = [float(v) for v in -rng.random(11)]
    x, y = rng.integers(0, 4, 70), rng.integers(0, 4, 70)
    return [(x, y, 4, submat, scores, None), (y[:40], x[:33], 4, submat, scores, np.arange(-5, 6, dtype=np.int32))]


def quick_jobs(pairs):
    """the C ABI's job array for (x_tok, y_tok, alph_size, submat, scores, diagonals) tuples, and what it points into"""
    keep = [[np.ascontiguousarray(x, dtype=np.int32), np.ascontiguousarray(y, dtype=np.int32), np.ascontiguousarray(sm, dtype=np.float64),
             None if dg is None else np.ascontiguousarray(dg, dtype=np.int32)] for x, y, _, sm, _, dg in pairs]
    arr = (capi.HxQuickJob * len(pairs))()
    i32p = C.POINTER(C.c_int32)
    for j, (x, y, sm, dg), (_, _, a, _, scores, _) in zip(arr, keep, pairs):
        j.x_tok, j.y_tok, j.x_len, j.y_len, j.alph_size = x.ctypes.data_as(i32p), y.ctypes.data_as(i32p), len(x), len(y), a
        j.submat = sm.ctypes.data_as(C.POINTER(C.c_double))
        j.diagonals, j.n_diagonals = (C.cast(None, i32p), 0) if dg is None else (dg.ctypes.data_as(i32p), len(dg))
        for k, v in enumerate(scores):
            j.scores[k] = v
    return arr, keep


def test_guide_alignment_batch():
    """two jobs, one inside a diagonal envelope"""
    base = live()
    qb = capi.QuickBatch(quick_pairs())
    created = live()
    assert created > base

    def use():
        qb.run()
        qb.results()
        return qb.read_matrix(0), qb.read_matrix(1)
    unchanged(use)
    qb.close()
    assert live() == base


def pair_walk_calls(b, best):
    """run, the walks, cells along a path, the dense matrix: nothing of it stays with the batch"""
    before = live()
    b.run()
    b.lp_end()
    if best:
        b.best_paths()
    rng = np.random.default_rng(5)
    words = [rng.integers(0, 2 ** 32, size=b.max_steps() + 8, dtype=np.uint64).astype(np.uint32) for _ in range(b.n)]
    if best:
        b.run(viterbi=False)
    b.sample_paths(words)
    for k in range(b.n):
        b.read_cells(k, [(0, 0, 0), (b.shapes[k][0] - 1, b.shapes[k][1] - 1, 1)])
        b.read_matrix(k)
    assert live() == before


def test_branch_batch():
    """two jobs of two strips, one banded"""
    jobs = [branch_job(random_branch(12, 70, 66)), branch_job(random_branch(15, 70, 70, band=6))]
    base = live()
    b = capi.BranchBatch(jobs)
    assert live() > base
    pair_walk_calls(b, best=True)
    b.close()
    assert live() == base


def test_sibling_batch():
    """two jobs of two strips, one banded"""
    jobs = []
    for seed, band in ((12, None), (16, 4)):
        case = sr.random_case(seed, 70, 66, band=band)
        jobs.append(sibling_job(case, sr.SiblingMatrix(fill=False, **case)))
    base = live()
    b = capi.SiblingBatch(jobs)
    assert live() > base
    pair_walk_calls(b, best=False)
    b.close()
    assert live() == base


def test_resident_history_and_its_branch_batch():
    """five leaves, nine nodes, eight columns: the evaluation at creation, a proposal from lengths, an excluded-neighbour query,
    a larger one (its buffers grow), a branch batch made from the history; the batch outlives nothing here"""
    parent = [5, 5, 6, 6, 8, 7, 7, 8, -1]
    tokens = np.full((8, 9), -1, dtype=np.int8)                    # internal nodes: wildcards
    tokens[:, :5] = np.random.default_rng(2).integers(0, 4, (8, 5))
    tokens[3, 0] = tokens[6, 4] = -2                               # a leaf gapped here and there
    rate = JC_RATE
    lengths = np.linspace(.05, .4, 9)
    ins_prob, log_w = np.full((1, 4), .25), np.zeros(1)
    base = live()
    h = capi.History.from_lengths(parent, ins_prob, log_w, tokens, rate, lengths)
    created = live()
    assert created > base
    unchanged(h.log_like)

    def proposal():
        h.propose_lengths([0, 5], [.2, .3])
        h.log_like(which=1)
        h.reject()
    unchanged(proposal)
    h.excluded_profiles([(5, 0)])
    queried = live()
    assert queried > created               # the query's plan and output and the block offsets stay with the history
    unchanged(lambda: h.excluded_profiles([(5, 0)]))
    unchanged(lambda: h.excluded_profiles([(r, parent[r]) for r in range(8)] + [(parent[r], r) for r in range(8)]))      # ... and grow in place
    log_sub, log_ins = np.log(h.branch_matrix(0)), np.log(ins_prob)
    trans = random_branch(1, 1, 1)[3]
    env = capi.branch_guide_envelope(tokens, parent[1], 1)
    bb = h.branch_batch([(0, log_sub, log_ins, trans, None, None, -1), (1, log_sub, log_ins, trans, env[0], env[1], 2)])
    assert live() > queried
    pair_walk_calls(bb, best=True)
    bb.close()
    assert live() == queried
    h.close()
    assert live() == base


def test_calls_that_keep_nothing():
    """the sum-product, the ancestors and both distance entry points on the reference's smallest fixtures"""
    _, model, tree, gapped = _fixture("testnj.jukescantor.json", "testaligncount.fa", "testaligncount.nh")
    rows = [gapped[n] for n in range(tree.nodes())]
    cc = counts.ColumnCounter(model, tree.parent, tree.branch_length)
    unchanged(lambda: cc.run(counts.tokenize_columns(model.alphabet, rows)))
    unchanged(lambda: counts.AncestorPredictor(model, tree.parent, tree.branch_length).run(counts.tokenize_columns(model.alphabet, rows), want_post=True))
    sub_rate, weight = JC_RATE, [1.]
    tok = np.random.default_rng(4).integers(0, 4, (3, 30)).astype(np.int8)
    unchanged(lambda: capi.distance_matrix(sub_rate, weight, 1., tok, 100))
    cnt = np.random.default_rng(6).integers(0, 5, (2, 4, 4)).astype(np.int32)
    unchanged(lambda: capi.distance_neg_log_like(sub_rate, weight, cnt, np.array([.1, 2.])))


def test_creation_that_fails_leaves_nothing():
    """a pair-fill batch whose second job has a null profile array, a guide-alignment batch whose second job has a token
    outside its alphabet: today's error codes, a null handle, and the count where it was"""
    lib = capi.load()
    imgs = [H.job_images(H.leaf_case(7, 70, 70)), H.job_images(H.leaf_case(8, 70, 70))]
    jobs = capi.make_jobs(imgs)
    broken = capi.HxProfile.from_buffer_copy(imgs[1][0].struct)
    broken.is_null = C.cast(None, C.POINTER(C.c_uint8))
    jobs[1].x = C.pointer(broken)
    base = live()
    handle = C.c_void_p(1)
    assert lib.hx_batch_create(jobs, 2, capi.HX_KEEP_BACKWARD | capi.HX_LSE_EXACT, C.byref(handle)) == capi.HX_ERR_INVALID_ARG
    assert lib.hx_last_error() == b"null profile arrays"
    assert handle.value is None and live() == base

    pairs = quick_pairs()
    pairs[1] = (np.array([0, 1, 4, 2]),) + pairs[1][1:]
    arr, keep = quick_jobs(pairs)
    handle = C.c_void_p(1)
    assert lib.hx_quick_batch_create(arr, 2, C.byref(handle)) == capi.HX_ERR_RANGE
    assert lib.hx_last_error() == b"job 1: x token 4 out of range"
    assert handle.value is None and live() == base
