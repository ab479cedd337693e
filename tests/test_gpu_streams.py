"""The stream contract of the C ABI (include/historian_hip.h, "Streams").

Every launch entry point takes a stream, and behind it the library keeps a side stream and a copy stream per device, per-batch
events, a remembered `last_stream`, state records that are built on first demand and progress counters zeroed with
hipMemsetAsync.  On the null stream all of that is serialised whatever the library does, so the rest of the suite cannot see an
ordering mistake.  Here the work runs on non-blocking caller streams behind a delay of tens of milliseconds
(tests/stream_helpers.py): a launch on the wrong stream, or in front of the wait it needs, reads memory that is not written
yet and the comparison with the oracle fails.  Each test asserts that the delay did its work (the delayed stream is still busy
when the calls under test have returned; where two streams must run side by side, that the second one did).

  a  every entry point on a delayed non-null stream, results through the ordinary readers;
  b  Forward on stream A, Backward on stream B with no host synchronisation between (both branches of hx_batch_backward), then
     everything that reads the state records;
  c  two batches in flight on two streams, through the one side stream and the one copy stream of the device - launched from
     one host thread and from two;
  d  relaunches on one non-null stream without host synchronisation.

Test b on the parent of the commit that added this file (leaf-only batch, both branches of hx_batch_backward):
hx_batch_backward built the state records on B in front of its ordering against the Forward launch, from per-class tables
the preparation kernel had not written yet.  Cells, lpEnd, lpStart, best_trace() and the sampled walks were right; the
assertion that failed was hx_batch_indel_counts of job 0 against oracle/counts_dp_oracle.py: "ins" 6.04557174858178 where
1.5113929371454342 is expected.  With only that one line moved back the same assertion fails with the same figures.  See
DESIGN.md section 16."""
import ctypes as C
import functools
import random
import threading

import numpy as np
import pytest

from tests import stream_helpers as SH          # (imports torch: before the HIP library is loaded)
from historian_amd import capi, counts
from oracle import branch_oracle as bo
from oracle import c_oracle, counts_dp_oracle as cd
from oracle import historian_oracle as ho
from oracle import quickalign_oracle as q
from oracle import sumprod_oracle as so
from tests import helpers as H
from tests import indel_carry_ref as R
from tests import recon_helpers as RH
from tests import sibling_ref as sr
from tests import walks_cases as wc
from tests import walks_ref as wr
from tests.test_gpu_branch import CASES as BRANCH_CASES, as_job as branch_job, dense as branch_dense, random_branch
from tests.test_gpu_mixed_batch import _mixed_cases
from tests.test_gpu_quickalign import make_pair, score_vector
from tests.test_gpu_sample_traces import oracle_walks, uniforms
from tests.test_gpu_sibling import CASES as SIBLING_CASES, as_job as sibling_job, build as sibling_build, dense as sibling_dense
from tests.test_gpu_sumprod import _fixture as sumprod_fixture
from tests.test_gpu_traceback import ArrayForward

pytestmark = pytest.mark.gpu

AA = "arndcqeghilkmfpstwyv"
G = "tests/golden/reference_data/"
M = "tests/golden/models/"
KEEP = capi.HX_KEEP_BACKWARD
TM = dict(l_t=.2, r_t=.3, l_ins_wait=.09, l_del_wait=.08, r_ins_wait=.14, r_del_wait=.13)      # (tests/test_gpu_counts_dp.py)


def _times(tm):
    return [tm[k] for k in ("l_t", "r_t", "l_ins_wait", "l_del_wait", "r_ins_wait", "r_del_wait")]


@pytest.fixture(scope="module", autouse=True)
def engine():
    capi.init(0, c_oracle.table())
    SH.one_hip_runtime()
    SH.cycles_per_ms()
    yield
    capi.shutdown()


@pytest.fixture
def S():
    s = SH.Streams()
    yield s
    s.release()


@pytest.fixture(scope="module")
def pair(engine):
    """two caller streams that run side by side (kept for the module: drawing them costs a delay per pair tried)"""
    s = SH.Streams()
    a, b = SH.concurrent_pair(s)
    yield a, b
    s.release()


# ---------------------------------------------------------------------------
# cases and their references: computed once, shared, never changed
# ---------------------------------------------------------------------------
class PairRef:
    """A list of pair DPs (unfilled oracle ForwardMatrix objects) with what the oracle says about them, on demand."""

    def __init__(self, cases, true_math=False):
        self.cases = list(cases)
        self.imgs = [H.job_images(f) for f in self.cases]
        self.true_math = true_math
        self.n = len(self.cases)

    @functools.lru_cache(maxsize=None)
    def fwd(self, k):
        return c_oracle.forward(*self.imgs[k], true_math=self.true_math)

    @functools.lru_cache(maxsize=None)
    def bwd(self, k):
        return c_oracle.backward(*self.imgs[k], true_math=self.true_math)

    @functools.lru_cache(maxsize=None)
    def best(self, k):
        """the oracle's best path over the oracle's own cells (tests/test_gpu_traceback.py)"""
        w = self.fwd(k)
        return [tuple(c) for c in ArrayForward(self.cases[k], w["cells"], w["lp_end"]).best_trace()]

    @functools.lru_cache(maxsize=None)
    def walks(self, k, seed, n_walks):
        w = self.fwd(k)
        return oracle_walks(self.cases[k], w["cells"], w["lp_end"], seed, n_walks)

    @functools.lru_cache(maxsize=None)
    def indel(self, k):
        """oracle/counts_dp_oracle.py over the plain-C oracle's Forward and Backward cells"""
        f = self.cases[k]
        fw = RH.ArrayForward(f.x, f.y, f.hmm, f.parent_row_index, f.envelope)
        return cd.get_indel_counts(RH.ArrayBackward(fw), TM)

    @functools.lru_cache(maxsize=None)
    def mask(self, k):
        return H.envelope_mask(self.cases[k])


@functools.lru_cache(maxsize=None)
def mixed_ref():
    return PairRef(_mixed_cases())


@functools.lru_cache(maxsize=None)
def leaf_only_ref():
    # no general-profile job: the state records of such a batch are deferred (hx_api.hip ensure_state_records)
    return PairRef([H.leaf_case(11, 70, 66), H.leaf_case(12, 130, 90, band=6), H.leaf_case(15, 3, 5)])


COUNT_KEEP = ho.DPMatrix.CountIndelEvents          # (no CollapseChains: the best-trace profile keeps its null states)


@functools.lru_cache(maxsize=None)
def chain_ref():
    """Pairs of in-degree-1 profiles with null states inside - the chain classes (5 unbanded, 6 banded): children made from
    the best trace alone.  The first three carry indel counts on their transitions (tests/indel_carry_ref.py)."""
    wag = ho.RateModel.from_file(M + "wag.json")
    pf = [s[:24] for _, s in R.read_fasta(G + "PF16593.fa")[:4]]
    tc = dict(R.read_fasta(G + "testcount.fa"))
    tcm = ho.RateModel.from_file(G + "testcount.jukescantor.json")
    roots = [R.root_pair(wag, pf, (.1, .2, .15, .3), COUNT_KEEP, kind="sampled", seed=4, samples=0),
             R.root_pair(wag, pf, (.1, .2, .15, .3), COUNT_KEEP, kind="sampled", seed=4, samples=0, band=4),
             R.root_pair(tcm, [tc["seq2"], tc["seq3"], tc["seq1"]], (1., 1., 1., .001), COUNT_KEEP, kind="sampled", seed=4, samples=0),
             H.dag_case(96, n=70, samples=0, keep_all=True)]    # more than one strip of rows; carries nothing
    roots[3].tm = cd.branch_times(H.jc_model(), .2, .05)        # (dag_case: an even seed takes jc_model, branches .2 and .05)
    return PairRef(roots)


@functools.lru_cache(maxsize=None)
def carry_ref(k):
    """tests/indel_carry_ref.py for job k of chain_ref(): (counts, x_post, y_post)"""
    f = chain_ref().cases[k]
    f.fill()
    return R.get_indel_counts(ho.BackwardMatrix(f), f.tm)


BAND2_CASES = [(401, 70, 66, 5), (402, 200, 90, 12), (403, 130, 150, 3), (404, 300, 330, 20), (405, 40, 45, 0), (407, 500, 520, 8),
               (408, 33, 31, 4), (409, 260, 250, 20), (410, 64, 64, 6)]


@functools.lru_cache(maxsize=None)
def band2_ref(lo=0, hi=9):
    """the nine banded pairs of tests/test_gpu_trunc.py::test_two_banded_pairs_per_wavefront (or a run of them), with the
    oracle in libm arithmetic with the reference's truncation: the yardstick of HX_LSE_TRUNC"""
    def case(seed, lx, ly, band):
        if seed in (404, 409):
            return H.leaf_case(seed, lx, ly, alphabet=AA, jc=False, band=band)
        return H.leaf_case(seed, lx, ly, band=band)
    return PairRef([case(*c) for c in BAND2_CASES[lo:hi]], true_math=2)


@functools.lru_cache(maxsize=None)
def multi_leaf_ref():
    # tests/test_gpu_parity.py::test_a_small_batch_of_leaf_pairs_dealt_to_several_workgroups
    return PairRef([H.leaf_case(701, 700, 650, alphabet=AA, jc=False), H.leaf_case(702, 330, 400), H.leaf_case(703, 130, 90),
                    H.leaf_case(704, 520, 300, alphabet=AA, jc=False, components=2), H.leaf_case(705, 641, 64)])


@functools.lru_cache(maxsize=None)
def multi_dag_ref():
    # tests/test_gpu_parity.py::test_a_small_batch_of_general_pairs_dealt_to_several_workgroups
    return PairRef([H.dag_case(86, n=400, samples=3), H.dag_case(87, n=300, samples=3), H.dag_case(88, n=200, samples=4, band=6),
                    H.dag_case(71, n=90, samples=4), H.dag_case(89, n=40, samples=3)])


@functools.lru_cache(maxsize=None)
def compressed_ref():
    # tests/test_gpu_parity.py::test_band_compressed_planes_in_the_table_policies, the few-pairs batch
    return PairRef([H.leaf_case(601, 200, 90, band=12), H.leaf_case(602, 130, 150, band=3), H.leaf_case(603, 70, 66),
                    H.leaf_case(604, 300, 310, band=0)])


@functools.lru_cache(maxsize=None)
def banded_dag_ref():
    return PairRef([H.dag_case(43, band=3)])


def decoy_images(imgs):
    """The same profiles under other branches: every substitution and insertion log-probability moved.  Run and destroyed
    before the batch under test is created, so that what the new batch's tables hold before its own preparation has run -
    fresh memory or the decoy's - is not accidentally what the preparation will write."""
    out = []
    for x, y, h, md in imgs:
        d = capi.HmmImage(h.lp_trans, h.log_root - .37, h.log_sub_l - .61, h.log_sub_r - .23, h.log_ins_l - .83, h.log_ins_r - .47,
                          h.log_cptw_l, h.log_cptw_r)
        out.append((x, y, d, md))
    return out


def run_decoy(imgs, flags):
    d = capi.Batch(decoy_images(imgs), flags | KEEP)
    d.forward()
    d.backward()
    d.lp_start()
    d.best_trace(raw=True)       # (builds the decoy's state records where the batch under test will have its own)
    d.close()


# ---------------------------------------------------------------------------
# comparisons
# ---------------------------------------------------------------------------
def check_exact_fills(b, ref, backward=True, what=""):
    """Forward and Backward cells, lpEnd and lpStart bit for bit the oracle's; best_trace() the oracle's best path"""
    lp_end = b.lp_end()
    lp_start = b.lp_start() if backward else None
    for k in range(ref.n):
        H.assert_same_bits(b.read_matrix(k, 0), ref.fwd(k)["cells"], "%s: Forward cells of job %d" % (what, k))
        H.assert_same_bits([lp_end[k]], [ref.fwd(k)["lp_end"]], "%s: lpEnd of job %d" % (what, k))
        if backward:
            H.assert_same_bits(b.read_matrix(k, 1), ref.bwd(k)["cells"], "%s: Backward cells of job %d" % (what, k))
            H.assert_same_bits([lp_start[k]], [ref.bwd(k)["lp_start"]], "%s: lpStart of job %d" % (what, k))
    paths = b.best_trace()
    for k in range(ref.n):
        assert paths[k] == ref.best(k), "%s: best path of job %d" % (what, k)


def check_record_readers(b, ref, what="", seed=5489, n_walks=2):
    """what reads the 80-byte state records: best_trace (check_exact_fills), sample_traces, indel_counts"""
    for k in range(ref.n):
        lay = b.layout(k)
        walks, draws = ref.walks(k, seed, n_walks)
        got, got_draws = b.sample_traces(k, n_walks, uniforms(seed, n_walks * (lay.n_rows + lay.n_cols + 4)))
        assert got_draws == draws and got == walks, "%s: sampled walks of job %d" % (what, k)
        counts_k, want = b.indel_counts(k, _times(TM)), ref.indel(k)
        for key in cd.KEYS:
            # exact policy: the oracle's cells bit for bit, so only exp() and the order of the sum differ
            # (the bound of tests/test_gpu_counts_dp.py)
            assert abs(counts_k[key] - want[key]) <= 1e-9 * max(1., abs(want[key])), (what, k, key, counts_k[key], want[key])


def check_trunc_fills(b, ref, what=""):
    """the yardsticks of tests/test_gpu_trunc.py::test_two_banded_pairs_per_wavefront, dense planes, both fills"""
    lt, st = b.lp_end(), b.lp_start()
    for k in range(ref.n):
        want, got = ref.fwd(k), b.read_matrix(k, 0)
        assert not np.isnan(got).any(), "%s: job %d" % (what, k)
        assert np.array_equal(np.isneginf(want["cells"]), np.isneginf(got)), "%s: job %d: -inf pattern" % (what, k)
        fin = np.isfinite(want["cells"])
        assert np.max(np.abs(want["cells"][fin] - got[fin]), initial=0.) < 1e-9, "%s: job %d" % (what, k)
        if np.isfinite(want["lp_end"]):
            assert abs(want["lp_end"] - lt[k]) <= 1e-12 * abs(lt[k]), "%s: lpEnd of job %d" % (what, k)
        else:
            assert lt[k] == want["lp_end"], "%s: lpEnd of job %d" % (what, k)
        want, got = ref.bwd(k), b.read_matrix(k, 1)
        assert np.array_equal(np.isneginf(want["cells"]), np.isneginf(got)), "%s: job %d Backward -inf pattern" % (what, k)
        fin = np.isfinite(want["cells"])
        assert np.max(np.abs(want["cells"][fin] - got[fin]), initial=0.) < 1e-9, "%s: job %d Backward" % (what, k)
        if np.isfinite(want["lp_start"]):
            assert abs(want["lp_start"] - st[k]) <= 1e-12 * abs(st[k]), "%s: lpStart of job %d" % (what, k)
        else:
            assert st[k] == want["lp_start"], "%s: lpStart of job %d" % (what, k)


def snapshot(b, ref, backward=True, env_only=False):
    """everything a fill leaves behind, for bit comparisons between two runs"""
    out = {"lp_end": b.lp_end().copy()}
    if backward:
        out["lp_start"] = b.lp_start().copy()
    for k in range(ref.n):
        for which in ((0, 1) if backward else (0,)):
            m = b.read_matrix(k, which)
            out["m%d_%d" % (which, k)] = m[ref.mask(k)] if env_only else m
    return out


def assert_same_snapshot(got, want, what):
    assert sorted(got) == sorted(want)
    for key in want:
        H.assert_same_bits(got[key], want[key], "%s: %s" % (what, key))


# ---------------------------------------------------------------------------
# a. every entry point on a delayed non-null stream
# ---------------------------------------------------------------------------
def test_a_mixed_batch_on_a_delayed_stream(S):
    ref = mixed_ref()
    twin = capi.Batch(ref.imgs, KEEP)                # (a first run on the null stream: kernels loaded, nothing left to set up)
    twin.forward()
    twin.backward()
    twin.sync()
    a = S.new()
    b = capi.Batch(ref.imgs, KEEP)
    S.busy(a)
    b.forward(SH.handle(a))
    b.backward(SH.handle(a))
    SH.assert_busy(a, "mixed batch")
    check_exact_fills(b, ref, what="delayed stream")
    b.close()
    twin.close()


@pytest.mark.parametrize("side", ["side stream", "no side stream"])
def test_a_two_banded_pairs_per_wavefront_on_a_delayed_stream(side, S, monkeypatch):
    # hx_band2.hip: the sweep on the caller's stream, its edge kernel on the device's side stream (fork behind the preparation,
    # join before the result kernel), or both on the caller's stream (HX_NO_SIDE_STREAM)
    monkeypatch.setenv("HX_BAND2", "1")
    if side == "no side stream":
        monkeypatch.setenv("HX_NO_SIDE_STREAM", "1")
    ref = band2_ref()
    flags = capi.HX_LSE_TRUNC | KEEP
    twin = capi.Batch(ref.imgs, flags)               # a second batch object on the null stream
    assert twin.shared_wavefront_pairs() == 9
    twin.forward()
    twin.backward()
    want = snapshot(twin, ref, env_only=True)
    a = S.new()
    b = capi.Batch(ref.imgs, flags)
    assert b.shared_wavefront_pairs() == 9
    S.busy(a)
    b.forward(SH.handle(a))
    b.backward(SH.handle(a))
    SH.assert_busy(a, "two banded pairs per wavefront")
    check_trunc_fills(b, ref, what=side)
    assert_same_snapshot(snapshot(b, ref, env_only=True), want, "delayed stream vs null stream (%s)" % side)
    b.close()
    twin.close()


@pytest.mark.parametrize("kind", ["leaf pairs", "general profiles"])
def test_a_pairs_dealt_to_several_workgroups_on_a_delayed_stream(kind, S, monkeypatch):
    # the progress counters of these launches are zeroed with hipMemsetAsync on the caller's stream
    if kind == "leaf pairs":
        monkeypatch.setenv("HX_CHAIN_MULTI", "3")
        ref, classes = multi_leaf_ref(), (0,)
    else:
        monkeypatch.setenv("HX_DAG_MULTI_MIN_STRIPS", "2")
        monkeypatch.delenv("HX_DAG_FWD_SINGLE", raising=False)
        monkeypatch.delenv("HX_DAG_BWD_SINGLE", raising=False)
        ref, classes = multi_dag_ref(), (7, 8)
    twin = capi.Batch(ref.imgs, KEEP)
    twin.forward()
    twin.backward()
    twin.sync()
    a = S.new()
    b = capi.Batch(ref.imgs, KEEP)
    assert all(b.job_kernel(k)[0] in classes for k in range(ref.n))
    S.busy(a)
    b.forward(SH.handle(a))
    b.backward(SH.handle(a))
    SH.assert_busy(a, kind)
    check_exact_fills(b, ref, what=kind)
    assert b.relaunches() == 0
    b.close()
    twin.close()


@functools.lru_cache(maxsize=None)
def quick_jobs():
    model = ho.RateModel.from_file(G + "testamino.json")
    model.sub_rate = [m.tolist() for m in model.sub_rate]
    sc = q.QuickAlignScores(model, 1.0)
    alph = model.alphabet
    rng = random.Random(11)
    pairs = [make_pair(rng, alph, lx, ly) + (None,) for lx, ly in ((33, 36), (65, 63), (200, 150))]
    x, y = make_pair(rng, alph, 120, 90, sub=.1)
    env = q.DiagonalEnvelope(x, y)
    env.init_sparse(q.KmerIndex(y, alph, 3), band_size=8, kmer_threshold=1)
    assert len(env.diagonals) < 120 + 90 - 1
    pairs.append((x, y, env.diagonals))
    jobs = [(q.tokens(x, alph), q.tokens(y, alph), len(alph), sc.submat, score_vector(sc), d) for x, y, d in pairs]
    return jobs, [c_oracle.quickalign(xt, yt, a, sm, sc, d) for xt, yt, a, sm, sv, d in jobs]


def test_a_guide_alignment_batch_on_a_delayed_stream(S):
    jobs, want = quick_jobs()
    twin = capi.QuickBatch(jobs)
    twin.run()
    twin.results()
    a = S.new()
    b = capi.QuickBatch(jobs)
    S.busy(a)
    b.run(SH.handle(a))
    SH.assert_busy(a, "QuickBatch")
    score, xe, ye = b.results()
    for k, w in enumerate(want):
        H.assert_same_bits(b.read_matrix(k), w["cells"], "pair %d cells" % k)
        H.assert_same_bits([score[k]], [w["score"]], "pair %d score" % k)
        assert (int(xe[k]), int(ye[k])) == (w["x_end"], w["y_end"])
    b.close()
    twin.close()


@functools.lru_cache(maxsize=None)
def branch_refs(viterbi):
    cases = [random_branch(*c) for c in BRANCH_CASES[0:5]]
    want = [bo.BranchMatrix(x, ysub, yemit, T, None if xe is None else list(xe), None if ye is None else list(ye), md, viterbi=viterbi)
            for x, ysub, yemit, T, xe, ye, md in cases]
    return cases, want


@pytest.mark.parametrize("viterbi", [True, False])
def test_a_branch_batch_on_a_delayed_stream(viterbi, S):
    cases, want = branch_refs(viterbi)
    twin = capi.BranchBatch([branch_job(c) for c in cases])
    twin.run(viterbi=viterbi)
    twin.lp_end()
    a = S.new()
    b = capi.BranchBatch([branch_job(c) for c in cases])
    S.busy(a)
    b.run(viterbi=viterbi, stream=SH.handle(a))
    SH.assert_busy(a, "BranchBatch")
    lp = b.lp_end()
    for k, w in enumerate(want):
        H.assert_same_bits(b.read_matrix(k), branch_dense(w), "job %d cells (%s)" % (k, "viterbi" if viterbi else "forward"))
        H.assert_same_bits([lp[k]], [w.lp_end], "job %d lpEnd" % k)
    b.close()
    twin.close()


# the three smallest cases of tests/test_gpu_sibling.py with more than one strip of 64 rows (l_len + 1 > 64)
SIBLING_PICK = sorted((c for c in SIBLING_CASES if c[1] + 1 > 64), key=lambda c: (c[1] + 1) * (c[2] + 1))[:3]


@functools.lru_cache(maxsize=None)
def sibling_refs():
    return [sibling_build(c) for c in SIBLING_PICK]


def test_a_sibling_batch_on_a_delayed_stream(S):
    assert [c[0] for c in SIBLING_PICK] == [14, 12, 13]
    built = sibling_refs()
    twin = capi.SiblingBatch([sibling_job(case, m) for case, m in built])
    twin.run()
    twin.lp_end()
    a = S.new()
    b = capi.SiblingBatch([sibling_job(case, m) for case, m in built])
    S.busy(a)
    b.run(SH.handle(a))
    SH.assert_busy(a, "SiblingBatch")
    lp = b.lp_end()
    for k, (case, want) in enumerate(built):
        got, full = b.read_matrix(k), sibling_dense(want)
        for s, name in enumerate(capi.SiblingBatch.STATES):
            H.assert_same_bits(got[:, :, s], full[:, :, s], "job %d plane %s" % (k, name))
        H.assert_same_bits([lp[k]], [want.lp_end], "job %d lpEnd" % k)
    b.close()
    twin.close()


def test_a_sumprod_columns_on_a_delayed_stream(S):
    # the smallest case of tests/test_gpu_sumprod.py: the reference's testaligncount alignment.  The call returns when its
    # kernels are done, so "still busy" is checked immediately before it.
    omodel, model, tree, gapped = sumprod_fixture("testnj.jukescantor.json", "testaligncount.fa", "testaligncount.nh")
    cc = counts.ColumnCounter(model, tree.parent, tree.branch_length)
    tok = counts.tokenize_columns(model.alphabet, [gapped[n] for n in range(tree.nodes())])
    args = (cc.parent, cc.ins_prob, cc.log_cpt_weight, cc.branch_sub, np.asarray(cc.eigen.evec), np.asarray(cc.eigen.evec_inv), cc.esc, tok)
    capi.sumprod_columns(*args, want_root_post=True)
    a = S.new()
    S.busy(a)
    SH.assert_busy(a, "sumprod_columns")
    cll, root, eig, post = capi.sumprod_columns(*args, want_root_post=True, stream=SH.handle(a))
    with open(G + "testaligncount.out") as f:
        assert so.write_sub_counts(omodel, root, cc.eigen.sub_counts(eig)) + "\n" == f.read()
    sp = so.SumProduct(omodel, tree)
    for col, seq in enumerate(so.columns_of(tree, gapped)):
        sp.init_column(seq)
        sp.fill_up()
        sp.fill_down()
        assert abs(cll[col] - sp.col_log_like) <= 1e-12 * abs(sp.col_log_like)
        np.testing.assert_allclose(np.exp(post[col]), np.exp(sp.log_node_post_prob(sp.column_root())), rtol=1e-9, atol=1e-300)


def test_a_branch_walks_on_a_delayed_stream(S):
    # best_paths / sample_paths / read_cells launch on the batch's last stream, behind the fill (tests/test_gpu_walks.py;
    # case 1 of tests/walks_cases.py, whose word streams tests/test_oracle_walks.py clears of near-boundary draws)
    k = 1
    c = wc.BRANCH_CASES[k]
    case, bm = wc.branch_matrix(c)
    _, vm = wc.branch_matrix(c, viterbi=True)
    twin = capi.BranchBatch([branch_job(case)])
    twin.run(viterbi=True)
    twin.best_paths()
    twin.run(viterbi=False)
    twin.sample_paths([wc.words(k, 0, c[1], c[2])])
    twin.read_cells(0, [(0, 0, 0)])
    a = S.new()
    b = capi.BranchBatch([branch_job(case)])
    S.busy(a)
    b.run(viterbi=True, stream=SH.handle(a))
    SH.assert_busy(a, "branch best_paths")
    paths, n_steps = b.best_paths()
    assert paths[0] == wr.best_states(vm) and n_steps[0] == len(paths[0])
    assert wr.branch_rows_of_states(vm, paths[0]) == vm.best()
    S.busy(a)
    b.run(viterbi=False, stream=SH.handle(a))
    SH.assert_busy(a, "branch sample_paths")
    for qq in range(wc.STREAMS):
        words = wc.words(k, qq, c[1], c[2])
        paths, n_steps, used = b.sample_paths([words])
        w = wr.branch_walk(bm, wr.WordSource(words))
        assert paths[0] == w.states, "stream %d" % qq
        assert (n_steps[0], used[0]) == (len(w.states), w.words_used)
    S.busy(a)
    b.run(viterbi=False, stream=SH.handle(a))
    SH.assert_busy(a, "branch read_cells")
    path = wr.branch_walk(bm, wr.WordSource(wc.words(k, 0, c[1], c[2]))).rows
    at = wr.path_cells_branch(path)
    cells, lm = b.read_cells(0, at)
    full = branch_dense(bm)
    H.assert_same_bits(cells, np.array([full[i, j, s] for i, j, s in at]), "gathered cells")
    cell = {cc: v for cc, v in zip(at, cells)}
    match = {cc[:2]: v for cc, v in zip(at, lm)}

    def lp_emit(i, j, s):
        return match[(i, j)] if s == bo.MATCH else bm.lp_emit(i, j, s)
    got_lp = wr.branch_log_post_prob(bm, path, cell=lambda i, j, s: cell[(i, j, s)], lp_emit=lp_emit, lp_end=b.lp_end()[0])
    H.assert_same_bits([got_lp], [wr.branch_log_post_prob(bm, path)], "logPostProb from gathered cells")
    b.close()
    twin.close()


def test_a_sibling_walks_on_a_delayed_stream(S):
    import copy
    k = 1
    c = wc.SIBLING_CASES[k]
    case, m = wc.sibling_matrix(c)
    twin = capi.SiblingBatch([sibling_job(case, m)])
    twin.run()
    twin.sample_paths([wc.words(100 + k, 0, c[1], c[2])])
    twin.read_cells(0, [(0, 0, 0)])
    a = S.new()
    b = capi.SiblingBatch([sibling_job(case, m)])
    S.busy(a)
    b.run(SH.handle(a))
    SH.assert_busy(a, "sibling sample_paths")
    for qq in range(wc.STREAMS):
        words = wc.words(100 + k, qq, c[1], c[2])
        paths, n_steps, used = b.sample_paths([words])
        w = wr.sibling_walk(m, wr.WordSource(words))
        assert paths[0] == w.states, "stream %d" % qq
        assert (n_steps[0], used[0]) == (len(w.states), w.words_used)
    S.busy(a)
    b.run(SH.handle(a))
    SH.assert_busy(a, "sibling read_cells")
    path = wr.sibling_walk(m, wr.WordSource(wc.words(100 + k, 0, c[1], c[2]))).rows
    at = wr.path_cells_sibling(path)
    cells, lm = b.read_cells(0, at)
    full = sibling_dense(m)
    H.assert_same_bits(cells, np.array([full[i, j, s] for i, j, s in at]), "gathered cells")
    dev = copy.copy(m)
    dev.cells, dev.lp_end = None, b.lp_end()[0]                    # nothing of the restatement's matrix is read
    dev._match = {cc[:2]: v for cc, v in zip(at, lm)}
    cell = {cc: v for cc, v in zip(at, cells)}
    dev.cell = lambda i, j, s, cell=cell, dev=dev: dev.lp_end if s == sr.EEE else cell[(i, j, s)]
    H.assert_same_bits([dev.log_post_prob(path)], [m.log_post_prob(path)], "logPostProb from gathered cells")
    b.close()
    twin.close()


# ---------------------------------------------------------------------------
# b. Forward on A, Backward on B
# ---------------------------------------------------------------------------
def forward_on_a_backward_on_b(S, pair, ref, keep, what):
    """-> the batch, both fills launched with no host synchronisation between them and both preconditions held"""
    a, b_stream = pair
    flags = KEEP if keep else 0
    run_decoy(ref.imgs, 0)
    b = capi.Batch(ref.imgs, flags)
    S.busy(a)
    b.forward(SH.handle(a))
    marker = SH.Marker(b_stream)
    assert marker.done_while_busy(a), "%s: the second stream waited for the first one's delay" % what
    if not keep:
        # hx_batch_backward allocates the Backward matrices now and synchronises with the Forward stream itself
        SH.assert_busy(a, what)
    b.backward(SH.handle(b_stream))
    if keep:
        SH.assert_busy(a, what)
    return b


@pytest.mark.parametrize("keep", [True, False], ids=["keep_backward", "allocate_now"])
def test_b_leaf_only_batch_forward_on_a_backward_on_b(keep, S, pair):
    ref = leaf_only_ref()
    b = forward_on_a_backward_on_b(S, pair, ref, keep, "leaf-only batch")
    assert all(b.job_kernel(k)[0] in (0, 1, 2, 3, 4) for k in range(ref.n))
    check_exact_fills(b, ref, what="leaf-only batch")
    check_record_readers(b, ref, what="leaf-only batch")
    b.close()


@pytest.mark.parametrize("keep", [True, False], ids=["keep_backward", "allocate_now"])
def test_b_chain_profile_batch_forward_on_a_backward_on_b(keep, S, pair):
    ref = chain_ref()
    b = forward_on_a_backward_on_b(S, pair, ref, keep, "chain-profile batch")
    assert [b.job_kernel(k)[0] for k in range(ref.n)] == [5, 6, 5, 5]
    check_exact_fills(b, ref, what="chain-profile batch")
    check_record_readers(b, ref, what="chain-profile batch")
    for k, f in enumerate(ref.cases):
        carried = hasattr(f.x, "trans_counts") or hasattr(f.y, "trans_counts")
        assert carried == (k < 3)
        got = b.event_counts(k, _times(f.tm), R.carried_table(f.x) if carried else None, R.carried_table(f.y) if carried else None)
        want = carry_ref(k)
        for key in R.KEYS:
            # exact policy (tests/test_gpu_event_counts.py::test_internal_node_pairs)
            assert abs(got[0][key] - want[0][key]) <= 1e-9 * max(1., abs(want[0][key])), (k, key, got[0][key], want[0][key])
        assert np.max(np.abs(got[1] - np.array(want[1]))) <= 1e-9 and np.max(np.abs(got[2] - np.array(want[2]))) <= 1e-9, k
    b.close()


@pytest.mark.parametrize("keep", [True, False], ids=["keep_backward", "allocate_now"])
def test_b_mixed_batch_forward_on_a_backward_on_b(keep, S, pair):
    ref = mixed_ref()
    b = forward_on_a_backward_on_b(S, pair, ref, keep, "mixed batch")
    check_exact_fills(b, ref, what="mixed batch")
    check_record_readers(b, ref, what="mixed batch")
    b.close()


# ---------------------------------------------------------------------------
# c. two batches in flight at once
# ---------------------------------------------------------------------------
def _host_alloc():
    lib = capi.load()
    lib.hx_host_alloc.argtypes = [C.c_size_t, C.POINTER(C.c_void_p)]
    lib.hx_host_free.argtypes = [C.c_void_p]
    return lib


def async_read_all(batches_refs):
    """hx_batch_read_matrix_async for every job and matrix of every batch (all on the device's one copy stream), then
    hx_batch_wait_read -> per batch a snapshot-like dict of un-skewed matrices"""
    lib = _host_alloc()
    started = []
    for n, (b, ref) in enumerate(batches_refs):
        for k in range(ref.n):
            for which in (0, 1):
                lay = b.layout(k, which)
                p = C.c_void_p()
                assert lib.hx_host_alloc(lay.matrix_doubles * 8, C.byref(p)) == 0
                assert lib.hx_batch_read_matrix_async(b._h, k, which, C.cast(p, C.POINTER(C.c_double))) == 0
                started.append((n, k, which, lay, p))
    out = [dict() for _ in batches_refs]
    for n, k, which, lay, p in started:
        b = batches_refs[n][0]
        assert lib.hx_batch_wait_read(b._h, k, which) == 0
        buf = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_double)), shape=(lay.matrix_doubles,)).copy()
        lib.hx_host_free(p)
        ii, jj = np.meshgrid(np.arange(lay.n_rows), np.arange(lay.n_cols), indexing="ij")
        slot = capi.slot_index(lay, ii, jj)
        out[n]["m%d_%d" % (which, k)] = np.stack([buf[s * lay.plane_stride + slot] for s in range(5)], axis=-1)
    for n, (b, ref) in enumerate(batches_refs):
        out[n]["lp_end"], out[n]["lp_start"] = b.lp_end().copy(), b.lp_start().copy()
    return out


@functools.lru_cache(maxsize=None)
def alone_on_the_null_stream(lo, hi):
    """five banded pairs in the two-pairs-per-wavefront sweep, run alone on the null stream (HX_BAND2=1 is the caller's)"""
    ref = band2_ref(lo, hi)
    b = capi.Batch(ref.imgs, capi.HX_LSE_TRUNC | KEEP)
    assert b.shared_wavefront_pairs() == 5
    b.forward()
    b.backward()
    want = snapshot(b, ref)
    b.close()
    return want


@pytest.mark.parametrize("threads", [1, 2], ids=["one_host_thread", "two_host_threads"])
def test_c_two_batches_in_flight_through_one_side_stream_and_one_copy_stream(threads, S, pair, monkeypatch):
    monkeypatch.setenv("HX_BAND2", "1")
    monkeypatch.delenv("HX_NO_SIDE_STREAM", raising=False)
    a, bs = pair
    refs = band2_ref(0, 5), band2_ref(4, 9)
    want = alone_on_the_null_stream(0, 5), alone_on_the_null_stream(4, 9)
    p, qb = (capi.Batch(r.imgs, capi.HX_LSE_TRUNC | KEEP) for r in refs)
    assert p.shared_wavefront_pairs() == 5 and qb.shared_wavefront_pairs() == 5
    S.busy(a)
    if threads == 1:
        p.forward(SH.handle(a))
        marker = SH.Marker(bs)                       # (before Q's launches: those join the shared side stream behind P's fork)
        qb.forward(SH.handle(bs))
        p.backward(SH.handle(a))
        qb.backward(SH.handle(bs))
    else:
        marker = SH.Marker(bs)
        barrier = threading.Barrier(2)
        failed = []

        def drive(batch, stream):
            try:
                barrier.wait()
                batch.forward(stream)                # (ctypes releases the GIL inside the calls)
                batch.backward(stream)
            except BaseException as e:              # noqa: BLE001 - handed to the main thread
                failed.append(e)
        workers = [threading.Thread(target=drive, args=(p, SH.handle(a))), threading.Thread(target=drive, args=(qb, SH.handle(bs)))]
        for w in workers:
            w.start()
        for w in workers:
            w.join()
        assert not failed, failed
    SH.assert_busy(a, "two batches in flight")
    assert marker.done_while_busy(a), "the second stream waited for the first one's delay"
    got = async_read_all([(p, refs[0]), (qb, refs[1])])
    for n, name in enumerate(("P", "Q")):
        assert_same_snapshot(got[n], want[n], "batch %s in flight beside the other vs alone on the null stream" % name)
    p.close()
    qb.close()


# ---------------------------------------------------------------------------
# d. back-to-back relaunches on one non-null stream without host synchronisation
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["several workgroups", "band compressed", "banded general profile"])
def test_d_relaunches_on_one_stream_give_the_bits_of_a_single_launch(kind, S, monkeypatch):
    backward = kind != "band compressed"             # (a band-compressed batch has no Backward fill)
    if kind == "several workgroups":
        monkeypatch.setenv("HX_CHAIN_MULTI", "3")
        ref, flags, classes = multi_leaf_ref(), KEEP, (0,)
    elif kind == "band compressed":
        ref, flags, classes = compressed_ref(), capi.HX_BAND_COMPRESSED, (0, 1, 2)
    else:
        ref, flags, classes = banded_dag_ref(), KEEP, (8,)
    single = capi.Batch(ref.imgs, flags)
    assert all(single.job_kernel(k)[0] in classes for k in range(ref.n))
    single.forward()
    if backward:
        single.backward()
    want = snapshot(single, ref, backward=backward, env_only=not backward)
    want_paths = single.best_trace()
    single.close()
    a = S.new()
    h = SH.handle(a)
    for sequence in (("forward", "forward"), ("forward", "backward", "forward", "backward")):
        if not backward and "backward" in sequence:
            continue
        b = capi.Batch(ref.imgs, flags)
        S.busy(a)
        for step in sequence:
            getattr(b, step)(h)
        SH.assert_busy(a, "%s: %s" % (kind, ", ".join(sequence)))
        with_backward = backward and "backward" in sequence
        got = snapshot(b, ref, backward=with_backward, env_only=not backward)
        assert_same_snapshot(got, {k: v for k, v in want.items() if k in got}, "%s: %s" % (kind, ", ".join(sequence)))
        assert b.best_trace() == want_paths
        assert b.relaunches() == 0
        b.close()
    if kind == "several workgroups":                 # (and the single launch is the oracle's, bit for bit)
        for k in range(ref.n):
            H.assert_same_bits(want["m0_%d" % k], ref.fwd(k)["cells"], "single launch vs oracle")
            H.assert_same_bits(want["m1_%d" % k], ref.bwd(k)["cells"], "single launch vs oracle")
