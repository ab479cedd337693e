"""Branch batches made from a resident history on the device (hx_history_branch_batch_create behind
capi.History.branch_batch) against the path that existed before it, on the same history: download the two profiles of a
branch (History.excluded_profiles), run oracle/branch_oracle.py's pre_multiply and calc_ins_probs on the child's in Python,
upload the three arrays as an ordinary capi.BranchBatch.

No bound anywhere: the device performs the additions and the table log_sum_exp of the restatement in its order, so the
inputs are compared as 64-bit patterns (the -inf pattern included) and so is everything the fills and walks make of them.
pre_multiply is pure Python at C * A * A table sums per position, hence the small shapes; each test says how many."""
import functools
import time

import numpy as np
import pytest

from historian_amd import capi
from oracle import branch_oracle as bo
from oracle import c_oracle
from tests import history_edge_cases as HE
from tests import stream_helpers as SH
from tests import test_gpu_condpwm as TC
from tests import test_gpu_history as TH
from tests.test_gpu_ancestors import CYCLIC

pytestmark = pytest.mark.gpu

TRANS = bo.trans_scores(0.02, 0.03, 0.4, 0.5)
A21 = "abcdefghijklmnopqrstu"


@pytest.fixture(scope="module", autouse=True)
def engine():
    capi.init(0, c_oracle.table())
    yield
    capi.shutdown()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def logs(mats, ins_prob):
    """what the caller brings: the host's log of exp(R t) [C][A][A] and of the insertion distribution [C][A]"""
    with np.errstate(divide="ignore"):
        return np.log(np.asarray(mats, dtype=np.float64)), np.log(np.asarray(ins_prob, dtype=np.float64))


def envelopes(c, node, tokens=None):
    return capi.branch_guide_envelope(c.tokens if tokens is None else tokens, c.parent[node], node)


def yardstick_job(h, c, node, normalize, which=0, md=-1, env=(None, None), mats=None):
    """one job of the path before the hand-off: (x_pwm, y_sub, y_emit, trans, x_env, y_env, max_distance)"""
    parent_pwm, child = h.branch_profiles(node, normalize=normalize, which=which)
    log_sub, log_ins = logs(c.branch_sub[:, node] if mats is None else mats, c.ins_prob)
    y_sub = np.asarray(bo.pre_multiply(child.tolist(), log_sub.tolist()), dtype=np.float64).reshape(child.shape)
    y_emit = np.asarray(bo.calc_ins_probs(child.tolist(), log_ins.tolist(), [float(w) for w in c.log_cpt_weight]), dtype=np.float64)
    return (parent_pwm, y_sub, y_emit, TRANS, env[0], env[1], md)


def branch(c, node, md=-1, env=(None, None), mats=None):
    log_sub, log_ins = logs(c.branch_sub[:, node] if mats is None else mats, c.ins_prob)
    return (node, log_sub, log_ins, TRANS, env[0], env[1], md)


def words_for(batch, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 2 ** 32, size=batch.max_steps() + 8, dtype=np.uint64).astype(np.uint32) for _ in range(batch.n)]


def assert_same_batch(got, want, what, seed=7):
    """inputs, lp_end and cells of both fills, the best paths, the sampled paths: all equal"""
    assert got.n == want.n and got.shapes == want.shapes, what
    for k in range(got.n):
        for name, a, b in zip(("x_pwm", "y_sub", "y_emit"), got.read_inputs(k), want.read_inputs(k)):
            assert same(a, b), (what, k, name, int(np.sum(bits(a) != bits(b))) if a.shape == b.shape else (a.shape, b.shape))
    assert got.max_steps() == want.max_steps() and got.total_cells() == want.total_cells()
    words = words_for(want, seed)
    for viterbi in (True, False):
        got.run(viterbi=viterbi)
        want.run(viterbi=viterbi)
        assert same(got.lp_end(), want.lp_end()), (what, viterbi)
        for k in range(got.n):
            assert same(got.read_matrix(k), want.read_matrix(k)), (what, viterbi, k)
        if viterbi:
            assert got.best_paths() == want.best_paths(), what
        else:
            assert got.sample_paths(words) == want.sample_paths(words), what


def check_branches(h, c, nodes, what, normalize=True, which=0, md=-1, banded=False, tokens=None, mats=None):
    """the named branches in one call against the yardstick batch; -> the device-made batch (closed by the caller)"""
    envs = [envelopes(c, r, tokens) if banded else (None, None) for r in nodes]
    t0 = time.time()
    want = capi.BranchBatch([yardstick_job(h, c, r, normalize, which, md, e, None if mats is None else mats[r]) for r, e in zip(nodes, envs)])
    print("%s: %d branches, %d positions of children through the Python yardstick in %.2f s"
          % (what, len(nodes), sum(s[1] - 1 for s in want.shapes), time.time() - t0))
    got = h.branch_batch([branch(c, r, md, e, None if mats is None else mats[r]) for r, e in zip(nodes, envs)], normalize=normalize, which=which)
    assert_same_batch(got, want, what)
    want.close()
    return got


def kinds_of_branches(c):
    """a leaf branch, an internal branch that is no child of the root, a child of the root"""
    has_child = set(c.parent)
    leaf = next(r for r in range(c.n - 1) if r not in has_child)
    internal = next(r for r in range(c.n - 1) if r in has_child and c.parent[r] != c.n - 1)
    top = next(r for r in range(c.n - 1) if c.parent[r] == c.n - 1)
    return [leaf, internal, top]


# ---- 1. inputs, cells and walks against the path before ----

@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("name", ["acgt", "prot4", A21])
def test_inputs_cells_and_walks_equal_the_downloaded_path(name, normalize):
    """acgt: 130 columns, all 16 branches; prot4 (4 x 20): 70 columns, three branches; 21 symbols (the general kernels, an
    odd alphabet): 40 columns, three branches"""
    c = TH.case(name) if name == "acgt" else TH.case(name, 70 if name == "prot4" else 40)
    nodes = list(range(c.n - 1)) if name == "acgt" else kinds_of_branches(c)
    assert c.n == 17 and (name != "acgt" or len(nodes) == 16)
    h = c.history()
    before = h.log_like()
    got = check_branches(h, c, nodes, "%s normalize=%d" % (name, normalize), normalize=normalize)
    ms, split = h.kernel_ms(), h.handoff_ms()
    assert ms > 0 and all(v > 0 for v in split) and abs(sum(split) - ms) <= 1e-3 * ms + 1e-3
    after = h.log_like()
    assert after[0] == before[0] and after[1].tobytes() == before[1].tobytes()      # nothing is written to the history
    got.close()
    h.close()


# ---- 2. batches ----

def test_one_call_for_all_branches_sixteen_calls_and_a_repeat_give_the_same_bytes():
    c = TH.case("acgt")
    h = c.history()
    nodes = list(range(c.n - 1))
    jobs = [branch(c, r) for r in nodes]
    both = [h.branch_batch(jobs), h.branch_batch(jobs)]
    singles = [h.branch_batch([j]) for j in jobs]
    for b in both + singles:
        b.run(viterbi=False)
    lp = both[0].lp_end()
    assert same(lp, both[1].lp_end())
    for k in nodes:
        want = both[0].read_inputs(k)
        for other, job in ((both[1], k), (singles[k], 0)):
            assert all(same(a, b) for a, b in zip(want, other.read_inputs(job))), k
            assert same(both[0].read_matrix(k), other.read_matrix(job)), k
        assert same(lp[k:k + 1], singles[k].lp_end())
    for b in both + singles:
        b.close()
    h.close()


# ---- 3. bands ----

@pytest.mark.parametrize("md", [-1, 0, 2])
def test_bands_from_the_guide_envelope(md):
    """acgt, 130 columns, four branches; the yardstick batch gets the same envelopes"""
    c = TH.case("acgt")
    h = c.history()
    nodes = kinds_of_branches(c) + [c.n - 2]
    got = check_branches(h, c, nodes, "band %d" % md, md=md, banded=True)
    if md >= 0:
        got.run(viterbi=True)
        m = got.read_matrix(0)
        assert np.any(np.isneginf(m[1:-1, 1:-1]).all(axis=2))       # (the band leaves cells out)
    got.close()
    h.close()


# ---- 4. edges ----

@pytest.mark.parametrize("n_cols", [1, 64, 65])
def test_one_column_one_block_and_a_block_and_a_column(n_cols):
    """the seven-node edge tree at 1, 64 and 65 columns, all six branches, both forms of the profiles"""
    c = TC._edge(n_cols)
    h = c.history()
    for normalize in (True, False):
        check_branches(h, c, list(range(c.n - 1)), "edge x %d" % n_cols, normalize=normalize).close()
    h.close()


@functools.lru_cache(maxsize=None)
def _empty_rows():
    """10 columns of three kinds: nodes 3 is a gap everywhere (y_len = 0), nodes 5 and 6 in all but every third column,
    and where only leaves 0, 1 and node 4 are there node 6 has no position under node 4's branch"""
    kinds = ["ac--*--", "a------", "acg-***"]
    cols = [kinds[k % 3] for k in range(10)]
    return TH.Case(CYCLIC, TH.EDGE_PARENT, TH.EDGE_LENGTH, ["".join(col[r] for col in cols) for r in range(7)])


def test_rows_without_positions_and_leaves_holding_residues():
    c = _empty_rows()
    assert set(c.rows[3]) == {"-"}
    h = c.history()
    lens = h.row_lengths()
    assert lens[3] == 0 and lens[2] > 0 and lens[5] > 0
    got = check_branches(h, c, list(range(c.n - 1)), "rows without positions")
    assert got.shapes[3] == (int(lens[5]) + 1, 1)                   # y_len = 0 under a parent with positions
    leaf = h.branch_profiles(0)[1]                                   # a leaf's residue: 0 / -inf rows went through preMultiply
    assert np.isneginf(leaf).any() and np.isfinite(got.read_inputs(0)[1]).all()
    got.close()
    h.close()
    # ... and a parent without positions: only the columns in which leaf 0 stands alone
    alone = TH.Case(CYCLIC, TH.EDGE_PARENT, TH.EDGE_LENGTH, ["".join(col[r] for col in ["a------"] * 5) for r in range(7)])
    h = alone.history()
    got = check_branches(h, alone, [0, 3], "a parent without positions")
    assert got.shapes == [(1, 6), (1, 1)]
    got.close()
    h.close()


def test_zero_length_branches():
    """exp(R 0) is the identity: log_sub is 0 on the diagonal and -inf off it, -inf + -inf terms arise under leaves"""
    c = TC._zero_lengths()
    assert np.array_equal(c.branch_sub[0, 0], np.eye(4))
    assert np.isneginf(logs(c.branch_sub[:, 0], c.ins_prob)[0]).sum() == 12
    h = c.history()
    check_branches(h, c, [0, 5, 1], "zero-length branches").close()
    h.close()


@pytest.mark.parametrize("name,n_cols", [("anc prot x 9", 40), ("anc alphabet 64 x 3", 60)])
def test_more_components_than_waves_and_the_largest_alphabet(name, n_cols):
    """9 components of 20 symbols at 40 columns (3600 table sums per position), 3 of 64 symbols at 60 columns (12288 per
    position; more than the 32 positions k_history_pre_multiply takes per tile at that alphabet); the branch with the
    longest child, one each"""
    c = HE.case(name)
    tokens = c.tokens[:n_cols]
    assert len(tokens) == n_cols
    node = max((r for r in range(c.n - 1) if np.any(tokens[:, c.parent[r]] != -2)), key=lambda r: int(np.sum(tokens[:, r] != -2)))
    h = c.history(tokens=tokens)
    got = check_branches(h, c, [node], name, tokens=tokens)
    assert c.a < 64 or got.shapes[0][1] - 1 > 32
    got.close()
    h.close()


# ---- 5. the slots of a proposal ----

def test_the_slots_of_a_proposal_of_lengths():
    """acgt at 130 columns: which = 1 is a history created on the proposed lengths, which = 0 the state before"""
    c = TH.case("acgt")
    rate = np.asarray(c.omodel.sub_rate, dtype=np.float64)

    def create(length):
        return capi.History.from_lengths(c.parent, c.ins_prob, c.log_cpt_weight, c.tokens, rate, length)

    def batch(hist, which, mats):
        return hist.branch_batch([branch(c, r, mats=mats[r]) for r in nodes], which=which)

    def run(b):
        b.run(viterbi=False)
        out = [b.read_inputs(k) + (b.read_matrix(k),) for k in range(b.n)], b.lp_end()
        b.close()
        return out

    def equal(x, y):
        return same(x[1], y[1]) and all(same(a, b) for ja, jb in zip(x[0], y[0]) for a, b in zip(ja, jb))

    has_child = sorted(set(c.parent) - {-1, c.n - 1})
    node = has_child[0]
    changed = [node] + [r for r in range(c.n - 1) if c.parent[r] == node]
    nodes = changed + [c.parent[node], 0, c.n - 2]
    nodes = sorted(set(r for r in nodes if r < c.n - 1))
    proposed = list(c.length)
    for r, t in zip(changed, (.27, .41, .13)):
        proposed[r] = t
    h, fresh = create(c.length), create(proposed)
    old_mats = {r: h.branch_matrix(r) for r in nodes}
    new_mats = {r: fresh.branch_matrix(r) for r in nodes}
    old = run(batch(h, 0, old_mats))
    want = run(batch(fresh, 0, new_mats))
    assert not equal(old, want)
    state = h.log_like()
    h.propose_lengths(changed, [proposed[r] for r in changed])
    pending = h.log_like(1)
    assert all(same(h.branch_matrix(r, 1), new_mats[r]) for r in nodes)
    assert equal(run(batch(h, 1, new_mats)), want) and equal(run(batch(h, 0, old_mats)), old)
    now = h.log_like(0), h.log_like(1)
    assert now[0][0] == state[0] and now[0][1].tobytes() == state[1].tobytes()
    assert now[1][0] == pending[0] and now[1][1].tobytes() == pending[1].tobytes()
    h.accept()
    after = h.log_like()
    assert after[0] == pending[0] and after[1].tobytes() == pending[1].tobytes()
    assert equal(run(batch(h, 0, new_mats)), want)
    h.propose_lengths(changed, [c.length[r] for r in changed])
    assert equal(run(batch(h, 1, old_mats)), old)
    h.reject()
    still = h.log_like()
    assert still[0] == pending[0] and still[1].tobytes() == pending[1].tobytes()
    assert equal(run(batch(h, 0, new_mats)), want)
    h.close()
    fresh.close()


# ---- 6. lifetime and stream ----

def test_the_batch_outlives_the_history_and_a_delayed_stream_gives_the_same_bytes():
    SH.one_hip_runtime()
    SH.cycles_per_ms()
    c = TH.case("acgt")
    nodes = kinds_of_branches(c)
    jobs = [branch(c, r) for r in nodes]
    h = c.history()
    want = h.branch_batch(jobs)
    want.run(viterbi=True)
    streams = SH.Streams()
    try:
        a = streams.new()
        streams.busy(a)
        SH.assert_busy(a, "History.branch_batch")
        got = h.branch_batch(jobs, stream=SH.handle(a))
    finally:
        streams.release()
    first = [got.read_inputs(k) for k in range(got.n)]
    h.close()                                                        # the batch owns its inputs
    got.run(viterbi=True)
    for k in range(got.n):
        assert all(same(x, y) for x, y in zip(got.read_inputs(k), want.read_inputs(k))), k
        assert all(same(x, y) for x, y in zip(got.read_inputs(k), first[k])), k
        assert same(got.read_matrix(k), want.read_matrix(k)), k
    assert same(got.lp_end(), want.lp_end()) and got.best_paths() == want.best_paths()
    got.close()
    want.close()


# ---- 7. read_inputs on an ordinary batch ----

def test_read_inputs_of_an_uploaded_batch_returns_the_upload():
    rng = np.random.default_rng(3)
    jobs = []
    for x_len, y_len in ((5, 7), (0, 3), (4, 0), (65, 2)):
        xp, ys = rng.normal(size=(x_len, 2, 5)), rng.normal(size=(y_len, 2, 5))
        ys[ys > 1.] = -np.inf
        jobs.append((xp, ys, rng.normal(size=y_len), TRANS, None, None, -1))
    b = capi.BranchBatch(jobs)
    for k, (xp, ys, ye) in enumerate(j[:3] for j in jobs):
        got = b.read_inputs(k)
        assert same(got[0], xp.reshape(got[0].shape)) and same(got[1], ys.reshape(got[1].shape)) and same(got[2], ye)
    lib = capi.load()
    assert lib.hx_branch_batch_read_inputs(b._h, 0, None, None, None) == 0          # each may be NULL
    assert TH._code(lambda: b.read_inputs(4)) == capi.HX_ERR_RANGE and TH._code(lambda: b.read_inputs(-1)) == capi.HX_ERR_RANGE
    assert lib.hx_branch_batch_read_inputs(None, 0, None, None, None) == capi.HX_ERR_INVALID_ARG
    b.close()


# ---- 8. refusals ----

def test_every_refusal_and_that_nothing_ran():
    import ctypes as C
    c = TC._edge(6)
    h = c.history()
    ms, state = h.kernel_ms(), h.log_like()
    lib = capi.load()
    good = branch(c, 0)
    env = envelopes(c, 0)

    def code(branches, **kw):
        return TH._code(lambda: h.branch_batch(branches, **kw))
    for node in (-1, 6, 7):                                          # outside 0 .. N - 2: the root (6) has no branch
        assert code([(node,) + good[1:]]) == capi.HX_ERR_RANGE == -8
    assert code([good, (6,) + good[1:]]) == -8                       # one bad branch among good ones
    assert code([]) == capi.HX_ERR_INVALID_ARG == -1                 # no branches
    assert code([good], which=2) == -1 and code([good], which=-1) == -1
    assert code([good], which=1) == -7          # nothing is pending
    assert code([good[:4] + (env[0], None, 2)]) == -1 and code([good[:4] + (None, env[1], 0)]) == -1 and code([good[:4] + (None, None, 0)]) == -1
    # null pointers, straight at the C ABI: *out is null after every refusal
    arr = (capi.HxHistoryBranch * 1)()
    ls, li = np.ascontiguousarray(good[1]), np.ascontiguousarray(good[2])
    f64p = C.POINTER(C.c_double)

    def raw(hist, branches, n, sub=True, ins=True, out=True, which=0):
        arr[0].node = 0
        arr[0].log_sub = ls.ctypes.data_as(f64p) if sub else C.cast(None, f64p)
        arr[0].log_ins = li.ctypes.data_as(f64p) if ins else C.cast(None, f64p)
        arr[0].max_distance = -1
        got = C.c_void_p(12345)
        rc = lib.hx_history_branch_batch_create(hist, which, 1, arr if branches else None, n, None, C.byref(got) if out else None)
        assert rc != 0 and (not out or not got.value)
        return rc
    assert raw(None, True, 1) == -1 and raw(h._h, False, 1) == -1 and raw(h._h, True, 1, out=False) == -1
    assert raw(h._h, True, 1, sub=False) == -1 and raw(h._h, True, 1, ins=False) == -1
    assert raw(h._h, True, 0) == -1 and raw(h._h, True, -3) == -1
    assert raw(h._h, True, 1, which=1) == -7
    assert lib.hx_history_last_handoff_ms(h._h, None) == -1 and lib.hx_history_last_handoff_ms(None, None) == -1
    # a parent row of 64 * 1024 positions: leaves 0 and 1 under node 2, every column ungapped
    tokens = np.repeat(np.asarray([[0, 1, -1]], dtype=np.int8), 65536, axis=0)
    hb = capi.History([2, 2, -1], c.ins_prob, c.log_cpt_weight, tokens, c.branch_sub[:, :3])
    assert hb.row_lengths().tolist() == [64 * 1024] * 3
    assert TH._code(lambda: hb.branch_batch([good])) == capi.HX_ERR_RANGE
    hb.close()
    # no hx_init for the history's device
    capi.shutdown()
    assert code([good]) == -2
    capi.init(0, c_oracle.table())
    assert h.kernel_ms() == ms
    still = h.log_like()
    assert still[0] == state[0] and still[1].tobytes() == state[1].tobytes()
    # a good query afterwards
    check_branches(h, c, list(range(c.n - 1)), "after the refusals").close()
    assert h.kernel_ms() > 0
    h.close()
