"""The walks through device-resident pair matrices (hx_pairdp.h: k_pair_walk, one wavefront per job) against what they
replace, on the batches of tools/sibling_bench.py: `jobs` pairs of profiles of `length` positions over the 20-letter alphabet,
one component, band around the diagonal or none, for the eleven-state (sibling) or the three-state (branch) lattice.
Behind a warm-up, `reps` runs each, median [min, max]:
  * sample_paths of the whole batch (and best_paths for the branch lattice): the call (allocation, copies, kernel, host clock
    around it - it ends in a synchronise) and the kernel alone (HIP events), microseconds per step; the same for a lone job;
  * the parent commit's path to a walk: read_matrix of every job into page-locked memory (hx_host_alloc) - what a host walk
    needs before it can start - and of a lone job.
    python tools/walks_bench.py sibling|branch [length] [jobs] [band] [reps]       (on the GPU box)
The mirror's side (fillBatch + walks with and without HX_HOST_WALKS=1) is `hxtest walktime`, driven by
    python tools/walks_bench.py mirror [length] [matrices] [band]"""
import ctypes as C
import math
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from historian_amd import capi, hostmodel

lattice = sys.argv[1] if len(sys.argv) > 1 else "sibling"
length = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
n = int(sys.argv[3]) if len(sys.argv) > 3 else 126
band = int(sys.argv[4]) if len(sys.argv) > 4 else -1
reps = int(sys.argv[5]) if len(sys.argv) > 5 else 7


def spread(v):
    return "%.3f [%.3f, %.3f]" % (statistics.median(v), min(v), max(v))


if lattice == "mirror":
    rng = np.random.default_rng(5)
    letters = "arndcqeghilkmfpstwyv"
    with tempfile.TemporaryDirectory() as d:
        fa = os.path.join(d, "pair.fa")
        with open(fa, "w") as f:
            for name in "xy":
                f.write(">%s\n%s\n" % (name, "".join(letters[k] for k in rng.integers(20, size=length))))
        cmd = [os.path.join(ROOT, "historian_amd", "bin", "hxtest"), "walktime", fa, os.path.join(ROOT, "tests", "golden", "models", "lg.json"),
               "0.3", "0.5", str(n)] + ([str(band)] if band >= 0 else [])
        for host in (False, True):
            env = dict(os.environ)
            env.pop("HX_HOST_WALKS", None)
            if host:
                env["HX_HOST_WALKS"] = "1"
            print("mirror, band %s, %s:" % (band if band >= 0 else "none", "HX_HOST_WALKS=1 (host walks over dense copies)" if host else "device walks"))
            sys.stdout.flush()
            subprocess.run(cmd, env=env, check=True, timeout=500)
    sys.exit(0)

capi.init(0, hostmodel.lse_table())
rng = np.random.default_rng(3)
A = 20
env = np.arange(length + 1, dtype=np.int32) if band >= 0 else None
emit = np.full(length, math.log(1. / A))


def profile():
    return np.log(rng.dirichlet(np.ones(A) * .3, size=length)).reshape(length, 1, A)


if lattice == "sibling":
    pm = dict(ins=.1, dele=.1, ins_ext=.6, del_ext=.6)
    T = hostmodel.sibling_trans(pm, pm, .6)
    root = np.full((1, A), math.log(1. / A))
    jobs = [(profile(), profile(), root, emit, emit, T, env, env, band) for _ in range(n)]
    make, states, words_per_job = capi.SiblingBatch, 11, 10 * length + 16
else:
    T = [[math.log(v) if v > 0 else -math.inf for v in row] for row in [[.9 * .9, .1, .9 * .1, .9], [.4 * .9, .6, .4 * .1, .4], [.4, 0., .6, .4]]]
    jobs = [(profile(), profile(), emit, T, env, env, band) for _ in range(n)]
    make, states, words_per_job = capi.BranchBatch, 3, 2 * length + 16
lib = capi.load()
lib.hx_host_alloc.argtypes = [C.c_size_t, C.POINTER(C.c_void_p)]
lib.hx_host_free.argtypes = [C.c_void_p]
pinned = C.c_void_p()
assert lib.hx_host_alloc(8 * states * (length + 1) ** 2, C.byref(pinned)) == 0
read_matrix = getattr(lib, "hx_%s_batch_read_matrix" % lattice)
title = "%s lattice, band %s" % (lattice, band if band >= 0 else "none")


def measure(b, what):
    nj = b.n
    shape = "%d x (%d x %d)" % (nj, length, length)
    words = [rng.integers(0, 2 ** 32, size=words_per_job, dtype=np.uint64).astype(np.uint32) for _ in range(nj)]
    modes = [("sample_paths", lambda: b.sample_paths(words, raw=True)[1])]
    if lattice == "branch":
        modes.append(("best_paths", lambda: b.best_paths(raw=True)[1]))
    for name, call in modes:
        if lattice == "branch":
            b.run(viterbi=name == "best_paths")
        else:
            b.run()
        b.lp_end()
        steps = call()                        # warm-up
        assert (steps > 0).all(), steps
        calls, kernels = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            call()
            calls.append((time.perf_counter() - t0) * 1e3)
            kernels.append(b.walk_ms())
        k = statistics.median(kernels)
        print("%s, %s, %s %s: call %s ms, kernel %s ms; %d steps in all, longest walk %d: %.3f us per step of the longest walk, "
              "%.4f us per step over the batch" % (title, what, name, shape, spread(calls), spread(kernels), steps.sum(), steps.max(),
                                                    k * 1e3 / steps.max(), k * 1e3 / steps.sum()))
    # what a host walk needs first on the parent commit: every matrix dense, in page-locked memory
    reads = []
    for r in range(reps + 1):
        t0 = time.perf_counter()
        for job in range(nj):
            assert read_matrix(b._h, job, C.cast(pinned, C.POINTER(C.c_double))) == 0
        if r:
            reads.append((time.perf_counter() - t0) * 1e3)
    gb = nj * 8 * states * (length + 1) ** 2 / 1e9
    print("%s, %s, read_matrix of every job into page-locked memory %s: %s ms for %.2f GB = %.1f GB/s"
          % (title, what, shape, spread(reads), gb, gb / (statistics.median(reads) * 1e-3)))
    sys.stdout.flush()


whole = make(jobs)
measure(whole, "full batch")
whole.close()
lone = make(jobs[:1])
measure(lone, "lone job")
lone.close()
lib.hx_host_free(pinned)
