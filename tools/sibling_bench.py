"""The sibling-pair parent-proposal DP (row N4's eleven-state lattice, hx_sibling.hip) on batches the size of
tools/branch_bench.py's: `jobs` pairs of child profiles of `length` positions over the 20-letter alphabet, one component, band
around the diagonal or none.  Prints, over `reps` timed runs behind a warm-up run (HIP events): the fill kernel's median time
and spread, every sample, Gcell/s, the fraction of the HBM roofline at 88 B/cell (eleven fp64 states), time per table
log_sum_exp (20 per cell), and the whole step - clearing, emission pre-pass and fill - next to it.
    python tools/sibling_bench.py [length] [jobs] [band] [reps]       (on the GPU box)"""
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from historian_amd import capi, hostmodel

LSE_PER_CELL = 20       # IIW 2, IIX 1, IMD 3, WWX 1; IMI 1, IDI 1, IDM 3, WWW 1, WXW 1; IMM 3, WWW 1; IDD 2 (hx_sibling.hip)
length = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
n = int(sys.argv[2]) if len(sys.argv) > 2 else 126
band = int(sys.argv[3]) if len(sys.argv) > 3 else -1
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 7
capi.init(0, hostmodel.lse_table())
rng = np.random.default_rng(3)
A = 20
pm = dict(ins=.1, dele=.1, ins_ext=.6, del_ext=.6)
T = hostmodel.sibling_trans(pm, pm, .6)
root = np.full((1, A), math.log(1. / A))
jobs = []
for k in range(n):
    ls = np.log(rng.dirichlet(np.ones(A) * .3, size=length)).reshape(length, 1, A)
    rs = np.log(rng.dirichlet(np.ones(A) * .3, size=length)).reshape(length, 1, A)
    env = np.arange(length + 1, dtype=np.int32) if band >= 0 else None
    emit = np.full(length, math.log(1. / A))
    jobs.append((ls, rs, root, emit, emit, T, env, env, band))
b = capi.SiblingBatch(jobs)
cells = b.total_cells()
if band >= 0:
    cells = n * sum(min(length, i + band) - max(0, i - band) + 1 for i in range(length + 1))
b.run()
b.lp_end()
fills, steps = [], []
for _ in range(reps):
    b.run()
    lp = b.lp_end()
    f, s = b.kernel_ms()
    fills.append(f)
    steps.append(s)
ms, st = statistics.median(fills), statistics.median(steps)
print("%d sibling pairs of %d x %d, band %s: fill kernel %.2f ms (min %.2f, max %.2f over %d runs) = %.2f Gcell/s (%.3f of the HBM "
      "roofline at 88 B/cell), %.2f ps per table log_sum_exp at %d per cell; whole step (clear + emission + fill) %.2f ms "
      "(min %.2f, max %.2f) = %.2f Gcell/s (%.3f); lpEnd[0] %.4f; fill samples %s; step samples %s"
      % (n, length, length, band if band >= 0 else "none", ms, min(fills), max(fills), reps, cells / ms / 1e6,
         cells * 88 / (ms * 1e-3) / 8e12, ms * 1e9 / (cells * LSE_PER_CELL), LSE_PER_CELL, st, min(steps), max(steps),
         cells / st / 1e6, cells * 88 / (st * 1e-3) / 8e12, lp[0], " ".join("%.4f" % f for f in fills), " ".join("%.4f" % f for f in steps)))
b.close()
