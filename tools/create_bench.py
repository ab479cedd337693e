"""Host cost of making and destroying batches: hx_batch_create / hx_batch_destroy of leaf pairs (unbanded and banded) and
hx_quick_batch_create / hx_quick_batch_destroy, timed around the C ABI calls alone (the job arrays are built once).  Every job
of a batch points at the same profiles, so the figures are the library's work per job, not Python's.
(tools/alloc_bench.py times raw hipMalloc / hipFree and never loads the library: it says nothing about a change to batch creation.)
usage: python tools/create_bench.py [--pairs N] [--len L] [--reps R]      (HX_LIB_PATH selects another build of the library)
Prints one JSON line: medians and ranges in milliseconds."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from historian_amd import capi                       # noqa: E402
from oracle import c_oracle                          # noqa: E402
from tests import helpers as H                       # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=512)
ap.add_argument("--len", type=int, default=300, dest="length")
ap.add_argument("--reps", type=int, default=20)
args = ap.parse_args()

capi.init(0, c_oracle.table())
lib = capi.load()


def timed(create, destroy):
    made, gone = [], []
    for _ in range(args.reps + 1):
        h = C.c_void_p()
        t0 = time.perf_counter()
        rc = create(C.byref(h))
        t1 = time.perf_counter()
        assert rc == 0, lib.hx_last_error()
        destroy(h)
        t2 = time.perf_counter()
        made.append((t1 - t0) * 1e3)
        gone.append((t2 - t1) * 1e3)
    summary = lambda v: dict(median=float(np.median(v[1:])), min=min(v[1:]), max=max(v[1:]))      # (the first round loads kernels)
    return dict(create_ms=summary(made), destroy_ms=summary(gone))


out = dict(pairs=args.pairs, length=args.length, reps=args.reps, lib=capi.LIB_PATH)
for name, band in (("leaf", None), ("leaf_banded", 8)):
    img = H.job_images(H.leaf_case(5, args.length, args.length, band=band))
    jobs = capi.make_jobs([img] * args.pairs)
    out[name] = timed(lambda h: lib.hx_batch_create(jobs, args.pairs, capi.HX_LSE_TRUNC | capi.HX_KEEP_BACKWARD, h), lib.hx_batch_destroy)
rng = np.random.default_rng(1)
x, y = rng.integers(0, 4, args.length), rng.integers(0, 4, args.length)
qb = capi.QuickBatch([(x, y, 4, rng.normal(size=(4, 4)), [-.5] * 11, np.arange(-20, 21))] * args.pairs)
out["quick"] = timed(lambda h: lib.hx_quick_batch_create(qb._jobs, args.pairs, h), lib.hx_quick_batch_destroy)
qb.close()
capi.shutdown()
print(json.dumps(out))
