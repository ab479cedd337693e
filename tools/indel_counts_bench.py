"""Cost of the carried indel counts (hx_batch_event_counts) next to the Forward and Backward fills of the same pairs.
  indel_counts_bench.py [reps] [fast|exact|trunc]: the gp120 family's six general-profile internal-node pairs (oracle-built
    profiles, as dag_bench.py) x reps, unbanded and with the reference's band of 20, one call per pair.  The wall times include
    each call's copies and sync; "bandwidth at wall time" divides the 80 bytes a lattice cell must be read with (Forward and
    Backward, five states each) by that wall time - it is not a kernel figure: run the tool under
    `rocprofv3 --kernel-trace --stats` for the kernels' own times (k_event_posts, k_event_finish).
  indel_counts_bench.py recon [n_leaves] [length] [model]: a recon_batch_bench.py-shaped family (32 x 1000 aa, WAG by
    default) through bin/hxrecon, as a plain reconstruction and with `count indel` (Backward fill + counts at the root instead
    of the root traceback); under rocprofv3 the root pair's k_event_posts stands next to its own fill kernels."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from historian_amd import capi
from oracle import c_oracle, historian_oracle as ho
from tests import helpers as H, recon_helpers as R

HBM_PEAK_GBS = 8000.0
G = os.path.join(ROOT, "tests", "golden", "reference_data") + os.sep
LG = os.path.join(ROOT, "tests", "golden", "models", "lg.json")
if len(sys.argv) > 1 and sys.argv[1] == "recon":
    import subprocess, tempfile
    n_leaves = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    length = int(sys.argv[3]) if len(sys.argv) > 3 else 1000
    MODEL = os.path.join(ROOT, "tests", "golden", "models", (sys.argv[4] if len(sys.argv) > 4 else "wag") + ".json")
    tree, seqs = R.balanced_family(n_leaves, length, "arndcqeghilkmfpstwyv", seed=21, branch=.05)
    exe = os.path.join(ROOT, "historian_amd", "bin", "hxrecon")
    with tempfile.TemporaryDirectory() as d:
        for label, opts in (("reconstruction", {}), ("count indel", {"count": "indel"})):
            job = os.path.join(d, "job.txt")
            R.write_job(job, MODEL, tree, seqs, {}, os.path.join(d, "s.fa"), os.path.join(d, "g.fa"), samples=10, **opts)
            t0 = time.perf_counter()
            out = subprocess.run([exe, job], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=1500)
            assert out.returncode == 0, out.stderr.decode()[-2000:]
            print("%d leaves x %d residues, %s: %.3f s wall" % (n_leaves, length, label, time.perf_counter() - t0))
            for line in out.stdout.decode().splitlines():
                if line.startswith("indelCountsTotal"):
                    print("   ", line)
    sys.exit(0)
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 16
policy = sys.argv[2] if len(sys.argv) > 2 else "fast"
flags = {"fast": capi.HX_LSE_FAST, "exact": capi.HX_LSE_EXACT, "trunc": capi.HX_LSE_TRUNC}[policy]
tree, seqs, guide = R.load_family(G + "gp120.tree.nh", G + "gp120.fa", G + "gp120.guide.fa")
res, rows = R.oracle_reconstruct(LG, tree, seqs, guide, max_distance_from_guide=20)
model = ho.RateModel.from_file(LG); model.sub_rate = [m.tolist() for m in model.sub_rate]
closest = ho.closest_leaves(tree)
capi.init(0, c_oracle.table())
rng = np.random.default_rng(5)
for band in (-1, 20):
    imgs, times = [], []
    for node in range(tree.nodes()):
        if tree.is_leaf(node): continue
        lc, rc = tree.child[node]
        if tree.is_leaf(lc) and tree.is_leaf(rc): continue
        tl, tr = tree.branch_length[lc], tree.branch_length[rc]
        lp = ho.ProbModel(model, tl, [ho.sub_prob_matrix_ss(sr, tl) for sr in model.sub_rate])
        rp = ho.ProbModel(model, tr, [ho.sub_prob_matrix_ss(sr, tr) for sr in model.sub_rate])
        env = ho.GuideAlignmentEnvelope(guide, closest[lc], closest[rc], band) if band >= 0 else ho.GuideAlignmentEnvelope()
        f = ho.ForwardMatrix(res["prof"][lc], res["prof"][rc], ho.PairHMM(lp, rp, model.ins_prob), node, env, fill=False)
        imgs.append(H.job_images(f))
        times.append([tl, tr, .5 * tl, .5 * tl, .5 * tr, .5 * tr])
    imgs, times = imgs * reps, times * reps
    b = capi.Batch(imgs, capi.HX_KEEP_BACKWARD | flags)
    b.forward(); b.sync(); b.forward(); b.sync()
    fms = b.kernel_ms(0)
    b.backward(); b.sync(); b.backward(); b.sync()
    bms = b.kernel_ms(1)
    tables = [(rng.random((len(x.trans_src), 6)), rng.random((len(y.trans_src), 6))) for x, y, _, _ in imgs]
    for k in range(len(imgs)):                                  # warm-up: one call per pair
        b.event_counts(k, times[k], *tables[k])
    t0 = time.perf_counter()
    for k in range(len(imgs)):
        b.event_counts(k, times[k], *tables[k])
    cms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    for k in range(len(imgs)):
        b.indel_counts(k, times[k])
    ims = (time.perf_counter() - t0) * 1e3
    cells = b.total_cells()
    print("band %3d, %d pairs, %s: Forward fill %.3f ms, Backward fill %.3f ms (whole batch, kernels); "
          "event counts %.3f ms for all pairs one call each (wall, with copies / sync: %.1f us per pair), "
          "80 B x %d lattice cells at wall time = %.3f of the HBM peak (not a kernel figure); hx_batch_indel_counts %.3f ms (wall)" %
          (band, len(imgs), policy, fms, bms, cms, cms * 1e3 / len(imgs), cells, cells * 80 / (cms * 1e-3) / 1e9 / HBM_PEAK_GBS, ims))
    sys.stdout.flush()
    b.close()
capi.shutdown()
