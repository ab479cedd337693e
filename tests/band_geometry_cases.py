"""The geometry families of the banded-fill tests: leaf pairs (and four-leaf profile pairs) banded round the true
alignment of a simulated history, so that the envelope has what real guide alignments have and a left-justified guide
never does - long gap runs, leading and trailing gaps, blocks with no match at all, rows of 99 in-envelope columns next to
rows of 5, a hundred rows sharing one span.  Shared by tests/test_oracle_band_geometry.py (which pins the yardstick on
them) and tests/test_gpu_band_geometry.py.

An event `p: +n` is an n-residue y-only run before x residue p (between rows p and p + 1 of the matrix; row i is x state i,
state 0 is START), `p: -n` an n-residue x-only run over rows p + 1 .. p + n."""
import functools

import numpy as np

from oracle import historian_oracle as ho
from tests import helpers as H

AA = "arndcqeghilkmfpstwyv"

# name -> (lx, events, band, keyword arguments of H.guided_leaf_case)
FAMILIES = {
    "long_y_run": (150, {40: +90}, 4, {}),
    "long_x_run": (200, {60: -100}, 4, {}),
    "staircase": (260, {30: +40, 80: -50, 150: +70, 200: -30}, 6, {}),
    "leading_y_run": (140, {0: +80}, 3, {}),
    "band0_runs": (130, {50: +20, 90: -25}, 0, {}),
    "no_match": (70, {0: +60, 1: -69}, 5, {}),
    "trailing_x_run": (180, {100: -80}, 4, {}),
    "trailing_y_run": (120, {120: +85}, 3, {}),
    "unaligned_70_80": (200, {60: -70, 130: +80}, 5, {}),
    "unaligned_40_40": (200, {80: -40, 120: +40}, 5, {}),
    "x_runs_across_64_128": (260, {30: -70, 120: -70}, 4, {}),         # rows 31..100 and 121..190
    "y_runs_at_64_128": (170, {63: +40, 127: +35}, 3, {}),             # between rows 63 | 64 and 127 | 128
    "y_runs_mod4": (200, {20: +10, 41: +12, 62: +9, 83: +14, 104: +8, 125: +11, 146: +13, 167: +10}, 2, {}),   # after rows = 0, 1, 2, 3 (mod 4)
    "band_over_both": (80, {20: +10, 40: -8}, 400, {}),
    "protein": (150, {40: +50, 100: -40}, 5, dict(alphabet=AA, jc=False, tl=.3, tr=.2)),
    "two_components": (140, {30: -45, 90: +60}, 4, dict(components=2, jc=False)),
}
SEED = 7
WHOLE = ("no_match", "band_over_both")          # every cell is inside the envelope
SMALL = ("band0_runs", "no_match", "band_over_both", "long_y_run")      # ... the Python oracle fills in about a second


@functools.lru_cache(maxsize=None)
def leaf(name):
    """(unfilled oracle ForwardMatrix, job image) of a family; built once per process, never modified"""
    lx, events, band, kw = FAMILIES[name]
    f = H.guided_leaf_case(SEED, lx, events, band, **kw)
    return f, H.job_images(f)


@functools.lru_cache(maxsize=None)
def mask(name):
    m = H.envelope_mask(leaf(name)[0])
    m.setflags(write=False)
    return m


def band_mask(f):
    """[R][Cc] bool: within max_distance of the guide (the envelope without its always-inside row and column)"""
    return np.array([[f.envelope.in_range(f.x_closest_leaf_pos[i], f.y_closest_leaf_pos[j]) for j in range(f.y_size - 1)]
                     for i in range(f.x_size - 1)], dtype=bool)


def run_corners(name):
    """cells just inside and just outside the envelope at every corner of its outline: all (i, j) where the band's first or
    last column changes from one row to the next, with their eight neighbours, clipped to the matrix"""
    f = leaf(name)[0]
    bm = band_mask(f)
    R, Cc = bm.shape
    lo = np.array([np.argmax(r) for r in bm])
    hi = np.array([Cc - 1 - np.argmax(r[::-1]) for r in bm])
    out = set()
    for i in range(1, R):
        for a, b in ((lo[i - 1], lo[i]), (hi[i - 1], hi[i])):
            if a != b:
                for ii in (i - 1, i):
                    for jj in (a, b):
                        out.update((ii + di, jj + dj) for di in (-1, 0, 1) for dj in (-1, 0, 1))
    out.update([(0, 0), (R - 1, Cc - 1), (1, Cc - 1), (R - 1, 0), (0, Cc - 1)])
    return np.array(sorted((i, j) for i, j in out if 0 <= i < R and 0 <= j < Cc), dtype=np.int32)


# name -> (n, events of the four leaves): x profiles of one strip of 64 rows, and of three or four
DAG_FAMILIES = {
    "dag_one_strip": (25, ({6: +10}, {}, {12: -10}, {20: +8})),
    "dag_three_strips": (110, ({20: +30}, {}, {50: -25}, {70: +15})),
}


@functools.lru_cache(maxsize=None)
def _dag_profiles(name, samples, keep_all):
    n, events = DAG_FAMILIES[name]
    return H.guided_dag_case(SEED, n, events, 0, samples, keep_all=keep_all)


@functools.lru_cache(maxsize=None)
def dag(name, band, samples, keep_all=False):
    """(unfilled oracle ForwardMatrix, job image): H.guided_dag_case(SEED, n, events, band, samples, keep_all), with the
    profiles (which do not depend on the band) built once"""
    g = _dag_profiles(name, samples, keep_all)
    f = ho.ForwardMatrix(g.x, g.y, g.hmm, 6, ho.GuideAlignmentEnvelope(g.guide, 0, 2, band), fill=False)
    f.guide, f.seqs = g.guide, g.seqs
    return f, H.job_images(f)
