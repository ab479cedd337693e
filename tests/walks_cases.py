"""The inputs of the walk tests, in one place: tests/test_gpu_walks.py compares the device's walks with the restatement's on
these cases and word streams, and tests/test_oracle_walks.py checks on the CPU that every one of them keeps random_key_log's
running variate at least 1e-12 (relative to norm) away from zero - the precondition under which a walk cannot depend on the
last bits of exp().  A case added to a list here is covered by both."""
from oracle import branch_oracle as bo
from tests import sibling_ref as sr
from tests import walks_ref as wr
from tests.test_gpu_branch import random_branch

# (seed, parent, child, components, alphabet, band, one-hot columns): 1 and 4 components, alphabets 4 and 20, bands none / 3 /
# 20, empty and one-residue sequences, several strips
BRANCH_CASES = [(101, 5, 7, 1, 4, None, False), (102, 70, 66, 4, 4, None, False), (103, 130, 90, 1, 20, 3, True),
                (104, 200, 180, 1, 4, 20, False), (105, 0, 3, 1, 4, None, False), (106, 3, 0, 4, 4, None, False),
                (107, 1, 1, 1, 4, None, False), (108, 0, 0, 1, 4, None, False), (109, 63, 129, 1, 4, 3, True),
                (110, 257, 140, 1, 4, None, False)]
# (seed, left, right, components, alphabet, band, one-hot columns, envelope coordinates non-decreasing)
SIBLING_CASES = [(201, 5, 7, 1, 4, None, False, True), (202, 70, 66, 4, 4, None, False, True), (203, 130, 90, 1, 20, 3, True, True),
                 (204, 150, 150, 1, 4, 20, False, False), (205, 0, 3, 1, 4, None, False, True), (206, 3, 0, 4, 20, 0, True, True),
                 (207, 1, 1, 1, 4, None, False, True), (208, 0, 0, 1, 4, None, False, True), (209, 63, 129, 4, 4, 3, True, True),
                 (210, 200, 130, 1, 4, None, False, True)]
STREAMS = 3          # word streams per case: stream q of case k is mt19937 seeded 7000 + 10 k + q


def words(k, q, nx, ny):
    # enough for any walk: at most 3 (nx + ny) + 3 steps (include/historian_hip.h), two more words at each visit of IDD
    return wr.mt_words(7000 + 10 * k + q, 6 * (nx + ny) + 16)


def branch_matrix(c, viterbi=False):
    x, ysub, yemit, T, xe, ye, md = case = random_branch(*c)
    return case, bo.BranchMatrix(x, ysub, yemit, T, None if xe is None else list(xe), None if ye is None else list(ye), md, viterbi=viterbi)


def sibling_matrix(c):
    seed, nx, ny, C, A, band, one_hot, sorted_env = c
    case = sr.random_case(seed, nx, ny, C=C, A=A, band=band, one_hot=one_hot, sorted_env=sorted_env)
    return case, sr.SiblingMatrix(**case)
