"""One small multiply for every ahead-of-time instance of the multiply kernel families that are instantiated from lists, and for the run-time compiled
class kernels of tests/test_gpu_class_mode.py's SHAPES.  The tables are built from the source, not from a copy of it: DBCSR_AMD_MID_SHAPES is parsed out
of dbcsr_amd/csrc/mm_choose.h, the ranges of mm_numeric_f64_big<TM,TN> and mm_numeric_z64<MA,NC> out of big_f64_has and z64_has -- an instance added
there has no case here until somebody writes one, and tests/test_kernel_instances_cpu.py fails until then.  No torch, no device library: this module is
imported by the CPU test (which checks every row against the choice rules and the oracle) and by tests/test_gpu_kernel_instances.py (which runs them).

A case is an oracle.perf_case tuple (M, N, K, sparsity A, B, C, mix m, mix n, mix k) with uniform block sizes and ONE smaller tail block in every
dimension: the C blocks of the tail row / column go through the family's other path (the slab kernels' second launch <10,10> / <12,12>, the workgroup
kernel's smaller blocks), so that path is part of every case.  The matrices have five or six block rows and columns: the oracle takes milliseconds.
"""
import ast
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHOOSE_H = os.path.join(ROOT, "dbcsr_amd", "csrc", "mm_choose.h")


# ---- the instance lists, from the source -----------------------------------------------------------------------------------------------------------
def _source():
    with open(CHOOSE_H) as fh:
        return fh.read()


def mid_shapes():
    """the (rows, columns) in units of 4 of DBCSR_AMD_MID_SHAPES, in the order of the macro"""
    body = re.search(r"#define DBCSR_AMD_MID_SHAPES\(X\)((?:.*\\\n)*.*)\n", _source()).group(1)
    return [(int(a), int(b)) for a, b in re.findall(r"X\(\s*(\d+)\s*,\s*(\d+)\s*\)", body)]


def _square_range(function, a, b):
    """the pairs a function of the form `return a >= LO && a <= HI && b >= LO && b <= HI;` answers yes for"""
    m = re.search(r"static inline bool %s\(int %s, int %s\) \{ return (.*?); \}" % (function, a, b), _source())
    lo_a, hi_a, lo_b, hi_b = [int(v) for v in re.fullmatch(r"%s >= (\d+) && %s <= (\d+) && %s >= (\d+) && %s <= (\d+)" % (a, a, b, b), m.group(1)).groups()]
    return [(x, y) for x in range(lo_a, hi_a + 1) for y in range(lo_b, hi_b + 1)]


def big_shapes():
    return _square_range("big_f64_has", "tm", "tn")


def z64_shapes():
    return _square_range("z64_has", "ma", "nc")


def mid_serves(m, n, class_mode):
    """mm_choose.h: mid_f64_serves, restated for the class cases (which classes of a mixed-size multiply take the slab kernel); the CPU test holds it
    against the header through the choice of uniform sizes"""
    rb, cb = (m + 3) // 4, (n + 3) // 4
    lo, hi = min(rb, cb), max(rb, cb)
    if lo < 6 or hi > 12 or hi < 8:
        return False
    if hi >= 11:
        return lo <= 10 or (m % 4 == 0 and n % 4 == 0)
    if hi >= 9:
        return True
    return class_mode > 0 and (lo == 8 or (lo == 6 and class_mode != 3))


# ---- sparsities ---------------------------------------------------------------------------------------------------------------------------------------
# The pattern of a random matrix depends on its block counts, its sparsity and its place in the case (oracle.random_pattern), not on the block sizes.
# Per (block rows, block columns, inner blocks): sparsities of A, B, C with which the C blocks of the instance's own size have product lists of length
# 0, 1, 2 and >= 3 (the kernels' look-ahead -- p2, i2, have_first -- has a branch for each) and C_in holds some of the product's blocks and lacks
# others (cin_off >= 0 and < 0).  The CPU test asserts both from the reference's patterns.
SPARSITY = {
    (6, 6, 8): [(0.5, 0.5, 0.5), (0.5, 0.6, 0.4), (0.5, 0.65, 0.5), (0.5, 0.55, 0.6)],
    (6, 6, 10): [(0.5, 0.6, 0.6), (0.5, 0.5, 0.5)],
    (5, 5, 8): [(0.5, 0.5, 0.5), (0.5, 0.55, 0.4), (0.55, 0.5, 0.5), (0.5, 0.65, 0.6)],
}


def _nblocks(total, size):
    return (total + size - 1) // size


def _case(M, N, K, m, n, k, salt):
    sp = SPARSITY[(_nblocks(M, m), _nblocks(N, n), _nblocks(K, k))]
    spa, spb, spc = sp[salt % len(sp)]
    return (M, N, K, spa, spb, spc, [1, m], [1, n], [1, k])


# ---- the slab kernels mm_numeric_f64_mid<RB,CB> -----------------------------------------------------------------------------------------------------
MID_K = [1, 5, 8, 9, 17, 23, 33, 40]   # slab tails (k mod 8, k mod 4), one slab, more than one
MID_CLASS_SHAPES = [(8, 8), (8, 6), (6, 8)]   # both dimensions within 32: taken only as (m, n) classes of a mixed-size multiply (mid_f64_serves)


def mid_cases():
    """{id: (case, (rb, cb))}: per instance "least" (4 rb - 3, 4 cb - 3: one row and one column in the last 4 x 4 unit) and "full" (4 rb, 4 cb);
    from 11 units in both dimensions on the choice wants multiples of 4 ("full" only).  M = 5 m + 5, N = 5 n + 6, seven inner blocks and a tail of 3."""
    out, i = {}, 0
    for rb, cb in mid_shapes():
        if (rb, cb) in MID_CLASS_SHAPES:
            continue
        for kind in ("least", "full"):
            if kind == "least" and min(rb, cb) >= 11:
                continue
            m, n = (4 * rb - 3, 4 * cb - 3) if kind == "least" else (4 * rb, 4 * cb)
            k = MID_K[i % len(MID_K)]
            out["%dx%d-%s-k%d" % (rb, cb, kind, k)] = (_case(5 * m + 5, 5 * n + 6, 7 * k + 3, m, n, k, i), (rb, cb))
            i += 1
    return out


def mid_class_cases():
    """{id: (case, (rb, cb))}: one multiply of blocks within 32 per class-mode shape, run with DBCSR_AMD_MM_CLASSES=2.  Row sizes {m, 5}, column sizes
    {n, 6}: of the four (m, n) classes only (m, n) itself is one mid_serves answers yes for, so "1 slab" in the kernel's name is that class."""
    out = {}
    for i, (rb, cb) in enumerate(MID_CLASS_SHAPES):
        m, n, k = 4 * rb - 3, 4 * cb - 3, (13, 9, 23)[i]
        out["%dx%d-class-k%d" % (rb, cb, k)] = (_case(5 * m + 5, 5 * n + 6, 7 * k + 3, m, n, k, i), (rb, cb))
    return out


# ---- the workgroup kernels mm_numeric_f64_big<TM,TN> --------------------------------------------------------------------------------------------------
BIG_M = {2: 13, 3: 45, 4: 53, 5: 69}   # ceil(m / 8) = 2, 6, 7, 9 tiles: both parities between the two wave rows
BIG_N = {2: 19, 3: 47, 4: 61, 5: 77}
BIG_K = [5, 16, 17, 33, 20, 37, 41]    # k mod 16 and k mod 4 vary


def big_cases():
    """{id: (case, (tm, tn))}: M = 4 m + 3, N = 4 n + 2, seven inner blocks and a tail of 3; <2,2> needs an inner size above 32 to leave the kernels of
    the blocks within 32"""
    out = {}
    for i, (tm, tn) in enumerate(big_shapes()):
        m, n, k = BIG_M[tm], BIG_N[tn], BIG_K[i % len(BIG_K)]
        if max(m, n) <= 32 and k <= 32:
            k = [v for v in BIG_K if v > 32][i % 3]
        out["%dx%d-k%d" % (tm, tn, k)] = (_case(4 * m + 3, 4 * n + 2, 7 * k + 3, m, n, k, i), (tm, tn))
    return out


# ---- the complex kernels mm_numeric_z64<MA,NC> --------------------------------------------------------------------------------------------------------
Z64_SIZE = {1: 5, 2: 13, 3: 23, 4: 32}
Z64_K = [1, 7, 8, 9, 23]


def z64_cases():
    """{id: (arguments of complex_case (tests/test_gpu_complex_multiply.py) without the seed, (ma, nc))}: one case per instance, and <4,1> / <1,4> once
    more with the large side at 45 (a dimension above 32 is covered in several tiles of 32)"""
    out = {}
    rows = [(ma, nc, Z64_SIZE[ma], Z64_SIZE[nc]) for ma, nc in z64_shapes()] + [(4, 1, 45, 5), (1, 4, 5, 45)]
    for i, (ma, nc, m, n) in enumerate(rows):
        k = Z64_K[i % len(Z64_K)]
        out["%dx%d-%dx%d-k%d" % (ma, nc, m, n, k)] = ((4 * m + max(1, m // 3), 4 * n + max(1, n // 2), 5 * k + 3, (0.3, 0.3, 0.5), [1, m], [1, n], [1, k]), (ma, nc))
    return out


# ---- the run-time compiled class kernels ----------------------------------------------------------------------------------------------------------------
def class_shapes():
    """SHAPES of tests/test_gpu_class_mode.py.  That module imports torch and the device library, so the list is read from its source; the GPU test
    holds it against the imported list."""
    with open(os.path.join(ROOT, "tests", "test_gpu_class_mode.py")) as fh:
        tree = ast.parse(fh.read())
    for node in tree.body:
        if isinstance(node, ast.Assign) and [t.id for t in node.targets if isinstance(t, ast.Name)] == ["SHAPES"]:
            return [tuple(s) for s in ast.literal_eval(node.value)]
    raise LookupError("tests/test_gpu_class_mode.py: no SHAPES")


CLASS_TAIL_RULE = "tail = lambda s, salt: 1 + (s * 7 + salt) % (s - 1)"   # test_class_kernels_at_scale_with_tails; the CPU test looks for this line there


def class_tail(s, salt):
    return 1 + (s * 7 + salt) % (s - 1)


def class_cases():
    """{id: (case, (m, n, k))}: (8 m + tail, 7 n + tail, 6 k + tail), run with DBCSR_AMD_MM_CLASSES=2"""
    out = {}
    for m, n, k in class_shapes():
        out["%dx%dx%d" % (m, n, k)] = ((8 * m + class_tail(m, 1), 7 * n + class_tail(n, 2), 6 * k + class_tail(k, 3), 0.5, 0.5, 0.5, [1, m], [1, n], [1, k]), (m, n, k))
    return out


# ---- what the reference says about a case -------------------------------------------------------------------------------------------------------------
def block_pattern(M):
    P = np.zeros((M.nbr, M.nbc), bool)
    P[M.rows(), M.col_i] = True
    return P


def product_list_lengths(A, B, ref, m, n):
    """lengths of the product lists of the blocks of `ref` (the reference's product) of size m x n, from the operands' patterns"""
    L = block_pattern(A).astype(np.int64) @ block_pattern(B).astype(np.int64)
    rows = ref.rows()
    own = (ref.row_sizes[rows] == m) & (ref.col_sizes[ref.col_i] == n)
    return L[rows[own], ref.col_i[own]]


def block_norms(M):
    """Frobenius norms of M's blocks"""
    rows = M.rows()
    size = M.row_sizes[rows].astype(np.int64) * M.col_sizes[M.col_i]
    return np.sqrt(np.array([np.sum(M.data[p:p + s] ** 2) for p, s in zip(M.blk_p, size)]))


FILTER_ALPHA, FILTER_BETA = 0.7, 1.3


def filter_eps(full):
    """A threshold for the filtered multiply of a case, from the block norms of the reference's unfiltered product `full`: the middle (geometric) of the
    widest gap between consecutive norms in the middle third of the sorted norms -- about half of the blocks survive and none sits near the threshold"""
    norms = np.sort(block_norms(full))
    lo, hi = len(norms) // 3, (2 * len(norms)) // 3
    gap = np.argmax(norms[lo + 1:hi + 1] / norms[lo:hi]) + lo
    return float(np.sqrt(norms[gap] * norms[gap + 1]))
