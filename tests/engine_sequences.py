"""One long-lived engine through mixed sequences of multiplies: the case pool and the walks of tests/test_gpu_engine_sequences.py, and what
tests/test_engine_sequences_cpu.py asserts about them without a GPU.

The pool holds 36 distinct multiplies with fixed seeds, taken from the generators of tests/test_gpu_random_sweep.py (make_case, make_big_case with
its two sets of block-size mixes) and four complex128 cases built as tests/test_gpu_complex_multiply.py builds its own.  Host operands and oracle
results are computed once per case (functools.lru_cache).  A walk is an ordered list of pool indices; what makes each walk worth running is
asserted by the CPU file.

FAMILY names, per pool entry, the kernel family the automatic choice takes for it: predicted on the host from mm_choose.h (tests/test_numeric_choice.py)
where that can answer -- a product matrix without symmetry --, and asserted on the device from last_kernel() for every entry.  `generic`
(mm_numeric_f64 / mm_numeric_f32) is not in the list: the generators make no block above 80 and no fp32 block above 32, so the automatic choice
never reaches it at these sizes; neither do they reach the fp32 exact-size kernels within the first 20000 seeds (fp32 AND one dominant cube)."""
import functools

import numpy as np

from oracle import oracle as O
from tests import test_gpu_complex_multiply as CM
from tests import test_gpu_filter_in_place as FIP
from tests import test_gpu_random_sweep as SW

S, B, M, Z = "sweep", "big", "mid", "z64"

# (generator, seed): make_case(seed), make_big_case(seed), make_big_case(seed, MID_MIXES, BIG_MIXES + MID_MIXES); Z: an entry of COMPLEX
POOL = (
    (S, 1071), (S, 1016), (S, 1019), (S, 1123), (S, 1117), (S, 1070), (S, 1068), (S, 1035), (S, 1020), (S, 1085),     # 0 ... 9
    (M, 12004), (M, 12029), (M, 12019), (M, 12035), (B, 9044), (S, 1131), (S, 1002), (S, 1010), (S, 1052), (S, 1023),  # 10 ... 19
    (S, 4852), (S, 12305), (S, 9790), (S, 1044), (S, 1015), (S, 1120), (S, 1011), (M, 12023), (B, 9029), (S, 1093),    # 20 ... 29
    (S, 1042), (S, 1099), (Z, 0), (Z, 1), (Z, 2), (Z, 3),                                                               # 30 ... 35
)

# the complex cases: arguments of test_gpu_complex_multiply.complex_case, then alpha, beta, retain_sparsity
COMPLEX = (
    dict(dims=(230, 260, 200), sp=(0.5, 0.6, 0.7), mixes=([1, 13, 1, 5], [1, 23, 1, 4], [1, 7, 1, 32]), ta="C", tb="N", seed=1, alpha=-0.5 + 2j, beta=2 - 1j,
         retain=False),
    dict(dims=(6 * 23 + 12, 5 * 23, 7 * 23 + 11), sp=(0.3, 0.3, 0.5), mixes=([1, 23], [1, 23], [1, 23]), ta="N", tb="N", seed=239, alpha=0.75 - 0.5j,
         beta=1.5 + 0.25j, retain=False),
    dict(dims=(5 * 45 + 15, 4 * 67 + 33, 4 * 78 + 3), sp=(0.3, 0.3, 0.5), mixes=([1, 45], [1, 67], [1, 78]), ta="N", tb="T", seed=190, alpha=-1.25 + 0.5j,
         beta=0.5 - 2j, retain=False),
    dict(dims=(270, 250, 290), sp=(0.4, 0.4, 0.6), mixes=([1, 13, 1, 23, 1, 32, 1, 40],) * 3, ta="T", tb="C", seed=77, alpha=2j, beta=0, retain=True),
)

# the family of every pool entry (see the module text); "pipe/lds" and "f32" are one family each for the pool's counts
FAMILY = (
    "pipe/lds", "pipe/lds", "pipe/lds", "pipe/lds", "f32", "pipe/lds", "pipe/lds", "pipe/lds", "pipe/lds", "pipe/lds",   # 0 ... 9
    "big", "mid", "mid", "mid", "big", "tiny", "tiny", "tiny", "small8", "small8",                                        # 10 ... 19
    "hot", "hot", "hot", "pipe/lds", "pipe/lds", "pipe/lds", "pipe/lds", "mid", "big", "f32",                            # 20 ... 29
    "f32", "f32", "z64", "z64", "z64", "z64",                                                                             # 30 ... 35
)
FAMILIES = ("tiny", "small8", "hot", "pipe/lds", "mid", "big", "f32", "z64")


def family_of(kernel):
    """the family a last_kernel() / mm_choose.h name belongs to"""
    for prefix, fam in (("mm_numeric_z64", "z64"), ("mm_numeric_f32", "f32"), ("mm_numeric_f64_tiny", "tiny"), ("mm_numeric_f64_small", "small8"),
                        ("mm_numeric_f64_hot", "hot"), ("mm_numeric_f64_pipe", "pipe/lds"), ("mm_numeric_f64_lds", "pipe/lds"), ("mm_numeric_f64_mid", "mid"),
                        ("mm_numeric_f64_big", "big"), ("mm_numeric_f64_class", "classes")):
        if kernel.startswith(prefix):
            return fam
    return "generic" if kernel in ("mm_numeric_f64", "mm_numeric_f32") else kernel


WALKS = {
    # by C block count, largest first: every later case runs in work areas left larger and dirtier than it needs
    "descending": [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15],
    # every case reallocates
    "ascending": [26, 15, 14, 13, 23, 24, 27, 20, 21, 22, 28, 30, 17, 31, 19, 29, 4, 25, 16, 18],
    # np.random.default_rng(71) / (72).permutation(36)[:18], written out
    "shuffled_a": [25, 2, 5, 10, 12, 1, 4, 9, 3, 15, 14, 24, 26, 32, 27, 7, 19, 17],
    "shuffled_b": [14, 7, 6, 31, 33, 5, 1, 17, 12, 3, 9, 26, 18, 34, 4, 2, 35, 30],
    # fp64, fp32 and complex128 cycling: the work areas are reread under another element size
    "types": [0, 4, 32, 16, 29, 33, 11, 30, 34, 28, 31, 35, 20, 29, 32, 18, 4, 33],
    # filtered and unfiltered cases alternating, each kind from large to small
    "filters": [3, 16, 5, 1, 30, 29, 9, 19, 10, 8, 23, 11, 14, 21, 24, 27, 15, 12],
}
# the walks that run again under a switch.  DBCSR_AMD_MM_CLASSES=2 compiles a kernel per (m, n) class of every mixed-size fp64 case the first time the process
# meets it (about half a second per case on MI355X): its three walks are those that share the fewest such cases, so that no test pays for more than eight
SWITCH_WALKS = {"DBCSR_AMD_MM_CLASSES=2": ("types", "ascending", "shuffled_a"), "DBCSR_AMD_MM_SYMBOLIC=rows": ("descending", "shuffled_b", "filters")}


class Host:
    """a pool entry on the host: operands, the oracle's result, and the numbers the walks are built from"""

    def __init__(self, index):
        self.index = index
        self.kind, seed = POOL[index]
        self.complex = self.kind == Z
        if self.complex:
            z = COMPLEX[seed]
            self.par = dict(ta=z["ta"], tb=z["tb"], alpha=z["alpha"], beta=z["beta"], retain=z["retain"], eps=0.0, symm_c="N", dtype=np.complex128,
                            M=z["dims"][0], N=z["dims"][1], K=z["dims"][2], mix_m=z["mixes"][0], mix_n=z["mixes"][1], mix_k=z["mixes"][2])
            self.A, self.B, self.C = CM.complex_case(*z["dims"], z["sp"], *z["mixes"], z["ta"], z["tb"], seed=z["seed"])
            self.ref, self.info = CM.index_reference(z["ta"], z["tb"], self.A, self.B, self.C, z["beta"], z["retain"])
            self.R, self.bound = CM.reference(z["ta"], z["tb"], z["alpha"], self.A, self.B, z["beta"], self.C)
            self.unfiltered_blocks = self.ref.nblks
        else:
            self.par = SW.make_case(seed) if self.kind == S else (SW.make_big_case(seed) if self.kind == B
                                                                   else SW.make_big_case(seed, SW.MID_MIXES, SW.BIG_MIXES + SW.MID_MIXES))
            self.A, self.B, self.C, self.ref, self.info = SW.build_case(self.par)
            self.unfiltered_blocks = self.ref.nblks
            if self.par["eps"] > 0:
                c = dict(self.par, eps=0.0)
                self.unfiltered_blocks = SW.build_case(c)[3].nblks
        self.dtype = np.dtype(self.par["dtype"]).name
        self.c_blocks = int(self.ref.nblks)
        self.products = int(self.info["nproducts"])
        self.filtered = self.par["eps"] > 0
        self.dropped = (self.unfiltered_blocks - self.c_blocks) / max(self.unfiltered_blocks, 1)

    def __repr__(self):
        p = self.par
        return "pool[%d] %s %s %s%s alpha %s beta %s%s%s symm %s: %d C blocks, %d products" % (
            self.index, POOL[self.index], self.dtype, p["ta"], p["tb"], p["alpha"], p["beta"], " retain" if p["retain"] else "",
            " eps %g" % p["eps"] if self.filtered else "", p["symm_c"], self.c_blocks, self.products)


@functools.lru_cache(maxsize=None)
def host(index):
    return Host(index)


def pool_counts():
    """what the issue asks the pool to hold, counted"""
    hs = [host(i) for i in range(len(POOL))]
    return {
        "cases": len(hs),
        "families": {f: FAMILY.count(f) for f in FAMILIES},
        "eps > 0": sum(h.filtered for h in hs),
        "retain": sum(bool(h.par["retain"]) for h in hs),
        "symmetric C": sum(h.par["symm_c"] != "N" for h in hs),
        "transposes": sorted({h.par["ta"] + h.par["tb"] for h in hs}),
        "alpha == 0": sum(h.par["alpha"] == 0 for h in hs),
        "beta == 0": sum(h.par["beta"] == 0 for h in hs),
        "C_in without a block": sum(h.C.nblks == 0 for h in hs),
        "result without a block": sum(h.c_blocks == 0 for h in hs),
        "A without a block": sum(h.A.nblks == 0 for h in hs),
    }


def choice_case(h):
    """the (M, N, K, ..., mixes) tuple and keyword facts tests/test_numeric_choice.py's `choose` takes, or None where the host build of mm_choose.h cannot
    answer: a product matrix with symmetry (its index goes into canonical form first), a product without a block (no numeric phase), complex data (one
    family, nothing to choose)"""
    p = h.par
    if h.complex or p["symm_c"] != "N" or h.unfiltered_blocks == 0:
        return None
    case = (p["M"], p["N"], p["K"], 0, 0, 0, p["mix_m"], p["mix_n"], p["mix_k"])
    nprod = SW.build_case(dict(p, eps=0.0))[4]["nproducts"] if h.filtered else h.products
    return case, dict(c_nblks=h.unfiltered_blocks, products_per_block=nprod / h.unfiltered_blocks, fp64=p["dtype"] == np.float64, retain=bool(p["retain"]),
                      filter_active=h.filtered)


# ---- part 4: block norms left by a numeric kernel, then C changed in place -------------------------------------------------------------------------------
# The filtered two-phase multiply runs on "23_with_tails" of tests/test_gpu_filter_in_place.py (mm_numeric_f64_hot<23,23,23>, which leaves norms); set_diag
# needs a square matrix, so its case is the square one below.  ON_THE_FLY is the eps of the symbolic phase: positive, so that the numeric kernel leaves its
# norms, and far below every product of block norms, so that the product is the oracle's unfiltered one.
STALE_CASE = "23_with_tails"
ON_THE_FLY = 1e-12
STALE_OPS = ("scale", "add", "set_diag", "scale_by_vector", "rank_update")
SQUARE = (23 * 5, 23 * 5, 23 * 5, 0.0, 0.0, 0.0, [1, 23], [1, 23], [1, 23])


@functools.lru_cache(maxsize=None)
def square_inputs():
    """five block rows and columns of 23, every block stored.  A and B are tiny against C_in, whose diagonal blocks are the smallest of all and whose other
    blocks are spread over two and a half decades: at the median eps every diagonal block of the product is dropped, and set_diag with elements of 10
    brings all five back -- 20 % of the blocks change sides"""
    A, B_, C = O.perf_case(*SQUARE)
    FIP.spread([C], seed=9)
    A.data *= 1e-4
    B_.data *= 1e-4
    rows = C.rows()
    for b in range(C.nblks):
        if rows[b] == C.col_i[b]:
            C.data[C.blk_p[b]:C.blk_p[b] + 23 * 23] *= 1e-4
    return A, B_, C


@functools.lru_cache(maxsize=None)
def stale_product(op):
    """(A, B, C_in, the oracle's unfiltered product P, eps of the final filter) for one in-place change"""
    if op == "set_diag":
        A, B_, C = square_inputs()
        P = O.multiply("N", "N", 1.0, A, B_, 1.0, C)[0]
        s = np.sort(np.sqrt(FIP.block_sq_norms(P)))
        i = int(round(0.5 * len(s)))
        return A, B_, C, P, float(0.5 * (s[i - 1] + s[i]))
    A, B_, C = FIP.inputs(STALE_CASE)
    return A, B_, C, FIP.oracle_product(STALE_CASE), FIP.quantile_eps(STALE_CASE, 0.5)


def stale_vectors(P, op):
    """the vectors the change takes, float64"""
    rng = np.random.default_rng(4)
    nr, nc = int(P.row_sizes.sum()), int(P.col_sizes.sum())
    if op == "set_diag":
        return (np.full(nr, 10.0),)
    if op == "scale_by_vector":    # (columns: decades apart, so that whole block columns change sides)
        return (np.repeat(10.0 ** rng.uniform(-1.5, 1.5, len(P.col_sizes)), P.col_sizes),)
    if op == "rank_update":   # (X is zero in every other block row: those blocks are only scaled down, the others grow past eps)
        x = rng.uniform(-1, 1, (nr, 3)) * np.repeat(np.arange(len(P.row_sizes)) % 2, P.row_sizes)[:, None]
        return x, rng.uniform(-1, 1, (nc, 3))
    return ()


def changed_host(P, op):
    """the oracle's side of the in-place change: P's data after it, in float64 on the dense scatter or the data area"""
    data = P.data.copy()
    rows = P.rows()
    ro, co = np.concatenate([[0], np.cumsum(P.row_sizes)]), np.concatenate([[0], np.cumsum(P.col_sizes)])
    v = stale_vectors(P, op)
    if op == "scale":
        return 4.0 * data
    if op == "add":           # C <- 1 C + 3 D, D a copy of C: the flat (same pattern) add
        return data + 3.0 * data
    for b in range(P.nblks):
        r, c = int(rows[b]), int(P.col_i[b])
        m, n = int(P.row_sizes[r]), int(P.col_sizes[c])
        blk = data[P.blk_p[b]:P.blk_p[b] + m * n].reshape(n, m).T    # (blocks are stored column by column)
        if op == "set_diag" and r == c:
            blk[np.arange(m), np.arange(m)] = v[0][ro[r]:ro[r + 1]]
        elif op == "scale_by_vector":
            blk *= v[0][co[c]:co[c + 1]][None, :]
        elif op == "rank_update":   # C <- 0.25 C + 40 X Y^T
            blk[:] = 0.25 * blk + 40.0 * (v[0][ro[r]:ro[r + 1]] @ v[1][co[c]:co[c + 1]].T)
    return data


def kept_sets(op):
    """(kept before the change, kept after it) at the final filter's eps: boolean per block of P, from the oracle's product"""
    _, _, _, P, eps = stale_product(op)
    before = ~(FIP.block_sq_norms(P) < eps * eps)
    Q = O.Bcsr(P.row_sizes, P.col_sizes, P.row_p, P.col_i, P.blk_p, changed_host(P, op))
    after = ~(FIP.block_sq_norms(Q) < eps * eps)
    return before, after, Q
