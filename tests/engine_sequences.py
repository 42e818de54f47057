"""One long-lived engine through mixed sequences of multiplies: the case pool and the walks of tests/test_gpu_engine_sequences.py, and what
tests/test_engine_sequences_cpu.py asserts about them without a GPU.  (Further down: the stale-norms scenario, and the pool and walks of the algebra.)

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


def subset(M, keep):
    """the blocks of M that the boolean `keep` names, as a packed matrix"""
    rows = M.rows()
    n = FIP.block_sizes(M)[keep]
    row_p = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=M.nbr))]).astype(np.int32)
    data = np.concatenate([M.data[p:p + k] for p, k in zip(M.blk_p[keep], n)]) if n.size else M.data[:0]
    return O.Bcsr(M.row_sizes, M.col_sizes, row_p, M.col_i[keep], np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int64), data)


def triangle(M):
    """the stored triangle (block row <= block column) of a square matrix, packed: what dbcsr_amd_bcsr_twin_count / _desymmetrize_count take"""
    return subset(M, M.rows() <= M.col_i)


# ---- part 4: block norms left by a numeric kernel, then C changed in place -------------------------------------------------------------------------------
# The filtered two-phase multiply runs on "23_with_tails" of tests/test_gpu_filter_in_place.py (mm_numeric_f64_hot<23,23,23>, which leaves norms); set_diag
# needs a square matrix, so its case is the square one below.  ON_THE_FLY is the eps of the symbolic phase: positive, so that the numeric kernel leaves its
# norms, and far below every product of block norms, so that the product is the oracle's unfiltered one.
STALE_CASE = "23_with_tails"
ON_THE_FLY = 1e-12
# the in-place writers the suite began with, then those of the block diagonals, the element-wise operations, the dense conversion and the submatrix method
STALE_OPS_FIRST = ("scale", "add", "set_diag", "scale_by_vector", "rank_update")
STALE_OPS = STALE_OPS_FIRST + ("add_on_diag", "invert_block_diag", "scale_by_block_diag", "function_of_elements", "hadamard_in_place", "copy_keep_sparsity",
                               "from_dense", "submatrix_scatter")
# ... on the square case: the diagonal operations, and the submatrix method (a square block structure; with every block stored each of its five submatrices is
# the whole matrix).  Which case an operation can tell stale norms from fresh ones on was tried with the oracle alone: 1/x keeps every block of the square case,
# tanh keeps none of "23_with_tails" (tests/test_engine_sequences_cpu.py asserts what the chosen ones give)
SQUARE_OPS = ("set_diag", "add_on_diag", "invert_block_diag", "submatrix_scatter")
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
    if op in SQUARE_OPS:
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
    if op == "from_dense":    # the window: P with block magnitudes three decades apart, and values outside P's pattern that nobody may read
        W = O.Bcsr(P.row_sizes, P.col_sizes, P.row_p, P.col_i, P.blk_p, P.data * per_block(P, 10.0 ** rng.uniform(-1.5, 1.5, P.nblks))).to_dense()
        W[W == 0] = 1e6
        return (W,)
    if op == "submatrix_scatter":   # one window per block column, each the whole matrix (every block is stored) at a magnitude of its own
        assert P.nblks == len(P.row_sizes) * len(P.col_sizes) and nr == nc
        return (10.0 ** rng.uniform(-1.5, 1.5, len(P.col_sizes))[:, None, None] * P.to_dense()[None, :, :],)
    return ()


def per_block(P, values):
    """one value per block, spread over the block's elements of P's data area"""
    out = np.zeros(P.data.size)
    for b, (p, n) in enumerate(zip(P.blk_p, FIP.block_sizes(P))):
        out[p:p + n] = values[b]
    return out


@functools.lru_cache(maxsize=None)
def stale_operand(op):
    """the second matrix of the changes that replace values from one, with block magnitudes three decades apart (as scale_by_vector's columns are)"""
    P = stale_product(op)[3]
    rng = np.random.default_rng(6)
    decades = per_block(P, 10.0 ** rng.uniform(-1.5, 1.5, P.nblks))
    if op == "hadamard_in_place":     # P's index
        return O.Bcsr(P.row_sizes, P.col_sizes, P.row_p, P.col_i, P.blk_p, decades * rng.uniform(0.5, 1.5, P.data.size))
    if op == "copy_keep_sparsity":    # two of three blocks of P: the others become +0.0
        return subset(O.Bcsr(P.row_sizes, P.col_sizes, P.row_p, P.col_i, P.blk_p, decades * P.data[::-1]), np.arange(P.nblks) % 3 != 2)
    if op == "scale_by_block_diag":   # one well-conditioned block per block row
        m = P.row_sizes.astype(np.int64)
        blocks = [10.0 ** rng.uniform(-1.5, 1.5) * (np.eye(k) + 0.1 * rng.uniform(-1, 1, (k, k))) for k in m]
        return O.Bcsr(P.row_sizes, P.row_sizes, np.arange(len(m) + 1), np.arange(len(m)), np.concatenate([[0], np.cumsum(m * m)[:-1]]),
                      np.concatenate([blk.T.reshape(-1) for blk in blocks]))
    raise AssertionError(op)


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
    if op == "hadamard_in_place":
        return data * stale_operand(op).data
    S = stale_operand(op) if op in ("copy_keep_sparsity", "scale_by_block_diag") else None
    if op == "copy_keep_sparsity":
        source = {(int(r), int(c)): S.data[p:p + n] for r, c, p, n in zip(S.rows(), S.col_i, S.blk_p, FIP.block_sizes(S))}
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
        elif op == "add_on_diag" and r == c:
            blk[np.arange(m), np.arange(m)] += 10.0
        elif op == "invert_block_diag" and r == c:
            blk[:] = np.linalg.inv(blk)
        elif op == "scale_by_block_diag":   # side = "left": D_r times the block
            blk[:] = S.data[S.blk_p[r]:S.blk_p[r] + m * m].reshape(m, m).T @ blk
        elif op == "function_of_elements":  # dbcsr_func_inverse
            blk[:] = 1.0 / blk
        elif op == "copy_keep_sparsity":
            blk[:] = source[r, c].reshape(n, m).T if (r, c) in source else 0.0
        elif op == "from_dense":
            blk[:] = v[0][ro[r]:ro[r + 1], co[c]:co[c + 1]]
        elif op == "submatrix_scatter":     # block column c out of the window of its own submatrix
            blk[:] = v[0][c][ro[r]:ro[r + 1], co[c]:co[c + 1]]
    return data


def kept_sets(op):
    """(kept before the change, kept after it) at the final filter's eps: boolean per block of P, from the oracle's product"""
    _, _, _, P, eps = stale_product(op)
    before = ~(FIP.block_sq_norms(P) < eps * eps)
    Q = O.Bcsr(P.row_sizes, P.col_sizes, P.row_p, P.col_i, P.blk_p, changed_host(P, op))
    after = ~(FIP.block_sq_norms(Q) < eps * eps)
    return before, after, Q


# ---- part E: an algebra walk ------------------------------------------------------------------------------------------------------------------------------
# About 25 entries of the algebra share the engine's alg_* buffers and the scan's partial sums, each with a layout of its own, and each clears only the words
# it knows about.  The walks below run every public operation of dbcsr_amd/operations.py and dbcsr_amd/submatrix.py, and the engine's filter, crop,
# transpose and desymmetrize, against each other on ONE engine, over ten square matrices of three element types and ten sets of block sizes (the ring of
# eight size sets the engine remembers, alg_len, wraps).  A step is (operation, matrix index).
#
# The pool: (full size, block-size mix, occupancy, element type, seed).  The mixes are those of the other test files; no block is above 80 (the block
# inverse and the block scale take up to 96).  Two matrices share every full size, with different element types and mixes: a walk ordered by full size can
# still change the element type at every step.  Every diagonal block is stored, and made diagonally dominant (so that its inverse is well defined).
ALG_POOL = (
    (600, [1, 16, 1, 32, 1, 33, 1, 80], 0.4, "float64", 201),
    (600, [1, 13, 1, 5], 0.3, "complex128", 202),
    (420, [1, 13, 1, 23, 1, 32, 1, 7], 0.4, "float64", 203),
    (420, [1, 5, 1, 7, 1, 3], 0.3, "float32", 204),
    (300, [1, 13, 1, 5, 1, 7], 0.5, "float64", 205),
    (300, [1, 23, 1, 4], 0.5, "complex128", 206),
    (160, [1, 23], 0.5, "float64", 207),
    (160, [1, 1, 1, 3], 0.5, "float32", 208),
    (60, [1, 5, 1, 8], 0.5, "float64", 209),
    (60, [1, 7, 1, 32], 0.4, "float32", 210),
)
# every public operation (dbcsr_add and dbcsr_hadamard_product once per path, dbcsr_norm for the one kind that has no entry of its own) and the engine's four
ALG_OPS = ("add_flat", "add_union", "scale", "add_on_diag", "trace", "dot", "frobenius_norm", "maxabs_norm", "gershgorin_norm", "norm_column", "get_diag",
           "set_diag", "scale_by_vector", "matvec", "multivec", "rank_update", "get_block_diag", "invert_block_diag", "scale_by_block_diag", "to_dense",
           "from_dense", "create_from_dense", "hadamard_flat", "hadamard_two_patterns", "copy_keep_sparsity", "function_of_elements", "submatrix_gather",
           "submatrix_scatter", "submatrix_apply", "filtered", "cropped", "transposed", "desymmetrized")
ALG_REAL_ONLY = ("dot", "function_of_elements")     # (NotImplementedError for complex data)
ALG_FUNCTION = ("tanh", 0.25, -0.5)                 # dbcsr_function_of_elements: the function, a0, a1


def with_diagonal(M, seed):
    """M with every diagonal block stored: the missing ones drawn from [0, 1) as the generator's values are"""
    from tests import test_gpu_matrix_norms as MN
    rng = np.random.default_rng(seed)
    blocks = dict(MN.blocks_of(M))
    for r, m in enumerate(M.row_sizes):
        if (r, r) not in blocks:
            blocks[(r, r)] = rng.uniform(0.0, 1.0, int(m) ** 2)
    return MN.from_blocks(M.row_sizes, M.col_sizes, blocks, np.float64)


def dominant(M):
    """2 m added to the diagonal elements of every diagonal block of m x m: diagonally dominant by rows, whatever the element type"""
    data = M.data.copy()
    for b, r in enumerate(M.rows()):
        if int(M.col_i[b]) == int(r):
            m = int(M.row_sizes[r])
            data[M.blk_p[b] + np.arange(m) * (m + 1)] += 2 * m
    return O.Bcsr(M.row_sizes, M.col_sizes, M.row_p, M.col_i, M.blk_p, data)


def block_sq_moduli(M):
    """sum of |x|^2 per block, float64 (complex data too)"""
    sq = np.abs(M.data).astype(np.float64) ** 2
    return np.array([sq[p:p + n].sum() for p, n in zip(M.blk_p, FIP.block_sizes(M))])


class AlgHost:
    """an entry of ALG_POOL on the host: the matrix M, a twin T on M's pattern with other values, a matrix Q of the same sizes on another pattern, the stored
    triangle of M, the input of the function of elements (real types), the eps that drops half of M's blocks, and the index sets of the submatrix method"""

    def __init__(self, k):
        from tests import elementwise_ref as R
        from tests import submatrix_ref as SR
        from tests import test_gpu_matrix_norms as MN
        full, mix, occupancy, dtype, seed = ALG_POOL[k]
        self.index, self.dtype = k, np.dtype(dtype)
        self.sizes = O.make_block_sizes(full, mix)
        self.n, self.nb = int(self.sizes.sum()), len(self.sizes)
        self.raw = with_diagonal(O.make_random_matrix(self.sizes, self.sizes, 1.0 - occupancy, O.RANDMAT_SEED_INIT + seed), seed)
        other = with_diagonal(O.make_random_matrix(self.sizes, self.sizes, 1.0 - occupancy, O.RANDMAT_SEED_INIT + seed + 50), seed + 50)
        self.M = dominant(MN.typed(self.raw, self.dtype, 1))
        self.T = O.Bcsr(self.sizes, self.sizes, self.M.row_p, self.M.col_i, self.M.blk_p, MN.typed(self.raw, self.dtype, 2).data[::-1].copy())
        self.Q = dominant(MN.typed(other, self.dtype, 3))
        self.tri = triangle(self.M)
        self.symmetry = "H" if self.dtype.kind == "c" else "S"
        self.F = None if self.dtype.kind == "c" else R.function_input(self.raw, *ALG_FUNCTION, self.dtype)
        s = np.sort(np.sqrt(block_sq_moduli(self.M)))
        self.eps = float(0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2]))
        assert s[len(s) // 2] - s[len(s) // 2 - 1] > 1e-6 * self.eps, "two block norms sit on the filter's threshold"
        # one submatrix per block column; the walks gather and scatter three of them, at the side of the largest of all (the plan's max_dim)
        self.sets, self.owner = SR.brute_sets(self.M)
        self.sub_n = int(SR.plan_arrays(self.sets, self.sizes)[3].max())
        self.subs = [0, self.nb // 2, self.nb - 1]
        # dbcsr_submatrix_apply: the first three block columns own a submatrix each, the others none
        self.groups = [0, 1, 2] + [-1] * (self.nb - 3)
        self.group_sets, self.group_owner = SR.brute_sets(self.M, self.groups)
        self.crop = ((self.n // 6, 3 * self.n // 4), (self.n // 5, 2 * self.n // 3))

    def admits(self, op):
        return not (self.dtype.kind == "c" and op in ALG_REAL_ONLY)

    def __repr__(self):
        return "alg[%d] %d rows in %d blocks %s, %d blocks stored" % (self.index, self.n, self.nb, self.dtype.name, self.M.nblks)


@functools.lru_cache(maxsize=None)
def alg(k):
    return AlgHost(k)


# 66 steps each: every operation twice (np.random.default_rng(81) / (82) / (83): two permutations of ALG_OPS one after the other, written out).  Where the
# drawn matrix does not admit the operation (ALG_REAL_ONLY on complex data) the real one of the same full size stands in.
ALG_WALKS = {
    # by full size, largest first, the two matrices of a size in turn: later steps run in areas left larger and dirtier than they need
    # ("ascending": the same the other way round, every growth reallocates; "shuffled": the matrix drawn too, rng.integers(0, 10))
    "descending": [
        ("desymmetrized", 0), ("dot", 0), ("norm_column", 0), ("maxabs_norm", 1), ("filtered", 0), ("set_diag", 1), ("invert_block_diag", 0),
        ("rank_update", 1), ("cropped", 0), ("submatrix_apply", 1), ("transposed", 0), ("frobenius_norm", 1), ("get_diag", 0), ("get_block_diag", 1),
        ("to_dense", 2), ("add_union", 3), ("matvec", 2), ("copy_keep_sparsity", 3), ("trace", 2), ("create_from_dense", 3),
        ("function_of_elements", 2), ("submatrix_scatter", 3), ("hadamard_two_patterns", 2), ("gershgorin_norm", 3), ("scale_by_block_diag", 2),
        ("add_flat", 3), ("scale_by_vector", 2), ("submatrix_gather", 3), ("scale", 4), ("hadamard_flat", 5), ("add_on_diag", 4), ("from_dense", 5),
        ("multivec", 4), ("multivec", 5), ("scale", 4), ("to_dense", 5), ("hadamard_flat", 4), ("function_of_elements", 4), ("add_flat", 4),
        ("frobenius_norm", 5), ("rank_update", 4), ("submatrix_scatter", 5), ("invert_block_diag", 6), ("gershgorin_norm", 7),
        ("scale_by_vector", 6), ("copy_keep_sparsity", 7), ("cropped", 6), ("create_from_dense", 7), ("norm_column", 6), ("add_on_diag", 7),
        ("submatrix_gather", 6), ("from_dense", 7), ("filtered", 6), ("submatrix_apply", 7), ("dot", 6), ("matvec", 7), ("add_union", 8),
        ("set_diag", 9), ("desymmetrized", 8), ("transposed", 9), ("maxabs_norm", 8), ("hadamard_two_patterns", 9), ("get_block_diag", 8),
        ("trace", 9), ("scale_by_block_diag", 8), ("get_diag", 9),
    ],
    "ascending": [
        ("cropped", 8), ("multivec", 9), ("norm_column", 8), ("maxabs_norm", 9), ("hadamard_two_patterns", 8), ("submatrix_scatter", 9),
        ("get_diag", 8), ("trace", 9), ("frobenius_norm", 8), ("to_dense", 9), ("get_block_diag", 8), ("set_diag", 9), ("dot", 8),
        ("invert_block_diag", 9), ("copy_keep_sparsity", 6), ("add_union", 7), ("scale", 6), ("add_on_diag", 7), ("add_flat", 6), ("transposed", 7),
        ("function_of_elements", 6), ("scale_by_vector", 7), ("rank_update", 6), ("submatrix_apply", 7), ("from_dense", 6), ("create_from_dense", 7),
        ("filtered", 6), ("gershgorin_norm", 7), ("submatrix_gather", 4), ("matvec", 5), ("scale_by_block_diag", 4), ("hadamard_flat", 5),
        ("desymmetrized", 4), ("set_diag", 5), ("get_diag", 4), ("filtered", 5), ("rank_update", 4), ("copy_keep_sparsity", 5), ("matvec", 4),
        ("get_block_diag", 5), ("norm_column", 4), ("scale_by_block_diag", 5), ("submatrix_scatter", 2), ("add_on_diag", 3), ("desymmetrized", 2),
        ("add_union", 3), ("submatrix_gather", 2), ("multivec", 3), ("to_dense", 2), ("hadamard_two_patterns", 3), ("hadamard_flat", 2),
        ("add_flat", 3), ("create_from_dense", 2), ("dot", 3), ("submatrix_apply", 2), ("function_of_elements", 3), ("gershgorin_norm", 0),
        ("scale_by_vector", 1), ("invert_block_diag", 0), ("cropped", 1), ("transposed", 0), ("scale", 1), ("trace", 0), ("maxabs_norm", 1),
        ("from_dense", 0), ("frobenius_norm", 1),
    ],
    "shuffled": [
        ("trace", 0), ("scale_by_block_diag", 6), ("norm_column", 8), ("transposed", 5), ("matvec", 4), ("scale", 2), ("hadamard_flat", 5),
        ("add_union", 2), ("get_diag", 4), ("invert_block_diag", 2), ("rank_update", 8), ("cropped", 8), ("copy_keep_sparsity", 6), ("multivec", 1),
        ("submatrix_scatter", 0), ("gershgorin_norm", 3), ("submatrix_gather", 4), ("function_of_elements", 4), ("hadamard_two_patterns", 8),
        ("dot", 4), ("frobenius_norm", 9), ("to_dense", 7), ("maxabs_norm", 2), ("create_from_dense", 4), ("get_block_diag", 6),
        ("submatrix_apply", 5), ("desymmetrized", 8), ("scale_by_vector", 8), ("add_on_diag", 3), ("add_flat", 3), ("from_dense", 0),
        ("filtered", 9), ("set_diag", 7), ("add_on_diag", 7), ("dot", 3), ("filtered", 1), ("scale_by_block_diag", 4), ("trace", 6),
        ("maxabs_norm", 0), ("submatrix_apply", 2), ("set_diag", 9), ("create_from_dense", 5), ("copy_keep_sparsity", 6), ("hadamard_flat", 0),
        ("add_flat", 8), ("submatrix_scatter", 3), ("norm_column", 2), ("hadamard_two_patterns", 9), ("get_block_diag", 4), ("transposed", 9),
        ("function_of_elements", 2), ("multivec", 1), ("to_dense", 5), ("scale", 7), ("add_union", 8), ("from_dense", 3), ("gershgorin_norm", 0),
        ("invert_block_diag", 1), ("rank_update", 4), ("matvec", 2), ("frobenius_norm", 4), ("cropped", 6), ("scale_by_vector", 3), ("get_diag", 2),
        ("desymmetrized", 4), ("submatrix_gather", 2),
    ],
}
