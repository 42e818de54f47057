"""The option sweep: seeded multiplies over the axes tests/test_gpu_random_sweep.py leaves out -- complex128 data, 'C' transposes, limits, operands and
products with symmetry ('S' / 'A' real, 'H' / 'K' complex), fp32 blocks above 32, blocks above 80 -- with the generators, the dense long-double reference
and the conditions on the inputs.  tests/test_option_sweep_cpu.py checks all of it without a GPU; tests/test_gpu_option_sweep.py runs every case through
the dbcsr_multiply mirror and through the C entry (dbcsr_amd_multiply and its siblings).  Nothing here touches a GPU.

THE REFERENCE.  A, B and C_in are scattered to dense np.longdouble / np.clongdouble (63-bit mantissa; fp32 inputs are the float32 values, converted
exactly), stored triangles are expanded as the multiply expands its operands (O.desymmetrize; 'H' / 'K': expected_full of tests/test_gpu_hermitian.py),
and R = beta C_in + alpha op(A)[rows, k] op(B)[k, cols] is formed inside the window only, following dbcsr_multiply: the default limits are "optimised
away", C_in counts as empty when product data is not kept, and outside the window a kept C keeps its bits.  `restate` does this at block level, as
oracle/dbcsr_oracle.c does (:539-565 the fp32 block norms and the row eps, :633 the on-the-fly rule, :635 the canonical form of a product with
symmetry, :669-679 the final filter): R is the sum of the KEPT block products.  It gives the block index and the flop count as well; the CPU file
shows that it reproduces the oracle's index, flop and values on every real case, which is what lets it stand for complex data with filter_eps.

THE BAR, element-wise: |got - R| <= gamma (|alpha| (|op A| |op B|) + |beta| |C_in|), the absolute-value product formed the same dense way.  With n the
number of inner-dimension elements inside the k window:
    real data     gamma = (n + 8) u / (1 - (n + 8) u), u = 2^-53 (fp64) / 2^-24 (fp32): the standard bound for a sum of n products in any order
                  (Higham, Accuracy and Stability, section 3.1: gamma_n), the 8 for alpha, beta, the final add and up to four roundings of C between k passes
    complex128    gamma = sqrt(2) (2 n + 10) 2^-53: the derivation in the header of tests/test_gpu_complex_multiply.py
The reference's own error is n 2^-64 of the same bound, 2^-11 of the fp64 bar.  Derived, not measured: a case above its bar is a finding.

SEEDS.  Each stratum has a seed range of its own; DBCSR_AMD_OPTSWEEP_<NAME> lengthens it and DBCSR_AMD_SWEEP_OFFSET shifts the seeds, as for the sweep of
tests/test_gpu_random_sweep.py.  A case that fails a condition on the inputs (`conditions`) is not skipped: its seed is replaced in RESEED."""
import functools
import os

import numpy as np

from oracle import oracle as O
from tests.test_gpu_complex_multiply import part, with_imag
from tests.test_gpu_hermitian import expected_full
from tests.test_gpu_random_sweep import BIG_MIXES, MID_MIXES, MIXES, SWEEP_OFFSET

LD, CLD = np.longdouble, np.clongdouble
LONG_DOUBLE_OK = bool(np.finfo(np.longdouble).eps < 2e-19)
FILLS = [0.0, 0.3, 0.6, 0.8, 0.95, 0.999]
F64, F32, Z64 = "float64", "float32", "complex128"
U = {F64: 2.0 ** -53, F32: 2.0 ** -24}

STRATA = ("complex", "limits", "symmetry", "sizes")
DEFAULT_COUNT = {"complex": 40, "limits": 48, "symmetry": 40, "sizes": 24}
BASE_SEED = {"complex": 20000, "limits": 30000, "symmetry": 40000, "sizes": 50000}
# (stratum, case number) -> the seed that replaces BASE_SEED + number: the case failed the named condition on its inputs (conditions(), asserted for
# every default case by tests/test_option_sweep_cpu.py)
RESEED = {
    ("complex", 8): 21008,    # 'C' does not differ from 'T'
    ("limits", 0): 33000,     # no stored element outside the window
    ("limits", 3): 31003,     # no stored element outside the window
    ("limits", 9): 31009,     # 'C' does not differ from 'T'; no stored element outside the window
    ("limits", 11): 31011,    # 'C' does not differ from 'T'
    ("limits", 15): 31015,    # no stored element outside the window
    ("limits", 30): 31030,    # no stored element outside the window
    ("limits", 33): 31033,    # 'C' does not differ from 'T'; no stored element outside the window
    ("limits", 36): 31036,    # no stored element outside the window
    ("limits", 38): 32038,    # no stored element outside the window
    ("limits", 40): 31040,    # no stored element outside the window
    ("limits", 41): 31041,    # no stored element outside the window
    ("limits", 42): 31042,    # no stored element outside the window
    ("limits", 44): 31044,    # no stored element outside the window
    ("symmetry", 10): 41010,  # 'C' does not differ from 'T'
    ("symmetry", 15): 41015,  # 'C' does not differ from 'T'
}

Z_ALPHA = [0.0, 1.0, 2j, -0.5 + 2j, 0.75 - 0.5j, 1 + 1j]       # 0, 1, a purely imaginary value, general values
Z_ALPHA_NONZERO = Z_ALPHA[1:]
Z_BETA = [0.0, 1.0, -1j, 2 - 1j, 1.5 + 0.25j, 0.5j]
R_ALPHA = [1.0, -0.5, 0.0, 2.25]                                # (exact in float32 too)
R_BETA = [1.0, 0.0, -1.5, 0.5]
PAIRS_Z = [a + b for a in "NTC" for b in "NTC"]
PAIRS_R = [a + b for a in "NT" for b in "NT"]
LIMIT_KINDS = ("none", "aligned", "inside", "single", "full")


def count(name):
    return int(os.environ.get("DBCSR_AMD_OPTSWEEP_" + name.upper(), str(DEFAULT_COUNT[name])))


def seed_of(name, i):
    return RESEED.get((name, i), BASE_SEED[name] + i) + SWEEP_OFFSET


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


# ---- generators ---------------------------------------------------------------------------------------------------------------------------------------
def _pick(rng, seq):
    return seq[int(rng.integers(len(seq)))]


def _forced(i):
    """one case in four of strata 1 and 2 runs with the product-driven / per-word symbolic kernels forced"""
    return {"DBCSR_AMD_MM_SYMBOLIC": "rows" if i % 8 == 2 else "word"} if i % 4 == 2 else {}


def _base(name, i, dtype):
    return dict(stratum=name, i=i, seed=seed_of(name, i), dtype=dtype, limits=None, kinds=None, symm_a="N", symm_b="N", symm_c="N", env={}, eps=0.0,
                retain=False, klimits=False)


def _dense_enough(c, rng):
    """a case with 'C' must differ from its 'T' twin, which takes products: its operands are drawn from the four denser fills"""
    if "C" in c["ta"] + c["tb"]:
        c["sp"] = tuple(float(x) for x in rng.choice(FILLS[:4], size=2)) + c["sp"][2:]


def make_complex(i):
    c = _base("complex", i, Z64)
    rng = np.random.default_rng(c["seed"])
    c["mix_m"], c["mix_n"], c["mix_k"] = (_pick(rng, MIXES) for _ in range(3))
    c["M"], c["N"], c["K"] = (int(rng.integers(1, 301)) for _ in range(3))
    c["sp"] = tuple(float(x) for x in rng.choice(FILLS, size=3))
    c["ta"], c["tb"] = PAIRS_Z[(i + i // 9) % 9]
    _dense_enough(c, rng)
    # (a case with 'C' must differ from its 'T' twin: alpha == 0 would make them equal)
    c["alpha"] = complex(_pick(rng, Z_ALPHA_NONZERO if "C" in c["ta"] + c["tb"] else Z_ALPHA))
    c["beta"] = complex(_pick(rng, Z_BETA))
    c["retain"] = i % 5 == 3
    c["eps"] = float(_pick(rng, [3.0, 25.0])) if i % 3 == 1 else 0.0
    c["env"] = _forced(i)
    return c


def _mix_pool(n):
    """(mixes for m and n, mixes for k) of the n-th fp64 case of a stratum: the small mixes, every fourth case in turn the mixes of 33 ... 80 and of 33 ... 48"""
    return (MIXES, MIXES) if n % 2 == 0 else ((BIG_MIXES, BIG_MIXES) if n % 4 == 1 else (MID_MIXES, BIG_MIXES + MID_MIXES))


def _window(rng, kind, sizes):
    """(first, last), 1-based inclusive, 0 = not given, of one dimension with the given block sizes"""
    off = offsets(sizes)
    n, nb = int(off[-1]), len(sizes)
    if kind == "none":
        return 0, 0
    if kind == "full":
        return 1, n
    if kind == "single":
        e = int(rng.integers(1, n + 1))
        return e, e
    b0 = int(rng.integers(nb))
    b1 = int(rng.integers(b0, nb))
    if kind == "aligned":
        return int(off[b0]) + 1, int(off[b1 + 1])
    wide = [b for b in range(nb) if sizes[b] >= 2]
    if not wide:   # blocks of one element only: nothing ends inside a block
        return int(off[b0]) + 1, int(off[b1 + 1])
    b = wide[int(rng.integers(len(wide)))]
    last = int(off[b]) + int(rng.integers(1, sizes[b]))   # 1 ... size - 1 elements of block b
    return int(rng.integers(1, last + 1)), last


def make_limits(i):
    dtype = (F64,) * 6 + (F32,) * 2 + (Z64,) * 4
    c = _base("limits", i, dtype[i % 12])
    rng = np.random.default_rng(c["seed"])
    cplx = c["dtype"] == Z64
    mn, kk = _mix_pool(6 * (i // 12) + i % 12) if c["dtype"] == F64 else (MIXES, MIXES)
    c["mix_m"], c["mix_n"], c["mix_k"] = _pick(rng, mn), _pick(rng, mn), _pick(rng, kk)
    c["M"], c["N"], c["K"] = (int(rng.integers(1, 301)) for _ in range(3))
    c["sp"] = tuple(float(x) for x in rng.choice(FILLS, size=3))
    c["ta"], c["tb"] = _pick(rng, PAIRS_Z if cplx else PAIRS_R)
    _dense_enough(c, rng)
    c["alpha"] = complex(_pick(rng, Z_ALPHA_NONZERO if "C" in c["ta"] + c["tb"] else Z_ALPHA)) if cplx else float(_pick(rng, R_ALPHA))
    c["beta"] = complex(_pick(rng, Z_BETA)) if cplx else float(_pick(rng, R_BETA))
    c["retain"] = i % 5 == 3
    c["eps"] = float(_pick(rng, [3.0, 25.0])) if (not cplx and i % 6 == 1) else 0.0
    c["env"] = _forced(i)
    kinds = tuple(_pick(rng, LIMIT_KINDS) for _ in range(3))
    if kinds[0] in ("none", "full") and kinds[1] in ("none", "full"):
        # no row or column of C lies outside the window: nothing of a kept C could show that the outside is left alone, so such a case runs as the
        # reference runs a k window alone, beta == 0 on a C that is emptied first
        c["beta"], c["retain"] = (0j if cplx else 0.0), False
    sm, sn, sk = (O.make_block_sizes(c[d], c[m]) for d, m in (("M", "mix_m"), ("N", "mix_n"), ("K", "mix_k")))
    c["kinds"] = kinds
    c["limits"] = _window(rng, kinds[0], sm) + _window(rng, kinds[1], sn) + _window(rng, kinds[2], sk)
    return c


def make_symmetry(i):
    product, j, t = i % 4 == 3, i // 4, i - i // 4   # (j: the number of the product case, t: of the operand case)
    rng = np.random.default_rng(seed_of("symmetry", i))
    if product:   # product symmetry the other sweep does not draw: fp32 'S' / 'A', complex 'H' / 'K'
        c = _base("symmetry", i, F32 if j % 2 == 0 else Z64)
    else:
        c = _base("symmetry", i, (F64, F32, Z64)[t % 3])
    cplx = c["dtype"] == Z64
    kinds = "HK" if cplx else "SA"
    mn, kk = _mix_pool(t // 3) if c["dtype"] == F64 and not product else (MIXES, MIXES)
    c["mix_m"], c["mix_n"], c["mix_k"] = _pick(rng, mn), _pick(rng, mn), _pick(rng, kk)
    c["M"], c["N"], c["K"] = (int(rng.integers(1, 301)) for _ in range(3))
    c["sp"] = tuple(float(x) for x in rng.choice(FILLS[:5], size=3))
    c["ta"], c["tb"] = _pick(rng, PAIRS_Z if cplx else PAIRS_R)
    _dense_enough(c, rng)
    c["alpha"] = complex(_pick(rng, Z_ALPHA_NONZERO if "C" in c["ta"] + c["tb"] else Z_ALPHA)) if cplx else float(_pick(rng, R_ALPHA))
    c["beta"] = complex(_pick(rng, Z_BETA)) if cplx else float(_pick(rng, R_BETA))
    if product:
        c["symm_c"] = kinds[(j // 2) % 2]
        c["N"], c["mix_n"] = c["M"], c["mix_m"]
        c["retain"] = j % 5 == 3
        c["eps"] = float(_pick(rng, [3.0, 25.0])) if j % 5 == 1 else 0.0   # (of the default ten: one complex, one fp32)
        c["klimits"] = j % 4 == 2   # real data: the C entry that takes k limits (not given: 0, 0)
    else:
        which = ("A", "B", "AB")[(t // 3) % 3]
        if "A" in which:   # A is square: op(A) is M x K
            c["symm_a"] = _pick(rng, kinds)
            c["K"], c["mix_k"] = c["M"], c["mix_m"]
        if "B" in which:   # B is square: op(B) is K x N
            c["symm_b"] = _pick(rng, kinds)
            c["N"], c["mix_n"] = c["K"], c["mix_k"]
        c["retain"] = i % 5 == 3
    return c


def make_sizes(i):
    kind = i % 3
    rng = np.random.default_rng(seed_of("sizes", i))
    c = _base("sizes", i, F32 if kind != 1 or (i // 3) % 2 else F64)
    if kind == 0:      # fp32 blocks of 33 ... 80
        mn, kk = (BIG_MIXES, BIG_MIXES) if (i // 3) % 2 == 0 else (MID_MIXES, BIG_MIXES + MID_MIXES)
        c["mix_m"], c["mix_n"], c["mix_k"] = _pick(rng, mn), _pick(rng, mn), _pick(rng, kk)
        c["M"], c["N"], c["K"] = (int(rng.integers(1, 301)) for _ in range(3))
    elif kind == 1:    # one block size of 81 ... 128 among smaller ones, in one, two or all three dimensions
        where = int(rng.integers(1, 8))
        for b, d in enumerate(("mix_m", "mix_n", "mix_k")):
            small = _pick(rng, MIXES)
            c[d] = [1, int(rng.integers(81, 129))] + small if where >> b & 1 else small
        c["M"], c["N"], c["K"] = (int(rng.integers(100, 301)) for _ in range(3))
    else:              # the fp32 cubes 16 / 24 / 32 (k % 8 == 0), at least nine blocks in ten of that size in every dimension
        s = (16, 24, 32)[(i // 3) % 3]
        c["mix_m"] = c["mix_n"] = c["mix_k"] = [1, s]
        dims = []
        for _ in range(3):
            nb = int(rng.integers(2, 300 // s + 1))
            tail = int(rng.integers(1, s)) if nb >= 10 and nb * s + s <= 300 and rng.random() < 0.5 else 0
            dims.append(nb * s + tail)
        c["M"], c["N"], c["K"] = dims
    c["sp"] = tuple(float(x) for x in rng.choice(FILLS[:3] if kind == 2 else FILLS[:5], size=3))
    c["ta"], c["tb"] = _pick(rng, PAIRS_R)
    c["alpha"], c["beta"] = float(_pick(rng, R_ALPHA)), float(_pick(rng, R_BETA))
    c["retain"] = i % 5 == 3
    c["eps"] = float(_pick(rng, [0.0, 0.0, 0.0, 30.0]))
    return c


MAKERS = {"complex": make_complex, "limits": make_limits, "symmetry": make_symmetry, "sizes": make_sizes}


@functools.lru_cache(maxsize=None)
def case(name, i):
    return MAKERS[name](i)


def runs_both_entries(c):
    """strata 1, 2 and 4 and the products with symmetry of stratum 3 (the C entry takes no operand with symmetry)"""
    return c["stratum"] != "symmetry" or c["symm_c"] != "N"


# ---- operands ---------------------------------------------------------------------------------------------------------------------------------------------
def bcsr(M, data):
    return O.Bcsr(M.row_sizes, M.col_sizes, M.row_p, M.col_i, M.blk_p, data)


def _typed(M, dtype, seed):
    if dtype == Z64:
        return with_imag(bcsr(M, M.data.astype(np.float64)), seed)
    return bcsr(M, M.data.astype(np.float32 if dtype == F32 else np.float64))


@functools.lru_cache(maxsize=None)
def operands(name, i):
    """(A, B, C_in) on the host as they are stored (a matrix with symmetry: its triangle), in the case's data type: computed once, never written"""
    c = case(name, i)
    sm, sn, sk = O.make_block_sizes(c["M"], c["mix_m"]), O.make_block_sizes(c["N"], c["mix_n"]), O.make_block_sizes(c["K"], c["mix_k"])
    c0, dt, s = O.RANDMAT_SEED_INIT, c["dtype"], c["seed"]
    rdt = np.float32 if dt == F32 else np.float64
    tri = lambda sizes, sp, counter, symm: O.make_random_matrix_symmetric(sizes, sp, counter, "A" if symm == "A" else "S")
    if c["symm_c"] != "N":
        Cm = tri(sm, c["sp"][2], c0 + 1, c["symm_c"])
    else:
        Cm = O.make_random_matrix(sm, sn, c["sp"][2], c0 + 1, rdt)
    if c["symm_a"] != "N":
        A = tri(sm, c["sp"][0], c0 + 2, c["symm_a"])
    else:
        A = O.make_random_matrix(sk, sm, c["sp"][0], c0 + 2, rdt) if c["ta"] != "N" else O.make_random_matrix(sm, sk, c["sp"][0], c0 + 2, rdt)
    if c["symm_b"] != "N":
        B = tri(sk, c["sp"][1], c0 + 3, c["symm_b"])
    else:
        B = O.make_random_matrix(sn, sk, c["sp"][1], c0 + 3, rdt) if c["tb"] != "N" else O.make_random_matrix(sk, sn, c["sp"][1], c0 + 3, rdt)
    return _typed(A, dt, 3 * s), _typed(B, dt, 3 * s + 1), _typed(Cm, dt, 3 * s + 2)


def expanded(M, symm):
    """the full matrix of a stored triangle, as the multiply expands an operand"""
    if symm == "N":
        return M
    if symm in ("S", "A"):
        full = O.desymmetrize(M, symm)
        return bcsr(full, full.data.astype(M.data.dtype))
    return expected_full(M, symm)


# ---- dense long double ------------------------------------------------------------------------------------------------------------------------------------
def dense_ld(M):
    """M scattered to dense long double (complex: clongdouble); every conversion is exact"""
    ro, co = offsets(M.row_sizes), offsets(M.col_sizes)
    cplx = M.data.dtype.kind == "c"
    D = np.zeros((int(ro[-1]), int(co[-1])), CLD if cplx else LD)
    data = M.data.astype(CLD if cplx else LD)
    rows = M.rows()
    for b in range(M.nblks):
        r, c = int(rows[b]), int(M.col_i[b])
        m, n = int(M.row_sizes[r]), int(M.col_sizes[c])
        D[ro[r]:ro[r] + m, co[c]:co[c] + n] = data[M.blk_p[b]:M.blk_p[b] + m * n].reshape(n, m).T
    return D


def dense_native(M):
    """M scattered to dense in its own data type (for comparisons of bits)"""
    ro, co = offsets(M.row_sizes), offsets(M.col_sizes)
    D = np.zeros((int(ro[-1]), int(co[-1])), M.data.dtype)
    rows = M.rows()
    for b in range(M.nblks):
        r, c = int(rows[b]), int(M.col_i[b])
        m, n = int(M.row_sizes[r]), int(M.col_sizes[c])
        D[ro[r]:ro[r] + m, co[c]:co[c] + n] = M.data[M.blk_p[b]:M.blk_p[b] + m * n].reshape(n, m).T
    return D


def pattern(M):
    P = np.zeros((M.nbr, M.nbc), bool)
    P[M.rows(), M.col_i] = True
    return P


def spread(P, rs, cs):
    """a per-block array as a per-element one"""
    return np.repeat(np.repeat(P, rs, axis=0), cs, axis=1)


def block_sums(X, rs, cs):
    return np.add.reduceat(np.add.reduceat(X, offsets(rs)[:-1], 0), offsets(cs)[:-1], 1)


def op(D, t):
    return D if t == "N" else (D.T if t == "T" else D.conj().T)


def sq(X):
    """|x|^2 per element in long double: re^2 + im^2"""
    return X.real * X.real + X.imag * X.imag if X.dtype.kind == "c" else X * X


def twin_dense(Y, symm):
    """the twin of a block: transposed, negated for 'A' / 'K', conjugated for 'H' / 'K'"""
    T = Y.conj().T if symm in ("H", "K") else Y.T
    return -T if symm in ("A", "K") else T


def moved(D, P, sizes, move, symm):
    """the blocks (r, c) of P with move(r, c) become blocks (c, r) = twin(block); D dense, P the block pattern (square blocking)"""
    off = offsets(sizes)
    D2, P2 = D.copy(), P.copy()
    for r, c in zip(*np.nonzero(P)):
        if move(int(r), int(c)):
            rr, cc = slice(off[r], off[r + 1]), slice(off[c], off[c + 1])
            D2[rr, cc] = 0
            P2[r, c] = False
    for r, c in zip(*np.nonzero(P)):
        if move(int(r), int(c)):
            rr, cc = slice(off[r], off[r + 1]), slice(off[c], off[c + 1])
            D2[cc, rr] = twin_dense(D[rr, cc], symm)
            P2[c, r] = True
    return D2, P2


to_canonical = lambda r, c: r != c and bool(O.checker_tr(r + 1, c + 1))
to_triangle = lambda r, c: r > c


# ---- the block-level restatement -----------------------------------------------------------------------------------------------------------------------------
def window_of(c):
    """(row, column, k bounds as 0-based inclusive element indices, window_keeps, limited) after the defaults are optimised away (dbcsr_mm.F:669-704)"""
    nr, nc, nk = c["M"], c["N"], c["K"]
    fr, lr, fc, lc, fk, lk = c["limits"] or (0,) * 6
    fr, lr = (0 if fr == 1 else fr), (0 if lr == nr else lr)
    fc, lc = (0 if fc == 1 else fc), (0 if lc == nc else lc)
    fk, lk = (0 if fk == 1 else fk), (0 if lk == nk else lk)
    keeps = (0 < lc < nc) or (0 < lr < nr)
    return ((fr or 1) - 1, (lr or nr) - 1), ((fc or 1) - 1, (lc or nc) - 1), ((fk or 1) - 1, (lk or nk) - 1), keeps, any((fr, lr, fc, lc, fk, lk))


def gamma_of(c):
    (_, _, (k0, k1), _, _) = window_of(c)
    n = k1 - k0 + 1
    if c["dtype"] == Z64:
        return float(np.sqrt(2.0) * (2 * n + 10) * 2.0 ** -53)
    u = U[c["dtype"]]
    return (n + 8) * u / (1.0 - (n + 8) * u)


class Restated:
    """what restate() returns: row_p / col_i of the result, flop, R and bound (dense, in the layout the result is stored in), stored (elements of the
    result's blocks), inside (elements held to the bar: the window), and the numbers the conditions and the kernel choice need"""


def restate(c, A, B, Cm, norm_of=sq):
    """The multiply of case c on the host operands A, B, C_in (stored forms).  norm_of: |x|^2 per element of a block, the complex norm re^2 + im^2 (a
    parameter so that the CPU file can show that a norm from the real part alone would be caught)."""
    cplx = c["dtype"] == Z64
    fa, fb = expanded(A, c["symm_a"]), expanded(B, c["symm_b"])
    Ad, Bd = op(dense_ld(fa), c["ta"]), op(dense_ld(fb), c["tb"])
    PA, PB = (pattern(fa) if c["ta"] == "N" else pattern(fa).T), (pattern(fb) if c["tb"] == "N" else pattern(fb).T)
    rs, ks = (fa.row_sizes, fa.col_sizes) if c["ta"] == "N" else (fa.col_sizes, fa.row_sizes)
    cs = fb.col_sizes if c["tb"] == "N" else fb.row_sizes
    assert np.array_equal(rs, Cm.row_sizes) and np.array_equal(cs, Cm.col_sizes) and np.array_equal(ks, fb.row_sizes if c["tb"] == "N" else fb.col_sizes)
    Cd, PC = dense_ld(Cm), pattern(Cm)
    symm_c, alpha, beta, eps, retain = c["symm_c"], c["alpha"], c["beta"], c["eps"], c["retain"]
    if symm_c != "N":
        Cd, PC = moved(Cd, PC, rs, to_canonical, symm_c)
    (r0, r1), (c0, c1), (k0, k1), window_keeps, limited = window_of(c)
    keep_data = bool(retain) or beta != 0 or window_keeps
    if not keep_data:
        Cd, PC = np.zeros_like(Cd), np.zeros_like(PC)
    ro, co, ko = offsets(rs), offsets(cs), offsets(ks)
    rin, cin, kin = ((np.arange(n) >= lo) & (np.arange(n) <= hi) for n, lo, hi in ((ro[-1], r0, r1), (co[-1], c0, c1), (ko[-1], k0, k1)))
    hit = lambda off, lo, hi: (off[1:] - 1 >= lo) & (off[:-1] <= hi)   # blocks that intersect the bounds
    Aw, Bw = Ad * np.outer(rin, kin), Bd * np.outer(kin, cin)           # dbcsr_crop_matrix: the outside of a boundary block is cleared
    PAw, PBw = PA & np.outer(hit(ro, r0, r1), hit(ko, k0, k1)), PB & np.outer(hit(ko, k0, k1), hit(co, c0, c1))
    inside = np.outer(rin, cin)
    R = Cd.copy()
    if keep_data:
        R[inside] = (beta * Cd)[inside]
    bound = np.abs(R).astype(LD)
    nbr, nbc, nbk = len(rs), len(cs), len(ks)
    allowed = np.ones((nbr, nbc), bool)
    if symm_c != "N":   # canonical form: the blocks whose twin is the stored one are left out (dbcsr_mm_csr.F:280-292)
        ii, jj = np.meshgrid(np.arange(nbr), np.arange(nbc), indexing="ij")
        allowed &= ~((ii != jj) & ((((ii + jj) & 1) == 1) == (jj >= ii)))
    if retain:
        allowed &= PC
    out = Restated()
    iA, iB = PAw.astype(np.int64), PBw.astype(np.int64)
    out.products_unfiltered = int(((iA @ iB) * allowed).sum())
    out.blocks_unfiltered = int((PC | (((iA @ iB) > 0) & allowed)).sum())
    area = np.outer(rs.astype(np.int64), cs.astype(np.int64))
    out.norms = []
    if eps > 0:
        NA = block_sums(norm_of(Aw), rs, ks)
        NB = (abs(alpha) ** 2) * block_sums(norm_of(Bw), ks, cs)
        out.norms = [NA[PAw], NB[PBw]]
        na32, nb32 = NA.astype(np.float32), NB.astype(np.float32)
        cnt = PAw.sum(axis=1)
        e = np.float32(eps) / np.maximum(cnt, 1).astype(np.float32)
        row_eps = (e * e).astype(np.float32)
        has = np.zeros((nbr, nbc), bool)
        flop = nprod = 0
        for kb in range(nbk):
            kept = np.outer(PAw[:, kb], PBw[kb, :]) & allowed & ~(np.outer(na32[:, kb], nb32[kb, :]).astype(np.float32) < row_eps[:, None])
            if not kept.any():
                continue
            ksl = slice(ko[kb], ko[kb + 1])
            el = spread(kept, rs, cs)
            R += alpha * ((Aw[:, ksl] @ Bw[ksl, :]) * el)
            bound += abs(alpha) * ((np.abs(Aw[:, ksl]) @ np.abs(Bw[ksl, :])) * el)
            has |= kept
            nprod += int(kept.sum())
            flop += 2 * int(ks[kb]) * int((area * kept).sum())
    else:
        has = ((iA @ iB) > 0) & allowed
        el = spread(allowed, rs, cs)
        R += alpha * ((Aw @ Bw) * el)
        bound += abs(alpha) * ((np.abs(Aw) @ np.abs(Bw)) * el)
        nprod = out.products_unfiltered
        flop = 2 * int(((((rs.astype(np.int64)[:, None] * iA) * ks.astype(np.int64)[None, :]) @ iB) * cs.astype(np.int64)[None, :] * allowed).sum())
    P = PC | has
    out.result_norms = np.zeros(0, LD)
    if eps > 0 and not retain:   # the final filter: ||blk||^2 < eps^2 goes
        n2 = block_sums(norm_of(R), rs, cs)
        out.result_norms = n2[P]
        P = P & ~(n2 < LD(eps) * LD(eps))
    out.canonical_pattern = P
    if symm_c != "N":   # back to the stored triangle
        R, _ = moved(R, P, rs, to_triangle, symm_c)
        bound, P = moved(bound, P, rs, to_triangle, "S")
        inside = np.ones_like(inside)
    out.flop, out.nproducts = int(flop), int(nprod)
    out.pattern = P
    out.row_p = np.concatenate([[0], np.cumsum(P.sum(axis=1))]).astype(np.int32)
    out.col_i = np.nonzero(P)[1].astype(np.int32)
    out.R, out.bound, out.stored, out.inside = R, bound, spread(P, rs, cs), inside
    out.keep_data, out.limited = keep_data, limited
    out.gamma = gamma_of(c)
    out.cplx = cplx
    return out


@functools.lru_cache(maxsize=None)
def reference(name, i):
    """restate() of a case, computed once: the two entries share it"""
    return restate(case(name, i), *operands(name, i))


# ---- the oracle's index and flop ---------------------------------------------------------------------------------------------------------------------------
def oracle_result(c, A, B, Cm):
    """(result, info) of the oracle for a case.  Real data: O.multiply / O.multiply_limits on the desymmetrized operands in float64, c_symmetry for a
    product with symmetry.  Complex data: the same on the REAL PARTS with alpha = 1 and beta 0 / 1 ('C' is 'T' there) -- index and flop only, and only
    without a filter (the pattern then does not depend on the values)."""
    cplx = c["dtype"] == Z64
    fa, fb = expanded(A, c["symm_a"]), expanded(B, c["symm_b"])
    if cplx:
        assert c["eps"] == 0
        w = lambda M: part(M, M.data.real)
        alpha, beta = 1.0, (0.0 if c["beta"] == 0 else 1.0)
    else:
        w = lambda M: bcsr(M, M.data.astype(np.float64))
        alpha, beta = c["alpha"], c["beta"]
    real = lambda t: "T" if t == "C" else t
    if c["limits"] is not None:
        return O.multiply_limits(real(c["ta"]), real(c["tb"]), alpha, w(fa), w(fb), beta, w(Cm), c["limits"], retain_sparsity=c["retain"], filter_eps=c["eps"])
    symm = None if c["symm_c"] == "N" else ("A" if c["symm_c"] == "A" else "S")
    return O.multiply(real(c["ta"]), real(c["tb"]), alpha, w(fa), w(fb), beta, w(Cm), retain_sparsity=c["retain"], filter_eps=c["eps"], c_symmetry=symm)


@functools.lru_cache(maxsize=None)
def expected_index(name, i):
    """(row_p, col_i, flop) a device result must have: the oracle's for real data and for complex data without a filter, the restatement's for complex
    data with filter_eps"""
    c = case(name, i)
    if c["dtype"] == Z64 and c["eps"] > 0:
        r = reference(name, i)
        return r.row_p, r.col_i, r.flop
    ref, info = oracle_result(c, *operands(name, i))
    return ref.row_p, ref.col_i, int(info["flop"])


# ---- the comparison -----------------------------------------------------------------------------------------------------------------------------------------
def compare(name, i, got, flop):
    """None when the result `got` (a host Bcsr in the case's data type) and its flop count meet the reference, else a dict that says what differs.
    The second value: worst err / bar over the elements held to the bar (0 without any)."""
    c, ref = case(name, i), reference(name, i)
    A, B, Cm = operands(name, i)
    row_p, col_i, want_flop = expected_index(name, i)
    if not (np.array_equal(got.row_p, row_p) and np.array_equal(got.col_i, col_i)):
        return {"what": "index", "nblks_device": int(got.col_i.size), "nblks_reference": int(col_i.size)}, 0.0
    if int(flop) != want_flop:
        return {"what": "flop", "device": int(flop), "reference": want_flop}, 0.0
    G = dense_ld(got)
    held = ref.stored & ref.inside
    err, bar = np.abs(G - ref.R)[held], ref.gamma * ref.bound[held]
    worst = 0.0
    if err.size:
        ratio = np.where(bar > 0, err / np.where(bar > 0, bar, 1), np.where(err > 0, np.inf, 0.0))
        w = int(np.argmax(np.where(np.isnan(ratio), np.inf, ratio)))
        worst = float(ratio[w])
        if not worst <= 1.0:   # (a NaN fails too)
            return {"what": "values", "error": float(err[w]), "bar": float(bar[w]), "count_above_bar": int(np.sum(~(ratio <= 1.0))),
                    "gamma": ref.gamma}, worst
    outside = ref.stored & ~ref.inside
    if outside.any():   # outside the window a kept C keeps its bits; what C_in does not hold there is zero
        Gn, Cn, had = dense_native(got), dense_native(Cm), spread(pattern(Cm), Cm.row_sizes, Cm.col_sizes) & ref.keep_data
        same = Gn[outside & had].tobytes() == Cn[outside & had].tobytes()
        if not same or np.any(Gn[outside & ~had] != 0):
            return {"what": "bits outside the window", "elements": int(np.sum(outside))}, worst
    return None, worst


# ---- conditions on the inputs -----------------------------------------------------------------------------------------------------------------------------------
def near_float32_midpoint(x, rel=1e-12):
    """True where the long double x lies within rel of the midpoint of two adjacent float32 values (its rounding to float32 could go either way)"""
    x = np.asarray(x, LD)
    f = x.astype(np.float32)
    bad = np.zeros(x.shape, bool)
    for other in (np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))):
        mid = (f.astype(LD) + other.astype(LD)) / 2
        ok = np.isfinite(mid) & (mid != 0)
        bad |= ok & (np.abs(x - mid) <= rel * np.abs(np.where(ok, mid, 1)))
    return bad


def twin_case(c):
    """the same case with 'C' replaced by 'T'"""
    return dict(c, ta=c["ta"].replace("C", "T"), tb=c["tb"].replace("C", "T"))


def cuts_inside(c):
    """per dimension: does a bound of the window (after the defaults are optimised away) fall inside a block?"""
    (r0, r1), (c0, c1), (k0, k1), _, _ = window_of(c)
    out = []
    for (lo, hi), n, mix in (((r0, r1), c["M"], c["mix_m"]), ((c0, c1), c["N"], c["mix_n"]), ((k0, k1), c["K"], c["mix_k"])):
        edges = set(offsets(O.make_block_sizes(n, mix)).tolist())
        out.append(lo not in edges or hi + 1 not in edges)
    return out


def conditions(name, i):
    """the names of the conditions on the inputs that case (name, i) fails (empty: a good case)"""
    c, ref = case(name, i), reference(name, i)
    A, B, Cm = operands(name, i)
    failed = []
    if any(np.any(near_float32_midpoint(n)) for n in ref.norms):
        failed.append("a block norm at a float32 rounding midpoint")
    if c["eps"] > 0 and ref.result_norms.size:
        e2 = LD(c["eps"]) ** 2
        if np.any(np.abs(ref.result_norms - e2) <= 1e-9 * e2):
            failed.append("a result block norm at eps^2")
    if "C" in c["ta"] + c["tb"]:
        t = restate(twin_case(c), A, B, Cm)
        both = ref.stored & t.stored & ref.inside
        if not np.any(np.abs(ref.R - t.R)[both] > 1e3 * ref.gamma * ref.bound[both]):
            failed.append("'C' does not differ from 'T'")
    if c["limits"] is not None and ref.keep_data:
        stored_in = spread(pattern(Cm), Cm.row_sizes, Cm.col_sizes)
        if not np.any(stored_in & ~ref.inside):
            failed.append("no stored element outside the window")
    return failed


# ---- the kernel choice -----------------------------------------------------------------------------------------------------------------------------------------
def family(kernel):
    """the kernel family of a last_kernel() / mm_choose.h name: family_of of tests/engine_sequences.py, with the generic kernels and the fp32 families
    told apart by type"""
    from tests.engine_sequences import family_of
    if kernel in ("mm_numeric_f64", "mm_numeric_f32"):
        return kernel[len("mm_numeric_"):] + "_generic"
    fam = family_of(kernel)
    if fam == "f32":
        return kernel[len("mm_numeric_"):].split("<")[0].split("[")[0]
    return fam if fam in ("z64", "classes") else "f64_" + fam


def choice_case(name, i):
    """(case tuple, keyword facts) for `choose` of tests/test_numeric_choice.py, or None where the host build of mm_choose.h cannot answer: complex data
    (one family), a product with symmetry (canonical index), a product without a block (no numeric phase)"""
    c = case(name, i)
    if c["dtype"] == Z64 or c["symm_c"] != "N":
        return None
    ref = reference(name, i)
    if ref.blocks_unfiltered == 0:
        return None
    q = (c["M"], c["N"], c["K"], 0, 0, 0, c["mix_m"], c["mix_n"], c["mix_k"])
    return q, dict(c_nblks=ref.blocks_unfiltered, products_per_block=ref.products_unfiltered / ref.blocks_unfiltered, fp64=c["dtype"] == F64,
                   retain=bool(c["retain"]), filter_active=c["eps"] > 0)
