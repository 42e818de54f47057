"""The block diagonal on the device (dbcsr_amd/operations.py: dbcsr_get_block_diag, dbcsr_invert_block_diag; dbcsr_amd_bcsr_block_diag_count / _apply /
_invert of include/dbcsr_amd_mm.h; kernels of dbcsr_amd/csrc/mm_block_inverse.h) for float64, float32 and complex128.

Reference and bar of an inverse, per element (reference_of, bar_of; tests/test_block_inverse_cpu.py checks both without a GPU):
    X   = numpy.linalg.inv(A) refined by three steps X <- X + X (I - A X) in long double, A in the exact values of its type
    w   = |X| |A| |X| (componentwise, float64)
    bar = K n 2^-53 w                   + 2^-24 |X| for float32, the one final rounding
the first-order forward bound of an inversion with backward-stable factors.  K is MEASURED on the inputs, never on the kernel's results: measured_K()
forms the inverse of every block of the input set in plain double with LAPACK (numpy.linalg.inv) and with gauss_jordan below, the algorithm restated in
numpy, and K is the smallest power of two that is at least four times the worst ratio |got - X| / (n 2^-53 w) either reaches (the four: the kernel's
different but equally valid order of operations).  Measured on the 3 families x 16 dimensions x 3 types below: worst ratio 0.637 for LAPACK and 0.637
for the restated Gauss-Jordan (both at n = 1, family permuted, float64: the one rounding of the reciprocal; every larger block stays below that), so
K = 4 (profiles/block_inverse.txt; tests/test_block_inverse_cpu.py measures it again on every run).

The input set: block(family, n, type) for the families spd (G G^H / n + I / 2), permuted ((R + n I / 2) with its rows in a random permutation without a
fixed point: elimination without pivoting meets pivots near zero; block() says which draw is taken) and general (U diag(logspace(0, -3, n)) V, U and V orthogonal / unitary), elements of R
and G uniform in [-1, 1] per component; dimensions DIMS: both sides of the boundary between the wave and the workgroup kernel, the tile-like sizes and
their neighbours, the limit.  Every matrix of this file takes its diagonal blocks from that set (diagonal_matrix, full_matrix, overlap_matrix), so K
covers them all.  `mixed` of tests/test_gpu_matrix_norms.py is a rectangular matrix (230 x 260 with different row and column block sizes), which neither
function accepts; it serves the refusals, and full_matrix() -- a square matrix with ten block sizes of both paths, blocks off the diagonal and a block
row without a diagonal block -- stands where a `mixed` matrix has to be square."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from dbcsr_amd.matrix import DbcsrMatrix, StreamHandle
from dbcsr_amd.multiply import MultiplyEngine, dbcsr_multiply
from dbcsr_amd.operations import dbcsr_add_on_diag, dbcsr_frobenius_norm, dbcsr_get_block_diag, dbcsr_invert_block_diag, dbcsr_multivec
from oracle import oracle as O
from tests import far_arena as FA
from tests.gpu_util import dev_to_bcsr, to_dev
from tests.test_gpu_matrix_norms import (base, blocks_of, dense, from_blocks, hole_positions, misaligned, same_bits, subset, symmetric_base, typed,
                                         with_holes)
from tests.test_gpu_matvec import U53, dense_parts
from tests.test_gpu_multivec import Dev, random_vectors, reference_columns, within_columns

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32, np.complex128]
IDS = ["fp64", "fp32", "z64"]
FAMILIES = ("spd", "permuted", "general")
DIMS = (1, 2, 3, 5, 13, 16, 17, 23, 31, 32, 33, 40, 64, 65, 80, 96)
K = 4
CANARY = -77.25
GUARD = 64   # canary elements on either side of a data area (a multiple of 16 bytes in every type)


@pytest.fixture(scope="module")
def eng():
    return MultiplyEngine()


# ---- host helpers (tests/test_block_inverse_cpu.py checks them without a GPU) ---------------------------------------------------------------------------
def is_complex(dtype):
    return np.dtype(dtype).kind == "c"


def wide(dtype):
    return np.clongdouble if is_complex(dtype) else np.longdouble


def uniform(rng, shape, cplx):
    x = rng.uniform(-1.0, 1.0, shape)
    return x + 1j * rng.uniform(-1.0, 1.0, shape) if cplx else x


def draw(family, n, cplx, seed):
    rng = np.random.default_rng([FAMILIES.index(family), n, int(cplx), seed])
    if family == "spd":
        G = uniform(rng, (n, n), cplx)
        return G @ G.conj().T / n + 0.5 * np.eye(n)
    if family == "permuted":
        perm = rng.permutation(n)
        while n > 1 and np.any(perm == np.arange(n)):
            perm = rng.permutation(n)
        return (uniform(rng, (n, n), cplx) + 0.5 * n * np.eye(n))[perm]
    U, V = np.linalg.qr(uniform(rng, (n, n), cplx))[0], np.linalg.qr(uniform(rng, (n, n), cplx))[0]
    return U @ np.diag(np.logspace(0.0, -3.0, n)) @ V


def breaks_without_pivoting(A):
    """the restated elimination WITHOUT pivoting misses the bar on this block (or meets a zero pivot)"""
    X, w = reference_of(A)
    got = gauss_jordan(A, pivoting=False)[0]
    return got is None or bool(np.any(np.abs(got.astype(X.dtype) - X).astype(np.float64) > bar_of(A, X, w)))


@functools.lru_cache(maxsize=None)
def block(family, n, dtype_name):
    """The n x n block of the family in the data type (float32: the float64 block rounded; the rounded values are the block).  spd and general: the
    first draw.  permuted, n >= 2: the first draw on which the restated elimination without pivoting misses the bar in float64 / complex128 -- a draw
    whose diagonal after the permutation holds a pivot near zero, which is what the family is for (the draws are uniform: most have none that small at
    n = 2 or 3).  Chosen with the restated algorithm on the host, never with the kernel."""
    dtype = np.dtype(dtype_name)
    cplx = is_complex(dtype)
    seed = 0
    A = draw(family, n, cplx, seed)
    while family == "permuted" and n >= 2 and not breaks_without_pivoting(A):
        seed += 1
        A = draw(family, n, cplx, seed)
    A = np.ascontiguousarray(A.astype(dtype))
    assert np.linalg.cond(A.astype(np.complex128 if cplx else np.float64)) <= 1.0e3 * (1 + 1e-3), (family, n, dtype_name, seed)   # (10^3; the rounding to float32 moves it in the fifth digit)
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def _reference_of(key, shape, dtype_name):
    A = np.frombuffer(key, np.dtype(dtype_name)).reshape(shape)
    W = wide(A.dtype)
    Aw = A.astype(W)
    X = np.linalg.inv(A.astype(np.complex128 if is_complex(A.dtype) else np.float64)).astype(W)
    eye = np.eye(shape[0], dtype=W)
    for _ in range(3):
        X = X + X @ (eye - Aw @ X)
    w = (np.abs(X) @ np.abs(Aw) @ np.abs(X)).astype(np.float64)
    return X, w


def reference_of(A):
    """(X in long double, w = |X| |A| |X| in float64) of the block A in the exact values of its type; formed once per block"""
    return _reference_of(np.ascontiguousarray(A).tobytes(), A.shape, A.dtype.name)


def bar_of(A, X, w):
    bar = K * A.shape[0] * U53 * w
    if A.dtype == np.float32:
        bar = bar + 2.0 ** -24 * np.abs(X).astype(np.float64)
    return bar


def gauss_jordan(A, pivoting=True):
    """(inverse, None), or (None, k) when column k has no pivot: Gauss-Jordan in place in float64 / complex128 with partial pivoting -- the largest |x|
    (complex: |re| + |im|) at or below the diagonal, compared with > against 0 so that a NaN never wins, the lowest row on ties --, the row exchanges
    undone on the columns at the end.  pivoting=False takes the diagonal element whatever it is (it must still be > 0 in modulus)."""
    a = np.array(A, dtype=np.complex128 if is_complex(A.dtype) else np.float64)
    n = a.shape[0]
    piv = []
    for k in range(n):
        mag = np.abs(a[k:, k].real) + np.abs(a[k:, k].imag)
        best, p = 0.0, None
        for i in range(n - k if pivoting else 1):
            if mag[i] > best:
                best, p = mag[i], k + i
        if p is None:
            return None, k
        piv.append(p)
        if p != k:
            a[[k, p]] = a[[p, k]]
        pinv = 1.0 / a[k, k]
        f = a[:, k].copy()
        f[k] = 0.0
        a[:, k] = 0.0
        a[k, k] = 1.0
        r = a[k] * pinv
        a -= np.outer(f, r)
        a[k] = r
    for k in reversed(range(n)):
        if piv[k] != k:
            a[:, [k, piv[k]]] = a[:, [piv[k], k]]
    return a, None


def ratio_of(got, A):
    """max |got - X| / (n 2^-53 w) of an inverse formed in double (before any rounding to float32)"""
    X, w = reference_of(A)
    return float(np.max(np.abs(got.astype(X.dtype) - X).astype(np.float64) / (A.shape[0] * U53 * w)))


def input_set():
    return [(f, n, np.dtype(d).name) for d in DTYPES for f in FAMILIES for n in DIMS]


def measured_K():
    """(K, worst ratio of LAPACK, worst ratio of the restated Gauss-Jordan) over the input set"""
    lap = gj = 0.0
    for key in input_set():
        A = block(*key)
        D = A.astype(np.complex128 if is_complex(A.dtype) else np.float64)
        lap = max(lap, ratio_of(np.linalg.inv(D), A))
        gj = max(gj, ratio_of(gauss_jordan(A)[0], A))
    k = 1
    while k < 4 * max(lap, gj):
        k *= 2
    return k, lap, gj


def column_major(A):
    return np.ascontiguousarray(A.T).reshape(-1)


def block_of_data(data, n):
    return np.asarray(data).reshape(n, n).T


def family_of_row(r):
    return FAMILIES[r % 3]


def diagonal_matrix(sizes, dtype, family=None, special=None):
    """the block-diagonal matrix of block(family or the row's, size, type); special: {block row: block} in place of the family's"""
    sizes = np.asarray(sizes, np.int32)
    blocks = {(r, r): column_major(block(family or family_of_row(r), int(n), np.dtype(dtype).name)) for r, n in enumerate(sizes)}
    for r, A in (special or {}).items():
        blocks[(r, r)] = column_major(np.asarray(A, dtype))
    return from_blocks(sizes, sizes, blocks, dtype)


FULL_SIZES = (13, 5, 23, 32, 1, 33, 17, 40, 3, 2)
FULL_NO_DIAGONAL = 6   # the block row of full_matrix() without a diagonal block


@functools.lru_cache(maxsize=None)
def full_matrix(dtype_name):
    """A square matrix of ten block rows (sizes FULL_SIZES: both paths), diagonal blocks from the families except in block row FULL_NO_DIAGONAL, and about
    half of the blocks off the diagonal, uniform in [-1, 1]"""
    dtype = np.dtype(dtype_name)
    sizes = np.asarray(FULL_SIZES, np.int32)
    rng = np.random.default_rng(77)
    blocks = {}
    for r in range(len(sizes)):
        for c in range(len(sizes)):
            if r == c and r != FULL_NO_DIAGONAL:
                blocks[(r, c)] = column_major(block(family_of_row(r), int(sizes[r]), dtype.name))
            elif r != c and rng.random() < 0.5:
                blocks[(r, c)] = uniform(rng, int(sizes[r]) * int(sizes[c]), is_complex(dtype)).astype(dtype)
    return from_blocks(sizes, sizes, blocks, dtype)


def check_inverses(M_before, M_after, what, skip=()):
    """every diagonal block of M_after (host) is within its bar of the inverse of M_before's; returns the worst error / bar"""
    before, after = blocks_of(M_before), blocks_of(M_after)
    worst = 0.0
    for (r, c), data in before.items():
        if r != c or r in skip:
            continue
        n = int(M_before.row_sizes[r])
        A = block_of_data(data, n)
        X, w = reference_of(A)
        err = np.abs(block_of_data(after[(r, r)], n).astype(X.dtype) - X).astype(np.float64)
        bar = bar_of(A, X, w)
        q = float(np.max(err / bar))
        worst = max(worst, q)
        assert np.all(err <= bar), "%s: block row %d (n = %d): error / bar = %.3f" % (what, r, n, q)
    print("%s: worst error / bar %.3f" % (what, worst))
    return worst


def others_kept(M_before, M_after):
    """every block off the diagonal bit for bit"""
    after = blocks_of(M_after)
    return all(same_bits(v, after[k]) for k, v in blocks_of(M_before).items() if k[0] != k[1])


# ---- device helpers -------------------------------------------------------------------------------------------------------------------------------------
def placed(dM, shift):
    """the same matrix with its data area GUARD + shift elements into an allocation full of canaries (shift 1: not 16-byte aligned for float64 / float32)"""
    n = dM.data.numel()
    big = torch.full((n + 2 * GUARD + 4,), CANARY, dtype=dM.data.dtype, device=dM.data.device)
    view = big[GUARD + shift:GUARD + shift + n]
    view.copy_(dM.data)
    assert shift == 0 or dM.data.is_complex() or view.data_ptr() % 16 != 0
    out = DbcsrMatrix(dM.row_blk_size, dM.col_blk_size, dM.row_p, dM.col_i, dM.blk_p, view, nze=dM.nze)
    out.symmetry = dM.symmetry
    return out, big


def check_block_diag(eng, M, dM, symmetry="N"):
    """dbcsr_get_block_diag(dM) against the host matrix M (dM's index and values): index, bits, packed, symmetry, source untouched"""
    dM.symmetry = symmetry
    stamp, before = dM.index_stamp(), dM.data.clone()
    D = dbcsr_get_block_diag(dM, engine=eng)
    torch.cuda.synchronize()
    assert isinstance(D, DbcsrMatrix) and D.symmetry == symmetry and D.dtype == dM.dtype and D.name == dM.name
    assert D.row_blk_size is dM.row_blk_size and D.col_blk_size is dM.col_blk_size
    assert dM.index_stamp() == stamp and same_bits(dM.data.cpu().numpy(), before.cpu().numpy()), "the source is only read (its holes included)"
    want = subset(M, lambda r, c: r == c)
    H = dev_to_bcsr(D)
    assert D.packed and D.nze == want.data.size
    assert np.array_equal(H.row_p, want.row_p) and np.array_equal(H.col_i, want.col_i) and np.array_equal(H.blk_p, want.blk_p)
    assert same_bits(H.data, want.data), "bit-for-bit copies of the diagonal blocks, in block-row order"
    return D


# ---- 1. get_block_diag ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("which", ["square", "full", "subset", "holes", "misaligned", "empty"])
def test_get_block_diag(eng, dtype, which):
    dtype = np.dtype(dtype)
    M = full_matrix(dtype.name) if which in ("full", "holes", "misaligned") else typed(base("square"), dtype, 1)
    have = sum(1 for r, c in blocks_of(M) if r == c)
    assert 0 < have < M.nbr, "diagonal blocks present, and missing"
    if which == "subset":
        M = subset(M, lambda r, c: r != c or r % 3 == 1)
        assert 0 < sum(1 for r, c in blocks_of(M) if r == c) < have
    if which == "empty":
        M = subset(M, lambda r, c: False)
    if which == "holes":
        M, dM = with_holes(eng, M, dtype)
        assert hole_positions(M).size > 0
    else:
        dM = to_dev(M, name="a name")
    if which == "misaligned":
        dM = misaligned(dM)
    D = check_block_diag(eng, M, dM)
    assert D.nblks == (0 if which == "empty" else sum(1 for r, c in blocks_of(M) if r == c))


@pytest.mark.parametrize("dtype,symmetry", [(np.float64, "S"), (np.float32, "S"), (np.float64, "A"), (np.complex128, "H"), (np.complex128, "K")],
                         ids=["fp64_S", "fp32_S", "fp64_A", "z64_H", "z64_K"])
def test_get_block_diag_of_a_stored_triangle(eng, dtype, symmetry):
    M = typed(symmetric_base(symmetry), dtype, 3)
    assert any(r == c for r, c in blocks_of(M)) and all(r <= c for r, c in blocks_of(M))
    check_block_diag(eng, M, to_dev(M), symmetry)


# ---- 2. the inverse against the bar --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("family", FAMILIES)
def test_inverse_of_every_dimension(eng, dtype, family):
    """one block-diagonal matrix whose block sizes are all of DIMS: the wave kernel and the workgroup kernel in one call"""
    M = diagonal_matrix(DIMS, dtype, family)
    dM = to_dev(M)
    assert dbcsr_invert_block_diag(dM, engine=eng) == (0, -1)
    torch.cuda.synchronize()
    check_inverses(M, dev_to_bcsr(dM), "%s, %s" % (family, np.dtype(dtype).name))


# ---- 3. in place inside a full matrix ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_in_place_inside_a_full_matrix_with_holes(eng, dtype):
    dtype = np.dtype(dtype)
    M, dH = with_holes(eng, full_matrix(dtype.name), dtype)
    holes = hole_positions(M)
    assert holes.size > 0 and any(r != c for r, c in blocks_of(M))
    dM, big = placed(dH, 1)
    before = big.cpu().numpy().copy()
    stamp = dM.index_stamp()
    assert dbcsr_invert_block_diag(dM, engine=eng) == (0, -1)
    torch.cuda.synchronize()
    after = big.cpu().numpy()
    assert dM.index_stamp() == stamp
    H = dev_to_bcsr(dM)
    check_inverses(M, H, "inside a full matrix, %s" % dtype.name)
    inside = np.zeros(after.size, bool)
    rows = M.rows()
    for b in range(M.nblks):
        if rows[b] == M.col_i[b]:
            n = int(M.row_sizes[rows[b]])
            inside[GUARD + 1 + M.blk_p[b]:GUARD + 1 + M.blk_p[b] + n * n] = True
    assert inside.sum() == sum(int(n) ** 2 for r, n in enumerate(FULL_SIZES) if r != FULL_NO_DIAGONAL)
    assert same_bits(after[~inside], before[~inside]), "blocks off the diagonal, holes and canaries keep their bits"


def test_a_multiply_reuses_its_plan_after_the_inversion(monkeypatch):
    monkeypatch.delenv("DBCSR_AMD_MM_PLAN", raising=False)
    eng = MultiplyEngine()
    M = full_matrix("float64")
    dA, dB = to_dev(M), to_dev(M)
    dC = to_dev(subset(M, lambda r, c: False))
    dbcsr_multiply("N", "N", 1.0, dA, dB, 0.0, dC, engine=eng)
    assert eng.plan_stats() == (0, 1)
    stamp = dA.index_stamp()
    assert dbcsr_invert_block_diag(dA, engine=eng) == (0, -1)
    D = dbcsr_get_block_diag(dA, engine=eng)
    assert dA.index_stamp() == stamp and D.nblks == len(FULL_SIZES) - 1
    dbcsr_multiply("N", "N", 1.0, dA, dB, 0.0, dC, engine=eng)
    assert eng.plan_stats() == (1, 1), "a multiply after the inversion and after get_block_diag must reuse its plan"
    torch.cuda.synchronize()
    got, ref = dense(dev_to_bcsr(dC)), dense(dev_to_bcsr(dA)) @ dense(M)
    assert np.max(np.abs(got - ref)) <= 1e-10 * np.max(np.abs(ref))


# ---- 4. the same bits -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_same_bits_wherever_the_block_lies(eng, dtype):
    """two calls on copies; the blocks alone in a block-diagonal matrix and inside the full matrix; aligned and misaligned data areas"""
    dtype = np.dtype(dtype)
    M = full_matrix(dtype.name)
    alone = subset(M, lambda r, c: r == c)
    got = {}
    for name, host, shift in (("full", M, 0), ("full again", M, 0), ("full, misaligned", M, 1), ("alone", alone, 0), ("alone, misaligned", alone, 1),
                              ("alone, misaligned by three", alone, 3)):
        dM, _ = placed(to_dev(host), shift)
        assert dbcsr_invert_block_diag(dM, engine=eng) == (0, -1)
        torch.cuda.synchronize()
        got[name] = {k: v.copy() for k, v in blocks_of(dev_to_bcsr(dM)).items() if k[0] == k[1]}
    first = got.pop("full")
    assert len(first) == len(FULL_SIZES) - 1
    for name, blocks in got.items():
        assert blocks.keys() == first.keys() and all(same_bits(blocks[k], first[k]) for k in first), name


# ---- 5. singular and non-finite blocks ----------------------------------------------------------------------------------------------------------------------
SINGULAR_SIZES = (5, 13, 23, 16, 33, 40, 17, 3)


def singular_matrix(dtype):
    """block row 2 all zeros, block row 5 with one exactly zero column; the others from the families"""
    zero_column = np.array(block("general", SINGULAR_SIZES[5], np.dtype(dtype).name))
    zero_column[:, 7] = 0
    return diagonal_matrix(SINGULAR_SIZES, dtype, special={2: np.zeros((SINGULAR_SIZES[2],) * 2), 5: zero_column})


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_singular_blocks_are_left_alone_and_counted(eng, dtype):
    M = singular_matrix(dtype)
    dM, big = placed(to_dev(M), 1)
    assert dbcsr_invert_block_diag(dM, engine=eng) == (2, 2)
    torch.cuda.synchronize()
    H = dev_to_bcsr(dM)
    for r in (2, 5):
        assert same_bits(blocks_of(H)[(r, r)], blocks_of(M)[(r, r)]), "a singular block keeps its bits"
    check_inverses(M, H, "beside singular blocks", skip=(2, 5))
    canaries = big.cpu().numpy()
    assert same_bits(canaries[:GUARD + 1], np.full(GUARD + 1, CANARY, canaries.dtype)) and same_bits(canaries[GUARD + 1 + M.data.size:],
                                                                                                   np.full(GUARD + 3, CANARY, canaries.dtype))
    # without the check: None, and the same data
    dN = to_dev(M)
    assert dbcsr_invert_block_diag(dN, check=False, engine=eng) is None
    torch.cuda.synchronize()
    assert same_bits(dev_to_bcsr(dN).data, H.data)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_nan_stays_inside_its_block(eng, dtype):
    M = singular_matrix(dtype)
    data = M.data.copy()
    nan_row, all_nan_row = 1, 6
    data[M.blk_p[nan_row] + 17] = np.nan
    data[M.blk_p[all_nan_row]:M.blk_p[all_nan_row] + SINGULAR_SIZES[all_nan_row] ** 2] = np.nan
    N = O.Bcsr(M.row_sizes, M.col_sizes, M.row_p, M.col_i, M.blk_p, data)
    dM, big = placed(to_dev(N), 1)
    # a block of NaN has no pivot: singular, like the two others.  The block with one NaN gets no promise: the NaN spreads, and when a whole pivot column
    # has become NaN the block is singular too -- then it is counted (it is the first such block row) and keeps its bits
    got = dbcsr_invert_block_diag(dM, engine=eng)
    assert got in ((3, 2), (4, nan_row)), got
    torch.cuda.synchronize()
    H = dev_to_bcsr(dM)
    for r in (2, 5, all_nan_row) + ((nan_row,) if got[0] == 4 else ()):
        assert same_bits(blocks_of(H)[(r, r)], blocks_of(N)[(r, r)])
    check_inverses(M, H, "beside a NaN", skip=(2, 5, nan_row, all_nan_row))
    canaries = big.cpu().numpy()
    assert same_bits(canaries[:GUARD + 1], np.full(GUARD + 1, CANARY, canaries.dtype)) and same_bits(canaries[GUARD + 1 + M.data.size:],
                                                                                                   np.full(GUARD + 3, CANARY, canaries.dtype))


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_call(monkeypatch):
    class Refuses:
        def __getattr__(self, name):
            raise AssertionError("the library was called (%s)" % name)

    eng = MultiplyEngine()
    monkeypatch.setattr(eng, "L", Refuses())
    M = full_matrix("float64")

    def refused(error, f, dM, **kw):
        before, stamp = dM.data.clone(), dM.index_stamp()
        with pytest.raises(error):
            f(dM, engine=eng, **kw)
        assert dM.index_stamp() == stamp and (dM.data.dtype == torch.int32 or same_bits(dM.data.cpu().numpy(), before.cpu().numpy()))

    for sym in ("A", "K"):
        dM = to_dev(M)
        dM.symmetry = sym
        refused(ValueError, dbcsr_invert_block_diag, dM)
        refused(ValueError, dbcsr_invert_block_diag, dM, check=False)
    dM = to_dev(M)
    dM.symmetry = "X"
    refused(ValueError, dbcsr_invert_block_diag, dM)
    refused(ValueError, dbcsr_get_block_diag, dM)
    rect = to_dev(typed(base("mixed"), np.float64, 1))   # 230 x 260, different row and column block sizes
    assert rect.nblkrows != rect.nblkcols
    refused(ValueError, dbcsr_invert_block_diag, rect)
    refused(ValueError, dbcsr_get_block_diag, rect)
    dM = to_dev(M)
    other = dM.row_blk_size.clone()
    other[[0, 1]] = other[[1, 0]]   # as many block columns, other sizes
    uneven = DbcsrMatrix(dM.row_blk_size, other, dM.row_p, dM.col_i, dM.blk_p, dM.data)
    refused(ValueError, dbcsr_invert_block_diag, uneven)
    refused(ValueError, dbcsr_get_block_diag, uneven)
    ints = DbcsrMatrix(dM.row_blk_size, dM.col_blk_size, dM.row_p, dM.col_i, dM.blk_p, torch.zeros(dM.data.numel(), dtype=torch.int32, device="cuda"))
    refused(TypeError, dbcsr_invert_block_diag, ints)
    refused(TypeError, dbcsr_get_block_diag, ints)
    sizes = np.asarray([5, 97], np.int32)
    big = to_dev(from_blocks(sizes, sizes, {(0, 0): np.eye(5).reshape(-1), (1, 1): np.eye(97).reshape(-1)}, np.float64))
    refused(NotImplementedError, dbcsr_invert_block_diag, big)
    refused(NotImplementedError, dbcsr_invert_block_diag, big, check=False)


# ---- 7. C-ABI answers ---------------------------------------------------------------------------------------------------------------------------------------
def c_invert(eng, dM, max_dim, info=True, code=None, handle=None, null_matrix=False):
    d = dM.desc()
    out = (C.c_int64 * 3)(7, 7, 7) if info else None
    rc = eng.L.dbcsr_amd_bcsr_block_diag_invert(eng.h if handle is None else handle, dM.dtype_code if code is None else code,
                                                None if null_matrix else C.byref(d), max_dim, out, StreamHandle().ptr)
    torch.cuda.synchronize()
    return rc, (list(out) if info else None)


def test_c_abi_answers(eng):
    M = diagonal_matrix((5, 13, 23, 32, 33, 40), np.float64)
    dM = to_dev(M)
    kept = lambda: same_bits(dev_to_bcsr(dM).data, M.data)
    assert c_invert(eng, dM, 96, handle=C.c_void_p())[0] == -1 and c_invert(eng, dM, 96, null_matrix=True)[0] == -1
    assert c_invert(eng, dM, -1)[0] == -1
    assert c_invert(eng, dM, 96, code=99)[0] == -10
    assert c_invert(eng, dM, 97)[0] == -11 and c_invert(eng, dM, 1 << 20)[0] == -11
    rect = to_dev(typed(base("mixed"), np.float64, 1))
    assert c_invert(eng, rect, 32)[0] == -1
    assert kept(), "a refused call writes nothing"
    empty = to_dev(subset(M, lambda r, c: False))
    assert c_invert(eng, empty, 96) == (0, [0, -1, 0]) and c_invert(eng, empty, 96, info=False) == (0, None)
    # a bound below some dimensions: those blocks are skipped and counted, the smaller ones inverted
    assert c_invert(eng, dM, 23) == (0, [0, -1, 3])
    H = dev_to_bcsr(dM)
    for r in (3, 4, 5):
        assert same_bits(blocks_of(H)[(r, r)], blocks_of(M)[(r, r)])
    check_inverses(M, H, "max_dim 23", skip=(3, 4, 5))
    # the bound of the wave kernel alone, and no info
    dM = to_dev(M)
    assert c_invert(eng, dM, 32, info=False) == (0, None)
    H = dev_to_bcsr(dM)
    assert all(same_bits(blocks_of(H)[(r, r)], blocks_of(M)[(r, r)]) for r in (4, 5))
    check_inverses(M, H, "max_dim 32", skip=(4, 5))
    # the count and the copy
    d = dM.desc()
    n = dM.nblkrows
    row_p, col_i, blk_p = (torch.full((n + 1,), -7, dtype=torch.int32, device="cuda"), torch.full((n,), -7, dtype=torch.int32, device="cuda"),
                           torch.full((n,), -7, dtype=torch.int64, device="cuda"))
    nb, nz, md = C.c_int64(-1), C.c_int64(-1), C.c_int32(-1)
    count = lambda h, m, rp: eng.L.dbcsr_amd_bcsr_block_diag_count(h, m, rp, col_i.data_ptr(), blk_p.data_ptr(), C.byref(nb), C.byref(nz), C.byref(md),
                                                                   StreamHandle().ptr)
    assert count(C.c_void_p(), C.byref(d), row_p.data_ptr()) == -1 and count(eng.h, None, row_p.data_ptr()) == -1 and count(eng.h, C.byref(d), None) == -1
    r = rect.desc()
    assert count(eng.h, C.byref(r), row_p.data_ptr()) == -1
    assert count(eng.h, C.byref(d), row_p.data_ptr()) == 0
    assert (nb.value, nz.value, md.value) == (6, int(M.data.size), 40)
    assert row_p.cpu().tolist() == list(range(7)) and col_i.cpu().tolist() == list(range(6)) and np.array_equal(blk_p.cpu().numpy(), M.blk_p)
    dst = DbcsrMatrix(dM.row_blk_size, dM.col_blk_size, row_p, col_i, blk_p, torch.zeros(nz.value, dtype=torch.float64, device="cuda"))
    dd = dst.desc(out=True)
    apply = lambda h, code, s, t: eng.L.dbcsr_amd_bcsr_block_diag_apply(h, code, s, t, StreamHandle().ptr)
    assert apply(C.c_void_p(), dM.dtype_code, C.byref(d), C.byref(dd)) == -1 and apply(eng.h, dM.dtype_code, None, C.byref(dd)) == -1
    assert apply(eng.h, 99, C.byref(d), C.byref(dd)) == -10 and apply(eng.h, dM.dtype_code, C.byref(d), C.byref(d)) == -1
    assert apply(eng.h, dM.dtype_code, C.byref(d), C.byref(dd)) == 0
    torch.cuda.synchronize()
    assert same_bits(dst.data.cpu().numpy(), dM.data.cpu().numpy())


# ---- 8. far offsets -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def arena():
    a = FA.arena()
    yield a
    if a is not None:
        a.release()
        del a
    torch.cuda.empty_cache()


def test_diagonal_blocks_at_far_offsets(eng, arena):
    """the diagonal blocks of a small matrix around 2^29, 2^31, 2^32, ... elements of one large allocation (tests/far_arena.py)"""
    from tests.test_gpu_far_offsets import one_far
    M = diagonal_matrix((5, 13, 23, 32, 33, 40, 17, 16, 3, 2, 31, 64), np.float64)
    far, dM = one_far(arena, M, np.float64, "blocks")
    blk_p = dM.blk_p.cpu().numpy()
    assert np.any((blk_p >= 2 ** 31) & (blk_p < 2 ** 32)) and np.any(blk_p >= 2 ** 32)
    D = dbcsr_get_block_diag(dM, engine=eng)
    assert dbcsr_invert_block_diag(dM, engine=eng) == (0, -1)
    torch.cuda.synchronize()
    assert same_bits(dev_to_bcsr(D).data, M.data)
    check_inverses(M, FA.blocks_to_host(dM), "far offsets")
    assert far.guards_kept()


# ---- 9. what it is for ----------------------------------------------------------------------------------------------------------------------------------------
OVERLAP_SIZES = (5, 13, 16, 17, 23, 13)


def overlap_matrix():
    """S: diagonal blocks of the family spd (eigenvalues >= 1/2), every block off the diagonal uniform in [-0.008, 0.008]: ||I - S blockdiag(S)^-1|| < 1"""
    sizes = np.asarray(OVERLAP_SIZES, np.int32)
    rng = np.random.default_rng(9)
    blocks = {}
    for r in range(len(sizes)):
        for c in range(len(sizes)):
            blocks[(r, c)] = (column_major(block("spd", int(sizes[r]), "float64")) if r == c
                              else 0.008 * rng.uniform(-1.0, 1.0, int(sizes[r]) * int(sizes[c])))
    return from_blocks(sizes, sizes, blocks, np.float64)


def hotelling(eng, dS, dX, steps):
    """(residuals ||I - S X||_F before every step and after the last, X) of X <- X (2 I - S X) on the device"""
    def residual(dX):
        dR = to_dev(subset(dev_to_bcsr(dS), lambda r, c: False))
        dbcsr_multiply("N", "N", -1.0, dS, dX, 0.0, dR, engine=eng)
        dbcsr_add_on_diag(dR, 1.0, engine=eng)      # I - S X
        return dR, dbcsr_frobenius_norm(dR, engine=eng)

    out = []
    for _ in range(steps):
        dR, res = residual(dX)
        out.append(res)
        dbcsr_add_on_diag(dR, 1.0, engine=eng)      # 2 I - S X
        dN = to_dev(subset(dev_to_bcsr(dS), lambda r, c: False))
        dbcsr_multiply("N", "N", 1.0, dX, dR, 0.0, dN, engine=eng)
        dX = dN
    out.append(residual(dX)[1])
    return out, dX


def test_hotelling_inverse_and_block_jacobi(eng):
    S = overlap_matrix()
    dS = to_dev(S)
    dX0 = dbcsr_get_block_diag(dS, engine=eng)
    assert dbcsr_invert_block_diag(dX0, engine=eng) == (0, -1)
    torch.cuda.synchronize()
    X0 = dev_to_bcsr(dX0)
    check_inverses(subset(S, lambda r, c: r == c), X0, "X0")
    res, dX = hotelling(eng, dS, dX0, 3)
    print("||I - S X||_F:", res)
    assert all(res[i + 1] < res[i] for i in range(3)) and res[0] < 1.0
    # the same run from blocks inverted on the host
    host = {k: column_major(np.linalg.inv(block_of_data(v, int(S.row_sizes[k[0]])))) for k, v in blocks_of(S).items() if k[0] == k[1]}
    res_h, dXh = hotelling(eng, dS, to_dev(from_blocks(S.row_sizes, S.col_sizes, host, np.float64)), 3)
    torch.cuda.synchronize()
    a, b = dense(dev_to_bcsr(dX)), dense(dev_to_bcsr(dXh))
    assert np.max(np.abs(a - b)) <= 1e-10 * np.max(np.abs(b))
    # the final residual norm: I - S X is formed from the product S X, whose elements are of size max |S X| ~ 1, so two runs of it agree to the multiply
    # tests' bar on THAT product, 1e-10 max |S X| per element (the norm of a difference is at most the largest difference times the root of the element
    # count, already inside the bar's slack over double rounding).  Relative to the residual itself nothing can agree to 1e-10: after three steps it is
    # below 1e-9, and 1e-10 of that is under the 2^-53 to which an element of I - S X is formed at all
    assert abs(res[-1] - res_h[-1]) <= 1e-10 * np.max(np.abs(dense(S) @ b))
    assert np.max(np.abs(dense(S) @ a - np.eye(a.shape[0]))) <= 2 * res[-1]
    # the preconditioner: Y = X0 R is the solve of every block, within the bar of the product plus the bar of the inverse carried through |R|
    n = int(S.row_sizes.sum())
    R = random_vectors(n, 5, np.float64, 33)
    dr = Dev(R)
    dy = Dev(np.zeros_like(R))
    dbcsr_multivec(dX0, dr.t, dy.t, 1.0, 0.0, "N", engine=eng)
    torch.cuda.synchronize()
    _, bar = reference_columns(dense_parts(X0, "N"), "N", 1.0, 0.0, R, None)
    ref = np.zeros(R.shape, np.longdouble)
    ro = np.concatenate([[0], np.cumsum(S.row_sizes)])
    for r, m in enumerate(S.row_sizes):
        A = block_of_data(blocks_of(S)[(r, r)], int(m))
        X, w = reference_of(A)
        ref[ro[r]:ro[r + 1]] = X @ R[ro[r]:ro[r + 1]].astype(np.longdouble)
        bar[ro[r]:ro[r + 1]] += bar_of(A, X, w) @ np.abs(R[ro[r]:ro[r + 1]])
        solve = np.linalg.solve(A, R[ro[r]:ro[r + 1]])
        assert np.max(np.abs(solve - ref[ro[r]:ro[r + 1]].astype(np.float64))) <= 1e-12 * np.max(np.abs(solve))
    within_columns(dy.host(), ref, bar, "block-Jacobi")


# ---- 10. on a side stream -------------------------------------------------------------------------------------------------------------------------------------
def test_on_a_stream_of_its_own(eng):
    M = full_matrix("float64")
    dM = to_dev(M)
    D0 = dbcsr_get_block_diag(dM, engine=eng)
    assert dbcsr_invert_block_diag(D0, engine=eng) == (0, -1)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        D1 = dbcsr_get_block_diag(dM, engine=eng, stream=side)
        assert dbcsr_invert_block_diag(D1, engine=eng, stream=side) == (0, -1)
        D2 = dbcsr_get_block_diag(dM, engine=eng, stream=side)
        assert dbcsr_invert_block_diag(D2, check=False, engine=eng, stream=side) is None
    side.synchronize()
    want = dev_to_bcsr(D0).data
    assert same_bits(dev_to_bcsr(D1).data, want) and same_bits(dev_to_bcsr(D2).data, want), "the same bits on a side stream as on the default stream"
    assert same_bits(dM.data.cpu().numpy(), M.data)
