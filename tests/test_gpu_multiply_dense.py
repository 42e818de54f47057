"""The block-sparse matrix times a dense matrix on the matrix cores, Y <- alpha op(A) X + beta Y (dbcsr_amd/operations.py: dbcsr_multiply_dense;
dbcsr_amd_bcsr_multiply_dense of include/dbcsr_amd_mm.h; kernels spmm_product / spmm_scale of dbcsr_amd/csrc/mm_spmm.h) for float64, float32 and
complex128, with X and Y row by row (layout 0) or column by column (layout 1).

Reference and bars are those of tests/test_gpu_matvec.py, applied per column exactly as tests/test_gpu_multivec.py::reference_columns does: numpy long
double on the dense (desymmetrized) scatter; |got - ref| <= (n_i + 6) u w_i for real data, (n_i + 12) u w_i for complex data, plus the reference's own
n_i eps_ld w_i, plus 2^-24 |ref| for float32.  The bars are derived there for ANY order of summation and for products exact in double, so they hold for
chains of MFMAs unchanged: no new tolerance.  Nothing is compared against the code's own output except the bits of a second call and, in the test of
column independence, the bits of the same column computed in other company.

Columns: 1 and 3 (a partial tile), 16 (one tile), 17 (a tile and one column), 64 (one full workgroup), 70 (a second workgroup with one partial wave and
three waves that only stage).  Each count in both layouts, each layout contiguous and as a window with ld three larger than needed that starts one
element into an allocation full of canaries (not 16-byte aligned for real data); every canary must keep its bits.
Matrices: those of tests/test_gpu_matrix_norms.py / test_gpu_matvec.py (every one a few hundred full rows; mixed block sizes that are no multiples of
4 or 16; tall70 / tall67 with block rows above 64: the chunk path).  The right-hand sides of one matrix, type and op are the leading columns of one
70-column pair (X, Y0), so one reference serves every count, layout and window."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import dbcsr_amd
from dbcsr_amd import lib as L
from dbcsr_amd import operations as OPS
from dbcsr_amd.matrix import StreamHandle
from dbcsr_amd.multiply import MultiplyEngine, _z, dbcsr_multiply
from dbcsr_amd.operations import dbcsr_multiply_dense
from tests.gpu_util import to_dev
from tests.test_gpu_matrix_norms import (DTYPES, IDS, TORCH, base, from_blocks, full_len, hole_positions, is_complex, same_bits, subset, typed, with_holes)
from tests.test_gpu_matvec import (TRIANGLE_IDS, TRIANGLES, Poisoned, dense_parts, host_matrix, lengths, op_of, scalars, scaled_in_own_precision)
from tests.test_gpu_multivec import random_vectors, reference_columns, within_columns

pytestmark = pytest.mark.gpu

NCOLS = [1, 3, 16, 17, 64, 70]
MATRICES = ["mixed", "tiny", "tall70", "tall67", "gappy"]
CANARY = -77.25
TILE, WAVES = 16, 4   # columns of Y per wave, waves per workgroup (mm_spmm.h)


@pytest.fixture(scope="module")
def eng():
    return MultiplyEngine()


def paths(ncol):
    """(workgroups per block row, waves with columns in the last one, columns of the last such wave): which path a count of columns reaches"""
    groups = -(-ncol // (TILE * WAVES))
    last = ncol - (groups - 1) * TILE * WAVES
    waves = -(-last // TILE)
    return groups, waves, last - (waves - 1) * TILE


@functools.lru_cache(maxsize=None)
def inputs(which, dtype_name, symmetry, trans):
    """(X, Y0, ref, bar) for 70 columns with general scalars: formed once per matrix, type and op; the leading columns serve the smaller counts"""
    M, *parts = host_matrix(which, dtype_name, symmetry)
    dtype = M.data.dtype
    n_x, n_y = lengths(M, trans)
    alpha, beta = scalars(dtype)
    x, y0 = random_vectors(n_x, max(NCOLS), dtype, 61), random_vectors(n_y, max(NCOLS), dtype, 62)
    ref, bar = reference_columns(tuple(parts), trans, alpha, beta, x, y0)
    for a in (x, y0, ref, bar):
        a.setflags(write=False)
    return x, y0, ref, bar


class Dense:
    """a host (n, ncol) matrix on the device, row by row (layout 0) or column by column (layout 1): contiguous, or (window) with ld three larger than
    needed, one element into an allocation full of canaries"""

    def __init__(self, a, layout, window=False):
        n, ncol = a.shape
        runs, length = (n, ncol) if layout == 0 else (ncol, n)   # `runs` pieces of `length` consecutive elements, ld apart
        self.ld, start = (length + 3, 1) if window else (length, 0)
        self.big = torch.full((start + runs * self.ld + (2 if window else 0),), CANARY, dtype=TORCH[a.dtype], device="cuda")
        w = self.big[start:start + runs * self.ld].view(runs, self.ld)[:, :length]
        self.t = w if layout == 0 else w.t()
        assert tuple(self.t.shape) == (n, ncol)
        self.t.copy_(torch.as_tensor(np.array(a)))   # (a copy: the shared inputs are read-only)
        own = np.zeros(self.big.numel(), bool)
        own[start:start + runs * self.ld].reshape(runs, self.ld)[:, :length] = True
        self.own = own
        assert self.t.data_ptr() == self.big.data_ptr() + start * self.big.element_size()
        assert not window or is_complex(a.dtype) or self.t.data_ptr() % 16 != 0
        if n > 1 and ncol > 1:
            assert self.t.stride() == ((self.ld, 1) if layout == 0 else (1, self.ld))

    def host(self):
        return self.t.cpu().numpy()

    def canaries_kept(self):
        b = self.big.cpu().numpy()
        return same_bits(b[~self.own], np.full(int((~self.own).sum()), CANARY, b.dtype))


def run(eng, dM, dx, dy, alpha, beta, trans, layout):
    """the product into dy.t in the layout asked for.  A tensor of ONE column fits both layouts and dbcsr_multiply_dense then takes row by row, so one
    column in layout 1 goes through the C entry, which is told the layout: the column-by-column kernel at one column."""
    if layout == 1 and dx.t.shape[1] == 1:
        kind = -1 if dM.symmetry == "N" else L.SYMMETRY_KIND[dM.symmetry]
        assert c_entry(eng, dM, trans, alpha, beta, kind, 1, dx.t, dx.t.shape[0], dx.ld, dy.t, dy.t.shape[0], dy.ld, 1) == 0
        return dy.t
    return dbcsr_multiply_dense(dM, dx.t, dy.t, alpha, beta, trans, engine=eng)


def check_product(eng, dM, which, symmetry, trans, ncol, layout, window):
    """one product with general scalars against the reference; the same bits from a second call; X unchanged; nothing written outside Y's window"""
    dtype = TORCH_TO_NUMPY[dM.dtype]
    dM.symmetry = symmetry
    alpha, beta = scalars(dtype)
    x, y0, ref, bar = (a[:, :ncol] for a in inputs(which, np.dtype(dtype).name, symmetry, trans))
    dx, dy = Dense(x, layout, window), Dense(y0, layout, window)
    out = run(eng, dM, dx, dy, alpha, beta, trans, layout)
    torch.cuda.synchronize()
    assert out is dy.t and same_bits(dx.host(), np.ascontiguousarray(x)) and dx.canaries_kept() and dy.canaries_kept()
    got = dy.host()
    within_columns(got, ref, bar, "%s %s, symmetry %s, %d columns, layout %d%s" % (which, trans, symmetry, ncol, layout, ", a window" if window else ""))
    dy2 = Dense(y0, layout, window)
    run(eng, dM, dx, dy2, alpha, beta, trans, layout)
    torch.cuda.synchronize()
    assert same_bits(dy2.host(), got), "the same bits on every call"
    return got


TORCH_TO_NUMPY = {v: k for k, v in TORCH.items()}


def c_entry(eng, dM, trans, alpha, beta, kind, ncol, x, n_x, ldx, y, n_y, ldy, layout, code=None):
    d = dM.desc()
    return eng.L.dbcsr_amd_bcsr_multiply_dense(eng.h, dM.dtype_code if code is None else code, trans.encode(), _z(alpha), C.byref(d), kind, ncol,
                                               x.data_ptr() if x is not None else None, n_x, ldx, _z(beta), y.data_ptr() if y is not None else None, n_y,
                                               ldy, layout, StreamHandle().ptr)


# ---- 1. every matrix, type, op, count of columns, layout and window ----------------------------------------------------------------------------------
@pytest.mark.parametrize("trans", ["N", "T", "C"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("which", MATRICES)
def test_multiply_dense(eng, which, dtype, trans):
    M = host_matrix(which, np.dtype(dtype).name, "N")[0]
    dM = to_dev(M)
    for ncol in NCOLS:
        for layout in (0, 1):
            for window in (False, True):
                check_product(eng, dM, which, "N", trans, ncol, layout, window)


# ---- 2. stored triangles -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trans", ["N", "T", "C"])
@pytest.mark.parametrize("dtype,symmetry", TRIANGLES, ids=TRIANGLE_IDS)
def test_multiply_dense_of_a_stored_triangle(eng, dtype, symmetry, trans):
    """the product is that of the desymmetrized matrix (formed in numpy): both passes of the walk into the same registers"""
    M = host_matrix("symmetric", np.dtype(dtype).name, symmetry)[0]
    dM = to_dev(M)
    for ncol in (3, 70):
        for layout in (0, 1):
            check_product(eng, dM, "symmetric", symmetry, trans, ncol, layout, window=ncol == 70)


# ---- 3. holes and empty block rows ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_multiply_dense_of_an_operand_with_holes(eng, dtype):
    hB, dB = with_holes(eng, typed(base("mixed"), dtype, 1), dtype)
    holes = hole_positions(hB)
    assert holes.size > 0
    dB.data[torch.as_tensor(holes[:: max(1, holes.size // 7)], device="cuda")] = 1e30   # a hole is not the matrix': it must not count
    torch.cuda.synchronize()
    parts = dense_parts(hB, "N")
    alpha, beta = scalars(dtype)
    for trans in ("N", "T", "C"):
        n_x, n_y = lengths(hB, trans)
        x, y0 = random_vectors(n_x, 17, dtype, 63), random_vectors(n_y, 17, dtype, 64)
        ref, bar = reference_columns(parts, trans, alpha, beta, x, y0)
        for layout in (0, 1):
            dy = Dense(y0, layout, True)
            dbcsr_multiply_dense(dB, Dense(x, layout, True).t, dy.t, alpha, beta, trans, engine=eng)
            torch.cuda.synchronize()
            within_columns(dy.host(), ref, bar, "holes, %s, layout %d" % (trans, layout))
            assert dy.canaries_kept()


def empty_rows(M, trans):
    """the full rows of op(A) whose block row stores nothing"""
    mask = host_pattern(M)
    return np.flatnonzero(~op_of(mask, "T" if trans != "N" else "N").any(axis=1))


def host_pattern(M):
    return dense_parts(M, "N")[2]


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_rows_of_an_empty_block_row(eng, dtype, layout):
    """gappy has block rows and block columns that store nothing: their rows of Y become beta Y0, and +0.0 for beta == 0 even from a Y full of NaN.
    beta Y0 is formed in double with one rounding to the data's type, checked bit for bit: for float64 and complex128 that is the product in the data's
    own precision (complex: every operation rounded on its own), for float32 one double product rounded once.  (The product in float32's own precision
    rounds twice, the scalar and the product: on this matrix it missed the bar of case 1 -- 9.5e-08 against 6.4e-08 -- and the bar is the one that
    stays.)"""
    M = host_matrix("gappy", np.dtype(dtype).name, "N")[0]
    dM = to_dev(M)
    alpha, beta = scalars(dtype)
    for trans in ("N", "T"):
        rows = empty_rows(M, trans)
        assert rows.size >= 3
        x, y0, ref, bar = (a[:, :17] for a in inputs("gappy", np.dtype(dtype).name, "N", trans))
        dy = Dense(y0, layout, True)
        dbcsr_multiply_dense(dM, Dense(x, layout).t, dy.t, alpha, beta, trans, engine=eng)
        torch.cuda.synchronize()
        got = dy.host()[rows]
        within_columns(got, ref[rows], bar[rows], "empty block rows, %s" % trans)
        if is_complex(dtype):
            assert same_bits(got, scaled_in_own_precision(beta, np.ascontiguousarray(y0[rows]))), "beta y in complex double, every operation rounded"
        else:
            assert same_bits(got, (np.float64(beta) * y0[rows].astype(np.float64)).astype(dtype)), "beta y, one rounding"
        nan = Dense(np.full(y0.shape, np.nan, dtype), layout, True)
        dbcsr_multiply_dense(dM, Dense(x, layout).t, nan.t, alpha, 0.0, trans, engine=eng)
        torch.cuda.synchronize()
        got = nan.host()
        assert not np.any(np.isnan(got)) and nan.canaries_kept()
        assert same_bits(got[rows], np.zeros((rows.size, 17), dtype)), "+0.0, bit for bit"


# ---- 4. a column's bits depend neither on its position nor on its company ------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("which,dtype,symmetry,trans", [("mixed", np.float64, "N", "N"), ("mixed", np.float64, "N", "T"), ("tall70", np.complex128, "N", "N"),
                                                        ("mixed", np.complex128, "N", "T"), ("symmetric", np.float64, "S", "N")],
                         ids=["fp64_N", "fp64_T", "z64_N", "z64_T", "fp64_S"])
def test_column_independence(eng, which, dtype, symmetry, trans, layout):
    M = host_matrix(which, np.dtype(dtype).name, symmetry)[0]
    dM = to_dev(M)
    dM.symmetry = symmetry
    alpha, beta = scalars(dtype)
    x, y0, _, _ = inputs(which, np.dtype(dtype).name, symmetry, trans)
    full = dbcsr_multiply_dense(dM, Dense(x, layout).t, Dense(y0, layout).t, alpha, beta, trans, engine=eng).cpu().numpy()
    for v in (0, 15, 16, 37, 63, 64, 69):
        xv, yv = np.ascontiguousarray(x[:, v:v + 1]), np.ascontiguousarray(y0[:, v:v + 1])
        alone = run(eng, dM, Dense(xv, layout), Dense(yv, layout), alpha, beta, trans, layout).cpu().numpy()   # (the same layout's kernel)
        assert same_bits(alone[:, 0], full[:, v]), "column %d alone" % v
        x3 = np.ascontiguousarray(np.concatenate([xv, x[:, :2]], axis=1))
        y3 = np.ascontiguousarray(np.concatenate([yv, y0[:, :2]], axis=1))
        three = dbcsr_multiply_dense(dM, Dense(x3, layout, True).t, Dense(y3, layout, True).t, alpha, beta, trans, engine=eng).cpu().numpy()
        assert same_bits(three[:, 0], full[:, v]), "column %d as column 0 of three" % v


# ---- 5. special values ---------------------------------------------------------------------------------------------------------------------------------
def special_row(M, trans):
    """(r, rows of Y that must see it): r is the first row of X directly behind a block (of the summed dimension) whose size is no multiple of 4, such
    that some rows of op(A) store an element in column r and some do not"""
    sizes = M.col_sizes if trans == "N" else M.row_sizes
    offs = np.concatenate([[0], np.cumsum(sizes)])
    col_has = op_of(host_pattern(M), "T" if trans != "N" else "N")
    for J in range(len(sizes) - 1):
        r = int(offs[J + 1])
        if sizes[J] % 4 != 0 and col_has[:, r].any() and not col_has[:, r].all():
            return r, int(sizes[J]), col_has[:, r]
    raise AssertionError("no such row")


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("trans", ["N", "T"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_nan_or_inf_in_one_row_of_x_reaches_only_the_rows_that_store_its_column(eng, dtype, trans, layout):
    M, *parts = host_matrix("mixed", np.dtype(dtype).name, "N")
    dM = to_dev(M)
    alpha, beta = scalars(dtype)
    r, size, hit = special_row(M, trans)
    assert size % 4 != 0 and hit.any() and not hit.all()
    x, y0, _, _ = (a[:, :17] for a in inputs("mixed", np.dtype(dtype).name, "N", trans))
    xz = np.array(x)
    xz[r] = 0
    ref, bar = reference_columns(tuple(parts), trans, alpha, beta, xz, np.ascontiguousarray(y0))   # (the rows that miss column r do not see row r)
    for bad in (np.nan, np.inf):
        xb = np.array(x)
        xb[r] = bad
        dy = Dense(y0, layout, True)
        dbcsr_multiply_dense(dM, Dense(xb, layout, True).t, dy.t, alpha, beta, trans, engine=eng)
        torch.cuda.synchronize()
        got = dy.host()
        assert np.all(~np.isfinite(got[hit])), "every row that stores column %d sees %r" % (r, bad)
        assert np.all(np.isfinite(got[~hit]))
        within_columns(got[~hit], ref[~hit], bar[~hit], "the rows that miss column %d, %r" % (r, bad))
        assert dy.canaries_kept()


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_zero_scalars(eng, dtype, layout):
    M, *parts = host_matrix("mixed", np.dtype(dtype).name, "N")
    dM = to_dev(M)
    alpha, beta = scalars(dtype)
    tdt = TORCH[np.dtype(dtype)]
    for trans in ("N", "C"):
        n_x, n_y = lengths(M, trans)
        x, y0, _, _ = (np.ascontiguousarray(a[:, :17]) for a in inputs("mixed", np.dtype(dtype).name, "N", trans))
        dx = Dense(x, layout)
        # beta == 0: Y is not read
        dy = Dense(np.full(y0.shape, np.nan, dtype), layout, True)
        dbcsr_multiply_dense(dM, dx.t, dy.t, alpha, 0.0, trans, engine=eng)
        torch.cuda.synchronize()
        got = dy.host()
        assert not np.any(np.isnan(got)) and dy.canaries_kept()
        ref, bar = reference_columns(tuple(parts), trans, alpha, 0.0, x, None)
        within_columns(got, ref, bar, "beta == 0, %s" % trans)
        # dense_out=None: the same product into a new tensor in X's layout
        new = dbcsr_multiply_dense(dM, dx.t, None, alpha, 0.0, trans, engine=eng)
        torch.cuda.synchronize()
        assert new.dtype == tdt and new.is_cuda and tuple(new.shape) == (n_y, 17) and new.stride() == ((17, 1) if layout == 0 else (1, n_y))
        assert same_bits(new.cpu().numpy(), got)
        # alpha == 0 with NaN in A and X: neither is read, Y <- beta Y in the data's precision
        dN = to_dev(typed(base("mixed"), dtype, 1))
        dN.data.fill_(float("nan"))
        dy = Dense(y0, layout, True)
        dbcsr_multiply_dense(dN, Dense(np.full(x.shape, np.nan, dtype), layout).t, dy.t, 0.0, beta, trans, engine=eng)
        torch.cuda.synchronize()
        assert same_bits(dy.host(), scaled_in_own_precision(beta, y0).astype(dtype)), "alpha == 0: beta Y, bit for bit"
        assert dy.canaries_kept()
        dbcsr_multiply_dense(dN, dx.t, dy.t, 0.0, 0.0, trans, engine=eng)
        torch.cuda.synchronize()
        assert not np.any(dy.host()) and dy.canaries_kept()


# ---- 6. the C entry ------------------------------------------------------------------------------------------------------------------------------------
def test_c_entry_refusals_write_nothing(eng):
    A, Sq = base("mixed"), base("square")
    dA, dS = to_dev(A), to_dev(Sq)
    n = full_len(Sq.row_sizes)
    k = 3
    big = torch.ones(2 * n * k, dtype=torch.float64, device="cuda")
    x, y = big[:n * k], big[n * k:]
    for code in (L.dbcsr_type_complex_4, 2, 99):
        assert c_entry(eng, dS, "N", 1.0, 0.0, -1, k, x, n, k, y, n, k, 0, code=code) == -10
    assert c_entry(eng, dS, "N", 1.0, 0.0, -1, k, None, n, k, y, n, k, 0) == -1
    assert c_entry(eng, dS, "N", 1.0, 0.0, -1, k, x, n, k, None, n, k, 0) == -1
    d = dS.desc()
    st = StreamHandle().ptr
    f64 = L.dbcsr_type_real_8
    call = eng.L.dbcsr_amd_bcsr_multiply_dense
    assert call(None, f64, b"N", _z(1.0), C.byref(d), -1, k, x.data_ptr(), n, k, _z(0.0), y.data_ptr(), n, k, 0, st) == -1
    assert call(eng.h, f64, b"N", None, C.byref(d), -1, k, x.data_ptr(), n, k, _z(0.0), y.data_ptr(), n, k, 0, st) == -1
    assert call(eng.h, f64, b"N", _z(1.0), None, -1, k, x.data_ptr(), n, k, _z(0.0), y.data_ptr(), n, k, 0, st) == -1
    assert call(eng.h, f64, b"N", _z(1.0), C.byref(d), -1, k, x.data_ptr(), n, k, None, y.data_ptr(), n, k, 0, st) == -1
    for kind in (4, -2):
        assert c_entry(eng, dS, "N", 1.0, 0.0, kind, k, x, n, k, y, n, k, 0) == -1
    for trans in ("X", "n"):
        assert c_entry(eng, dS, trans, 1.0, 0.0, -1, k, x, n, k, y, n, k, 0) == -1
    for layout in (-1, 2):
        assert c_entry(eng, dS, "N", 1.0, 0.0, -1, k, x, n, n, y, n, n, layout) == -1
    assert c_entry(eng, dS, "N", 1.0, 0.0, -1, -1, x, n, k, y, n, k, 0) == -1       # ncol < 0
    assert c_entry(eng, dS, "N", 1.0, 0.0, -1, k, x, -1, k, y, n, k, 0) == -1
    assert c_entry(eng, dS, "N", 1.0, 0.0, -1, k, x, n, k - 1, y, n, k, 0) == -1    # row by row: ld below ncol
    assert c_entry(eng, dS, "N", 1.0, 0.0, -1, k, x, n, k, y, n, k - 1, 0) == -1
    assert c_entry(eng, dS, "N", 1.0, 0.0, -1, k, x, n, n - 1, y, n, n, 1) == -1    # column by column: ld below n
    assert c_entry(eng, dS, "N", 1.0, 0.0, -1, k, x, n, n, y, n, n - 1, 1) == -1
    # element ranges that intersect, in either layout: the same, by one element from either side
    for layout, ld in ((0, k), (1, n)):
        assert c_entry(eng, dS, "N", 1.0, 0.0, -1, k, x, n, ld, x, n, ld, layout) == -1
        assert c_entry(eng, dS, "N", 1.0, 0.0, -1, k, x, n, ld, big[n * k - 1:], n, ld, layout) == -1
        assert c_entry(eng, dS, "N", 1.0, 0.0, -1, k, big[1:], n, ld, x, n, ld, layout) == -1
    # a stored triangle needs a square block structure
    xa = torch.ones((full_len(A.col_sizes), k), dtype=torch.float64, device="cuda")
    ya = torch.ones((full_len(A.row_sizes), k), dtype=torch.float64, device="cuda")
    assert c_entry(eng, dA, "N", 1.0, 0.0, 0, k, xa, xa.shape[0], k, ya, ya.shape[0], k, 0) == -1
    # a grid above INT32_MAX, reached by ranges that cannot intersect: 100000 block rows of one element times 21475 workgroups of 64 columns.  X and Y
    # are one row each (n_x = n_y = 1) in allocations of their own, so nothing but the grid refuses the call; and the answer comes before any launch
    many = 100000
    wide = 64 * (2 ** 31 // many + 1)
    ones = np.ones(many, np.int32)
    dL = to_dev(from_blocks(ones, ones, {(0, 0): np.ones(1)}, np.float64))
    assert dL.nblkrows * (wide // 64) > 2 ** 31 - 1
    xw, yw = torch.ones(wide, dtype=torch.float64, device="cuda"), torch.ones(wide, dtype=torch.float64, device="cuda")
    for layout, ld in ((0, wide), (1, 1)):
        assert c_entry(eng, dL, "N", 1.0, 0.0, -1, wide, xw, 1, ld, yw, 1, ld, layout) == -1
    torch.cuda.synchronize()
    assert not np.any(xw.cpu().numpy() != 1.0) and not np.any(yw.cpu().numpy() != 1.0)
    assert c_entry(eng, dL, "N", 2.0, 0.0, -1, 64, xw, 1, 64, yw, 1, 64, 0) == 0   # (the same call at one workgroup per block row is served)
    torch.cuda.synchronize()
    assert not np.any(xw.cpu().numpy() != 1.0) and not np.any(yw.cpu().numpy()[:64] != 2.0) and not np.any(yw.cpu().numpy()[64:] != 1.0)
    torch.cuda.synchronize()
    assert not np.any(big.cpu().numpy() != 1.0) and not np.any(ya.cpu().numpy() != 1.0)


def test_c_entry_answers_zero_and_multiplies(eng):
    Sq = base("square")
    dS = to_dev(Sq)
    n = full_len(Sq.row_sizes)
    k = 3
    big = torch.ones(2 * n * k, dtype=torch.float64, device="cuda")
    x, y = big[:n * k], big[n * k:]
    for layout, ld in ((0, k), (1, n)):
        assert c_entry(eng, dS, "N", 1.0, 0.5, -1, 0, x, n, ld if layout else 0, y, n, ld if layout else 0, layout) == 0   # ncol == 0
        assert c_entry(eng, dS, "N", 1.0, 0.5, -1, k, x, n, ld, y, 0, k if layout == 0 else 0, layout) == 0                 # n_y == 0
    torch.cuda.synchronize()
    assert not np.any(big.cpu().numpy() != 1.0)
    # an empty matrix: 0, Y <- beta Y
    dE = to_dev(subset(Sq, lambda r, c: False))
    for layout, ld in ((0, k), (1, n)):
        ye = torch.full((n * k,), 3.0, dtype=torch.float64, device="cuda")
        assert c_entry(eng, dE, "N", 1.0, 0.5, -1, k, x, n, ld, ye, n, ld, layout) == 0
        torch.cuda.synchronize()
        assert not np.any(ye.cpu().numpy() != 1.5)
    # one product per layout, on ranges that touch
    M, *parts = host_matrix("mixed", "float64", "N")
    dM = to_dev(M)
    n_x, n_y = lengths(M, "N")
    alpha, beta = scalars(np.float64)
    xh, y0, ref, bar = (a[:, :17] for a in inputs("mixed", "float64", "N", "N"))
    for layout in (0, 1):
        dx, dy = Dense(xh, layout, True), Dense(y0, layout, True)
        assert c_entry(eng, dM, "N", alpha, beta, -1, 17, dx.t, n_x, dx.ld, dy.t, n_y, dy.ld, layout) == 0
        torch.cuda.synchronize()
        within_columns(dy.host(), ref, bar, "the C entry, layout %d" % layout)
        assert dx.canaries_kept() and dy.canaries_kept()


# ---- 7. refusals of the Python function ------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_call(monkeypatch):
    bad = Poisoned()
    monkeypatch.setattr(OPS, "default_engine", lambda: bad)   # (and no engine of its own is made either)
    A = base("mixed")
    dA = to_dev(A)
    rows, cols = full_len(A.row_sizes), full_len(A.col_sizes)
    x = torch.ones((cols, 3), dtype=torch.float64, device="cuda")
    y = torch.ones((rows, 3), dtype=torch.float64, device="cuda")
    xc = torch.ones((3, cols), dtype=torch.float64, device="cuda").t()
    yc = torch.ones((3, rows), dtype=torch.float64, device="cuda").t()
    with pytest.raises(ValueError):
        dbcsr_multiply_dense(dA, x, yc, engine=bad)   # mixed layouts
    with pytest.raises(ValueError):
        dbcsr_multiply_dense(dA, xc, y, engine=bad)
    with pytest.raises(ValueError):
        dbcsr_multiply_dense(dA, y, x, engine=bad)   # the rows' length for the columns
    with pytest.raises(ValueError):
        dbcsr_multiply_dense(dA, x, y[:-1].contiguous(), engine=bad)
    with pytest.raises(ValueError):
        dbcsr_multiply_dense(dA, x, y, trans="T", engine=bad)   # op(A) has the other shape
    with pytest.raises(ValueError):
        dbcsr_multiply_dense(dA, x, y[:, :2].contiguous(), engine=bad)   # another count of columns
    with pytest.raises(ValueError):
        dbcsr_multiply_dense(dA, x[:, 0], y[:, 0], engine=bad)   # 1-D
    with pytest.raises(TypeError):
        dbcsr_multiply_dense(dA, x.float(), y, engine=bad)
    with pytest.raises(TypeError):
        dbcsr_multiply_dense(dA, x, y.to(torch.complex128), engine=bad)
    with pytest.raises(TypeError):
        dbcsr_multiply_dense(dA, np.ones((cols, 3)), y, engine=bad)
    with pytest.raises(ValueError):
        dbcsr_multiply_dense(dA, x.cpu(), y, engine=bad)   # wrong device type
    with pytest.raises(ValueError):
        dbcsr_multiply_dense(dA, x, y.cpu(), engine=bad)
    with pytest.raises(ValueError):
        dbcsr_multiply_dense(dA, torch.ones((cols, 6), dtype=torch.float64, device="cuda")[:, ::2], y, engine=bad)   # neither layout
    with pytest.raises(ValueError):
        dbcsr_multiply_dense(dA, torch.ones(3 * cols, dtype=torch.float64, device="cuda").as_strided((cols, 3), (2, 1)), y, engine=bad)   # ld below ncol
    for trans in ("X", "n", "", None):
        with pytest.raises(ValueError):
            dbcsr_multiply_dense(dA, x, y, trans=trans, engine=bad)
    with pytest.raises(ValueError):
        dbcsr_multiply_dense(dA, x, beta=0.5, engine=bad)   # beta != 0 without dense_out
    with pytest.raises(ValueError):
        dbcsr_multiply_dense(dA, x, beta=0.5)   # (nor is the default engine asked for)
    with pytest.raises(TypeError):
        dbcsr_multiply_dense(dA, x, y, alpha=1j, engine=bad)
    # overlap, in either layout
    Sq = to_dev(base("square"))
    n = full_len(base("square").row_sizes)
    big = torch.ones(2 * n * 3 + 8, dtype=torch.float64, device="cuda")
    first, second = big[:3 * n].view(n, 3), big[3 * n:6 * n].view(n, 3)
    with pytest.raises(ValueError):
        dbcsr_multiply_dense(Sq, first, first, engine=bad)
    with pytest.raises(ValueError):
        dbcsr_multiply_dense(Sq, first, big[3 * n - 1:6 * n - 1].view(n, 3), engine=bad)
    with pytest.raises(ValueError):
        dbcsr_multiply_dense(Sq, big[:3 * n].view(3, n).t(), big[3 * n - 1:6 * n - 1].view(3, n).t(), engine=bad)
    basis = big[:6 * n].view(n, 6)
    with pytest.raises(ValueError):
        dbcsr_multiply_dense(Sq, basis[:, :3], basis[:, 3:], engine=bad)
    # symmetry
    Sq.symmetry = "X"
    with pytest.raises(ValueError):
        dbcsr_multiply_dense(Sq, first, second, engine=bad)
    Sq.symmetry = "H"   # real data: 'S' and 'A'
    with pytest.raises(ValueError):
        dbcsr_multiply_dense(Sq, first, second, engine=bad)
    Z = to_dev(typed(base("square"), np.complex128, 1))
    Z.symmetry = "S"    # complex data: 'H' and 'K'
    zx = torch.ones((n, 3), dtype=torch.complex128, device="cuda")
    with pytest.raises(NotImplementedError):
        dbcsr_multiply_dense(Z, zx, torch.ones_like(zx), engine=bad)
    tri = to_dev(subset(A, lambda r, c: r <= c))
    tri.symmetry = "S"
    with pytest.raises(ValueError):
        dbcsr_multiply_dense(tri, x, y, engine=bad)   # a matrix with symmetry that is not square
    torch.cuda.synchronize()
    assert not np.any(big.cpu().numpy() != 1.0) and not np.any(y.cpu().numpy() != 1.0)
    assert dbcsr_amd.dbcsr_multiply_dense is dbcsr_multiply_dense and "dbcsr_multiply_dense" in dbcsr_amd.__all__


# ---- 8. between multiplies -----------------------------------------------------------------------------------------------------------------------------
def test_multiply_dense_between_multiplies_keeps_the_plan(monkeypatch):
    from oracle import oracle as O
    monkeypatch.delenv("DBCSR_AMD_MM_PLAN", raising=False)
    eng = MultiplyEngine()
    sizes = O.make_block_sizes(200, [1, 13, 1, 5, 1, 7])
    A = typed(O.make_random_matrix(sizes, sizes, 0.5, O.RANDMAT_SEED_INIT + 31), np.float64, 5)
    B = typed(O.make_random_matrix(sizes, sizes, 0.6, O.RANDMAT_SEED_INIT + 32), np.float64, 6)
    dA, dB = to_dev(A), to_dev(B)
    dC = to_dev(subset(A, lambda r, c: False))
    dbcsr_multiply("N", "N", 1.0, dA, dB, 0.0, dC, engine=eng)
    assert eng.plan_stats() == (0, 1)
    xh = random_vectors(full_len(sizes), 70, np.float64, 65)
    tensors = [(m.row_p, m.col_i, m.blk_p, m.data) for m in (dA, dC)]
    stamps = (dA.index_stamp(), dC.index_stamp())
    for layout in (0, 1):
        x = Dense(xh, layout).t
        for trans in ("N", "T"):
            dbcsr_multiply_dense(dA, x, trans=trans, engine=eng)   # of its operand ...
            dbcsr_multiply_dense(dC, x, trans=trans, engine=eng)   # ... and of its result
        dA.symmetry = "S"
        dbcsr_multiply_dense(dA, x, engine=eng)   # (both passes: the per-column lists are built in the algebra's own buffers)
        dA.symmetry = "N"
    assert (dA.index_stamp(), dC.index_stamp()) == stamps
    assert all(a is b for m, t in zip((dA, dC), tensors) for a, b in zip((m.row_p, m.col_i, m.blk_p, m.data), t))
    dbcsr_multiply("N", "N", 1.0, dA, dB, 0.0, dC, engine=eng)
    assert eng.plan_stats() == (1, 1), "a multiply after the product with a dense matrix must reuse its plan"
