"""The block-sparse matrix-vector product on the device, y <- alpha op(A) x + beta y (dbcsr_amd/operations.py: dbcsr_matvec; dbcsr_amd_bcsr_matvec of
include/dbcsr_amd_mm.h; kernels algebra_matvec_rows / _cols / _combine of dbcsr_amd/csrc/mm_algebra.h) for float64, float32 and complex128.

Reference: numpy on the dense scatter of the matrix (for a stored triangle: of the desymmetrized matrix), transposed / conjugated for op, with products
and sums in numpy's long double (complex long double): where that is the 80-bit format its own error, n_i eps_ld w_i with eps_ld = 2^-63, is 2^-10 of
the bars below.  It is derived, not observed, and is added to them (n_i eps_ld w_i): the reference's own error.  On a platform whose long double is
float64 (eps_ld = 2^-52) that term is 2 n_i u w_i, which about triples the bar beyond the (n_i + 6) u w_i of the arithmetic under test -- such a
platform checks less sharply, never the code against its own output.  x and the old
y come from a seeded generator with both signs; alpha and beta are neither 0 nor 1, complex for complex data.

Bars, derived (u = 2^-53: products and sums are carried in double / complex double for every data type).  n_i = the stored elements of full row i of
op(A), desymmetrized; w_i = |alpha| sum_j |a_ij| |x_j| + |beta| |y_i|.
  real data     |got - ref| <= (n_i + 6) u w_i: one rounding per product (none for float32 data, whose products are exact in double; a product
                contracted into a fused multiply-add rounds less, not more), n_i - 1 for the sum of the n_i terms in ANY order -- a lane's
                accumulator, the hand-over through LDS, the partial vectors of both passes: all of it is one sum of the same terms --, three for
                alpha s + beta y, two for the second-order terms.
  complex data  (n_i + 12) u w_i in modulus: a complex product in double is within 3 u of |a| |x|, and there are three of them (the term, alpha s,
                beta y).
  float32       the one final rounding adds 2^-24 |ref|.
  alpha == 0    y == beta y formed in the data's own precision, bit for bit: real data one rounded product of the scalar converted to the data type;
                complex data (br yr - bi yi, br yi + bi yr) with every operation rounded on its own (written out on the real parts here: numpy's
                own complex product may use fused operations).  The same for an empty matrix.
  power steps   the project's 1e-10 by maximum element against the same iteration in numpy (the vectors have unit norm).
Matrices: those of tests/test_gpu_matrix_norms.py, the smallest that reach every branch -- "mixed" (230 x 260, fewer than 64 lanes busy, odd element
counts, blocks that start at odd elements), "tiny" (sizes 1 and 3, more than 64 blocks per row), "tall70" / "tall67" (the slot form with a period of
35 and the form for tall blocks; more than 64 columns: two column passes; more than one staged piece), "gappy" (empty block rows and columns, missing
diagonal blocks), the stored triangles, an operand with holes, a data area that is not 16-byte aligned, an empty matrix."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import dbcsr_amd
from dbcsr_amd import lib as L
from dbcsr_amd.matrix import StreamHandle
from dbcsr_amd.multiply import MultiplyEngine, _z, dbcsr_multiply
from dbcsr_amd.operations import dbcsr_gershgorin_norm, dbcsr_matvec
from tests.gpu_util import dev_to_bcsr, to_dev
from tests.test_gpu_matrix_norms import (DTYPES, IDS, TORCH, U53, base, blocks_of, dense, desymmetrized_dense, full_len, hole_positions, is_complex,
                                         misaligned, pattern_mask, product_bar, random_vector, same_bits, subset, symmetric_base, typed, with_holes)

pytestmark = pytest.mark.gpu

EPS_LD = float(np.finfo(np.longdouble).eps)
TRIANGLES = [(np.float64, "S"), (np.float32, "S"), (np.float64, "A"), (np.float32, "A"), (np.complex128, "H"), (np.complex128, "K")]
TRIANGLE_IDS = ["fp64_S", "fp32_S", "fp64_A", "fp32_A", "z64_H", "z64_K"]


@pytest.fixture(scope="module")
def eng():
    return MultiplyEngine()


def scalars(dtype):
    return (0.7 - 0.4j, -0.3 + 0.9j) if is_complex(dtype) else (-1.3, 0.6)


def wide(dtype):
    return np.clongdouble if is_complex(dtype) else np.longdouble


@functools.lru_cache(maxsize=None)
def host_matrix(which, dtype_name, symmetry):
    """(the host matrix, its dense / desymmetrized dense scatter in long double, |that| in float64, the pattern of stored elements): formed once"""
    dtype = np.dtype(dtype_name)
    M = typed(base(which) if symmetry == "N" else symmetric_base(symmetry), dtype, 1 if symmetry == "N" else 3)
    return (M,) + dense_parts(M, symmetry)


def dense_parts(M, symmetry):
    F = dense(M) if symmetry == "N" else desymmetrized_dense(M, symmetry)
    return F.astype(wide(M.data.dtype)), np.abs(F).astype(np.float64), pattern_mask(M, symmetry)


def op_of(F, trans):
    return F if trans == "N" else (F.T if trans == "T" else F.conj().T)


def reference(parts, trans, alpha, beta, x, y0):
    """(ref in long double, bar per element) of alpha op(F) x + beta y0"""
    F, absF, mask = parts
    dtype = x.dtype
    ref = alpha * (op_of(F, trans) @ x.astype(F.dtype)) + (beta * y0.astype(F.dtype) if y0 is not None else 0)
    w = abs(alpha) * (op_of(absF, "T" if trans != "N" else "N") @ np.abs(x).astype(np.float64)) + (abs(beta) * np.abs(y0) if y0 is not None else 0.0)
    n = op_of(mask, "T" if trans != "N" else "N").sum(axis=1)
    bar = (n + (12 if is_complex(dtype) else 6)) * U53 * w + n * EPS_LD * w
    if dtype == np.float32:
        bar = bar + 2.0 ** -24 * np.abs(ref).astype(np.float64)
    return ref, bar


def within(got, ref, bar, what):
    assert got.shape == ref.shape
    err = np.abs(got.astype(ref.dtype) - ref).astype(np.float64)
    worst = int(np.argmax(err - bar)) if err.size else 0
    print("%s: worst element %d: error %.3e against a bar of %.3e" % (what, worst, float(err[worst]) if err.size else 0.0, float(bar[worst]) if err.size else 0.0))
    assert np.all(err <= bar), what


def on_device(v, view=False):
    """the host vector on the device; view: one element into a larger tensor (not 16-byte aligned for float64 and float32)"""
    if not view:
        return torch.as_tensor(v.copy()).cuda()
    big = torch.zeros(v.size + 3, dtype=TORCH[v.dtype], device="cuda")
    big[1:1 + v.size].copy_(torch.as_tensor(v))
    return big[1:1 + v.size]


def lengths(M, trans):
    rows, cols = full_len(M.row_sizes), full_len(M.col_sizes)
    return (cols, rows) if trans == "N" else (rows, cols)


def check_product(eng, M, dM, parts, symmetry, trans, view=False):
    """one product with general scalars against the reference, and the same bits from a second call"""
    dtype = M.data.dtype
    dM.symmetry = symmetry
    n_x, n_y = lengths(M, trans)
    alpha, beta = scalars(dtype)
    x, y0 = random_vector(n_x, dtype, 21), random_vector(n_y, dtype, 22)
    dx, dy = on_device(x, view), on_device(y0, view)
    out = dbcsr_matvec(dM, dx, dy, alpha, beta, trans, engine=eng)
    torch.cuda.synchronize()
    assert out is dy and same_bits(dx.cpu().numpy(), x)
    got = dy.cpu().numpy()
    ref, bar = reference(parts, trans, alpha, beta, x, y0)
    within(got, ref, bar, "matvec %s, symmetry %s" % (trans, symmetry))
    dy2 = on_device(y0, view)
    dbcsr_matvec(dM, dx, dy2, alpha, beta, trans, engine=eng)
    torch.cuda.synchronize()
    assert same_bits(dy2.cpu().numpy(), got), "the same bits on every call"
    return got


def scaled_in_own_precision(beta, y):
    """beta y in the precision of y, every operation rounded on its own"""
    if is_complex(y.dtype):
        b, out = complex(beta), np.empty_like(y)
        out.real = b.real * y.real - b.imag * y.imag
        out.imag = b.real * y.imag + b.imag * y.real
        return out
    return (y.dtype.type(beta) * y).astype(y.dtype)


def c_matvec(eng, dM, trans, alpha, beta, kind, x, n_x, y, n_y, code=None):
    d = dM.desc()
    return eng.L.dbcsr_amd_bcsr_matvec(eng.h, dM.dtype_code if code is None else code, trans.encode(), _z(alpha), C.byref(d), kind,
                                       x.data_ptr() if x is not None else None, n_x, _z(beta), y.data_ptr() if y is not None else None, n_y, StreamHandle().ptr)


# ---- 1. every shape, type and op ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trans", ["N", "T", "C"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("which", ["mixed", "tiny", "tall70", "tall67", "gappy"])
def test_matvec(eng, which, dtype, trans):
    M, *parts = host_matrix(which, np.dtype(dtype).name, "N")
    check_product(eng, M, to_dev(M), tuple(parts), "N", trans)


@pytest.mark.parametrize("trans", ["N", "T", "C"])
@pytest.mark.parametrize("dtype,symmetry", TRIANGLES, ids=TRIANGLE_IDS)
def test_matvec_of_a_stored_triangle(eng, dtype, symmetry, trans):
    """the product is that of the desymmetrized matrix (formed in numpy)"""
    M, *parts = host_matrix("symmetric", np.dtype(dtype).name, symmetry)
    assert any(r != c for r, c in blocks_of(M)) and any(r == c for r, c in blocks_of(M))
    check_product(eng, M, to_dev(M), tuple(parts), symmetry, trans)


# ---- 2. operands like any other ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_matvec_of_an_operand_with_holes(eng, dtype):
    hB, dB = with_holes(eng, typed(base("mixed"), dtype, 1), dtype)
    holes = hole_positions(hB)
    assert holes.size > 0
    dB.data[torch.as_tensor(holes[:: max(1, holes.size // 7)], device="cuda")] = 1e30   # a hole is not the matrix': it must not count
    torch.cuda.synchronize()
    parts = dense_parts(hB, "N")
    for trans in ("N", "T", "C"):
        check_product(eng, hB, dB, parts, "N", trans)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("which", ["mixed", "tall70"])
def test_matvec_of_a_misaligned_data_area_and_vectors_that_are_views(eng, which, dtype):
    M, *parts = host_matrix(which, np.dtype(dtype).name, "N")
    dM = misaligned(to_dev(M))
    for trans in ("N", "T"):
        check_product(eng, M, dM, tuple(parts), "N", trans, view=True)


def test_matvec_of_a_misaligned_stored_triangle(eng):
    M, *parts = host_matrix("symmetric", "float64", "S")
    check_product(eng, M, misaligned(to_dev(M)), tuple(parts), "S", "N", view=True)


# ---- 3. special scalars --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,symmetry", [(np.float64, "N"), (np.float32, "N"), (np.complex128, "N"), (np.float64, "S"), (np.complex128, "H")],
                         ids=["fp64", "fp32", "z64", "fp64_S", "z64_H"])
def test_special_scalars(eng, dtype, symmetry):
    M, *parts = host_matrix("mixed" if symmetry == "N" else "symmetric", np.dtype(dtype).name, symmetry)
    parts = tuple(parts)
    dM = to_dev(M)
    dM.symmetry = symmetry
    alpha, beta = scalars(dtype)
    for trans in ("N", "C"):
        n_x, n_y = lengths(M, trans)
        x, y0 = random_vector(n_x, dtype, 23), random_vector(n_y, dtype, 24)
        dx = on_device(x)
        # beta == 0: y is not read
        dy = torch.full((n_y,), float("nan"), dtype=TORCH[np.dtype(dtype)], device="cuda")
        dbcsr_matvec(dM, dx, dy, alpha, 0.0, trans, engine=eng)
        torch.cuda.synchronize()
        got = dy.cpu().numpy()
        assert not np.any(np.isnan(got))
        ref, bar = reference(parts, trans, alpha, 0.0, x, None)
        within(got, ref, bar, "beta == 0, %s" % trans)
        # vec_out=None: the same product into a new vector of the matrix' type, on its device
        new = dbcsr_matvec(dM, dx, None, alpha, 0.0, trans, engine=eng)
        torch.cuda.synchronize()
        assert new.dtype == TORCH[np.dtype(dtype)] and new.is_cuda and new.shape == (n_y,) and same_bits(new.cpu().numpy(), got)
        # alpha == 0: A and x are not read, y <- beta y in the data's precision
        dy = on_device(y0)
        dnan = torch.full((n_x,), float("nan"), dtype=TORCH[np.dtype(dtype)], device="cuda")
        dbcsr_matvec(dM, dnan, dy, 0.0, beta, trans, engine=eng)
        torch.cuda.synchronize()
        assert same_bits(dy.cpu().numpy(), scaled_in_own_precision(beta, y0).astype(dtype)), "alpha == 0: beta y, bit for bit"
        # both zero: zeros
        dbcsr_matvec(dM, dnan, dy, 0.0, 0.0, trans, engine=eng)
        torch.cuda.synchronize()
        assert not np.any(dy.cpu().numpy())


# ---- 4. empty matrices, rows without blocks ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_empty_matrix(eng, dtype):
    M = typed(subset(base("mixed"), lambda r, c: False), dtype)
    dM = to_dev(M)
    alpha, beta = scalars(dtype)
    for trans in ("N", "T"):
        n_x, n_y = lengths(M, trans)
        x, y0 = random_vector(n_x, dtype, 25), random_vector(n_y, dtype, 26)
        dy = on_device(y0)
        dbcsr_matvec(dM, on_device(x), dy, alpha, beta, trans, engine=eng)
        torch.cuda.synchronize()
        assert same_bits(dy.cpu().numpy(), scaled_in_own_precision(beta, y0).astype(dtype))
        out = dbcsr_matvec(dM, on_device(x), trans=trans, engine=eng)
        torch.cuda.synchronize()
        assert out.shape == (n_y,) and not np.any(out.cpu().numpy())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_rows_without_blocks_get_beta_y(eng, dtype):
    M, *parts = host_matrix("gappy", np.dtype(dtype).name, "N")
    for trans in ("N", "T"):
        n = op_of(parts[2], "T" if trans != "N" else "N").sum(axis=1)
        bare = np.flatnonzero(n == 0)
        assert bare.size >= 3 and bare.size < n.size
        got = check_product(eng, M, to_dev(M), tuple(parts), "N", trans)
        _, beta = scalars(dtype)
        y0 = random_vector(n.size, dtype, 22)   # (check_product's old y)
        want = beta * y0.astype(wide(dtype))
        lim = (12 if is_complex(dtype) else 6) * U53 * np.abs(want).astype(np.float64) + (2.0 ** -24 * np.abs(want).astype(np.float64) if dtype == np.float32 else 0.0)
        assert np.all(np.abs(got.astype(want.dtype) - want).astype(np.float64)[bare] <= lim[bare])


# ---- 6. the lengths are kept ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,symmetry,trans", [(np.float64, "N", "N"), (np.float32, "N", "T"), (np.complex128, "N", "C"), (np.float64, "S", "N"),
                                                  (np.complex128, "K", "T")], ids=["fp64_N", "fp32_T", "z64_C", "fp64_S_N", "z64_K_T"])
def test_guard_elements(eng, dtype, symmetry, trans):
    """n_y three short: the last three elements of a full-length y keep their bits, the others are those of the full call; n_x three short with NaN
    behind it: no NaN comes out, the product is that of x with zeros there"""
    M, *parts = host_matrix("mixed" if symmetry == "N" else "symmetric", np.dtype(dtype).name, symmetry)
    parts = tuple(parts)
    dM = to_dev(M)
    kind = -1 if symmetry == "N" else L.SYMMETRY_KIND[symmetry]
    n_x, n_y = lengths(M, trans)
    alpha, beta = scalars(dtype)
    x, y0 = random_vector(n_x, dtype, 27), random_vector(n_y, dtype, 28)
    dx = on_device(x)
    full = on_device(y0)
    assert c_matvec(eng, dM, trans, alpha, beta, kind, dx, n_x, full, n_y) == 0
    short = on_device(y0)
    assert c_matvec(eng, dM, trans, alpha, beta, kind, dx, n_x, short, n_y - 3) == 0
    torch.cuda.synchronize()
    full, short = full.cpu().numpy(), short.cpu().numpy()
    ref, bar = reference(parts, trans, alpha, beta, x, y0)
    within(full, ref, bar, "the C entry")
    assert same_bits(short[-3:], y0[-3:]) and same_bits(short[:-3], full[:-3])
    xn = x.copy()
    xn[-3:] = np.nan
    dy = on_device(y0)
    assert c_matvec(eng, dM, trans, alpha, beta, kind, on_device(xn), n_x - 3, dy, n_y) == 0
    torch.cuda.synchronize()
    got = dy.cpu().numpy()
    assert not np.any(np.isnan(got))
    xz = x.copy()
    xz[-3:] = 0
    ref, bar = reference(parts, trans, alpha, beta, xz, y0)
    within(got, ref, bar, "n_x short")


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------------------
class Poisoned:
    """an engine that must not be used: any attribute access raises"""

    def __getattr__(self, name):
        raise AssertionError("the engine was used (%s)" % name)


def test_refusals_come_before_any_call():
    bad = Poisoned()
    A = base("mixed")
    dA = to_dev(A)
    rows, cols = full_len(A.row_sizes), full_len(A.col_sizes)
    x = torch.ones(cols, dtype=torch.float64, device="cuda")
    y = torch.ones(rows, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):
        dbcsr_matvec(dA, y, x, engine=bad)   # the rows' length for the columns
    with pytest.raises(ValueError):
        dbcsr_matvec(dA, x, y[:-1].contiguous(), engine=bad)
    with pytest.raises(ValueError):
        dbcsr_matvec(dA, x, y, trans="T", engine=bad)   # op(A) has the other shape
    with pytest.raises(TypeError):
        dbcsr_matvec(dA, x.float(), y, engine=bad)
    with pytest.raises(TypeError):
        dbcsr_matvec(dA, x, y.to(torch.complex128), engine=bad)
    with pytest.raises(TypeError):
        dbcsr_matvec(dA, np.ones(cols), y, engine=bad)
    with pytest.raises(ValueError):
        dbcsr_matvec(dA, x.cpu(), y, engine=bad)   # wrong device type
    with pytest.raises(ValueError):
        dbcsr_matvec(dA, x, y.cpu(), engine=bad)
    with pytest.raises(ValueError):
        dbcsr_matvec(dA, torch.ones(2 * cols, dtype=torch.float64, device="cuda")[::2], y, engine=bad)   # not contiguous
    with pytest.raises(ValueError):
        dbcsr_matvec(dA, x, torch.ones(2 * rows, dtype=torch.float64, device="cuda")[::2], engine=bad)
    for trans in ("X", "n", "", None):
        with pytest.raises(ValueError):
            dbcsr_matvec(dA, x, y, trans=trans, engine=bad)
    with pytest.raises(ValueError):
        dbcsr_matvec(dA, x, beta=0.5, engine=bad)   # beta != 0 without vec_out
    with pytest.raises(TypeError):
        dbcsr_matvec(dA, x, y, alpha=1j, engine=bad)
    with pytest.raises(TypeError):
        dbcsr_matvec(dA, x, y, beta=0.5 + 0j, engine=bad)
    # overlap
    Sq = to_dev(base("square"))
    n = full_len(base("square").row_sizes)
    big = torch.ones(2 * n, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):
        dbcsr_matvec(Sq, big[:n], big[:n], engine=bad)
    with pytest.raises(ValueError):
        dbcsr_matvec(Sq, big[:n], big[n - 1:2 * n - 1], engine=bad)
    with pytest.raises(ValueError):
        dbcsr_matvec(Sq, big[1:n + 1], big[:n], engine=bad)
    # symmetry
    Sq.symmetry = "X"
    with pytest.raises(ValueError):
        dbcsr_matvec(Sq, big[:n], big[n:], engine=bad)
    Sq.symmetry = "H"   # real data: 'S' and 'A'
    with pytest.raises(ValueError):
        dbcsr_matvec(Sq, big[:n], big[n:], engine=bad)
    tri = to_dev(subset(A, lambda r, c: r <= c))
    tri.symmetry = "S"
    with pytest.raises(ValueError):
        dbcsr_matvec(tri, x, y, engine=bad)   # a matrix with symmetry that is not square
    torch.cuda.synchronize()
    assert not np.any(big.cpu().numpy() != 1.0) and not np.any(y.cpu().numpy() != 1.0)
    assert dbcsr_amd.dbcsr_matvec is dbcsr_matvec and "dbcsr_matvec" in dbcsr_amd.__all__


# ---- 8. the C entry's answers ----------------------------------------------------------------------------------------------------------------------------
def test_c_abi_answers(eng):
    A, Sq = base("mixed"), base("square")
    dA, dS = to_dev(A), to_dev(Sq)
    n = full_len(Sq.row_sizes)
    big = torch.ones(2 * n, dtype=torch.float64, device="cuda")
    x, y = big[:n], big[n:]
    for code in (L.dbcsr_type_complex_4, 2, 99):
        assert c_matvec(eng, dS, "N", 1.0, 0.0, -1, x, n, y, n, code=code) == -10
    assert c_matvec(eng, dS, "N", 1.0, 0.0, -1, None, n, y, n) == -1
    assert c_matvec(eng, dS, "N", 1.0, 0.0, -1, x, n, None, n) == -1
    d = dS.desc()
    st = StreamHandle().ptr
    f64 = L.dbcsr_type_real_8
    assert eng.L.dbcsr_amd_bcsr_matvec(None, f64, b"N", _z(1.0), C.byref(d), -1, x.data_ptr(), n, _z(0.0), y.data_ptr(), n, st) == -1
    assert eng.L.dbcsr_amd_bcsr_matvec(eng.h, f64, b"N", None, C.byref(d), -1, x.data_ptr(), n, _z(0.0), y.data_ptr(), n, st) == -1
    assert eng.L.dbcsr_amd_bcsr_matvec(eng.h, f64, b"N", _z(1.0), None, -1, x.data_ptr(), n, _z(0.0), y.data_ptr(), n, st) == -1
    assert eng.L.dbcsr_amd_bcsr_matvec(eng.h, f64, b"N", _z(1.0), C.byref(d), -1, x.data_ptr(), n, None, y.data_ptr(), n, st) == -1
    for kind in (4, -2):
        assert c_matvec(eng, dS, "N", 1.0, 0.0, kind, x, n, y, n) == -1
    for trans in ("X", "n"):
        assert c_matvec(eng, dS, trans, 1.0, 0.0, -1, x, n, y, n) == -1
    assert c_matvec(eng, dS, "N", 1.0, 0.0, -1, x, -1, y, n) == -1
    # overlapping vectors: the same, by one element from either side; vectors that touch do not overlap
    assert c_matvec(eng, dS, "N", 1.0, 0.0, -1, x, n, x, n) == -1
    assert c_matvec(eng, dS, "N", 1.0, 0.0, -1, x, n, big[n - 1:2 * n - 1], n) == -1
    assert c_matvec(eng, dS, "N", 1.0, 0.0, -1, big[1:n + 1], n, x, n) == -1
    # a stored triangle needs a square block structure
    xa = torch.ones(full_len(A.col_sizes), dtype=torch.float64, device="cuda")
    ya = torch.ones(full_len(A.row_sizes), dtype=torch.float64, device="cuda")
    assert c_matvec(eng, dA, "N", 1.0, 0.0, 0, xa, xa.numel(), ya, ya.numel()) == -1
    torch.cuda.synchronize()
    assert not np.any(big.cpu().numpy() != 1.0) and not np.any(ya.cpu().numpy() != 1.0)
    assert c_matvec(eng, dS, "N", 1.0, 0.0, -1, x, n, y, n) == 0   # (and the vectors that touch are served)
    # H and K on real data behave as S and A
    T = typed(symmetric_base("S"), np.float64, 3)
    dT = to_dev(T)
    nt = full_len(T.row_sizes)
    xt = on_device(random_vector(nt, np.float64, 29))
    outs = []
    for kind in (0, 2, 1, 3):
        yt = torch.zeros(nt, dtype=torch.float64, device="cuda")
        assert c_matvec(eng, dT, "C", 1.0, 0.0, kind, xt, nt, yt, nt) == 0
        torch.cuda.synchronize()
        outs.append(yt.cpu().numpy())
    assert same_bits(outs[0], outs[1]) and same_bits(outs[2], outs[3]) and not same_bits(outs[0], outs[2])
    # an empty matrix: 0, y <- beta y
    dE = to_dev(subset(Sq, lambda r, c: False))
    ye = torch.full((n,), 3.0, dtype=torch.float64, device="cuda")
    assert c_matvec(eng, dE, "N", 1.0, 0.5, -1, x, n, ye, n) == 0
    torch.cuda.synchronize()
    assert not np.any(ye.cpu().numpy() != 1.5)


# ---- 9. between multiplies -----------------------------------------------------------------------------------------------------------------------------
def test_matvec_between_multiplies_keeps_the_plan(monkeypatch):
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
    x = on_device(random_vector(full_len(sizes), np.float64, 30))
    tensors = [(m.row_p, m.col_i, m.blk_p, m.data) for m in (dA, dC)]
    stamps = (dA.index_stamp(), dC.index_stamp())
    for trans in ("N", "T"):
        dbcsr_matvec(dA, x, trans=trans, engine=eng)   # of its operand ...
        dbcsr_matvec(dC, x, trans=trans, engine=eng)   # ... and of its result
    dA.symmetry = "S"
    dbcsr_matvec(dA, x, engine=eng)   # (both passes: the per-column lists are built in the algebra's own buffers)
    dA.symmetry = "N"
    assert (dA.index_stamp(), dC.index_stamp()) == stamps
    assert all(a is b for m, t in zip((dA, dC), tensors) for a, b in zip((m.row_p, m.col_i, m.blk_p, m.data), t))
    dbcsr_multiply("N", "N", 1.0, dA, dB, 0.0, dC, engine=eng)
    assert eng.plan_stats() == (1, 1), "a multiply after matrix-vector products must reuse its plan"
    torch.cuda.synchronize()
    assert same_bits(dev_to_bcsr(dA).data, A.data)
    product_bar(dev_to_bcsr(dC), 1.0, dense(A), dense(B))


# ---- 10. end to end --------------------------------------------------------------------------------------------------------------------------------------
def test_power_iteration_on_the_device(eng):
    """twelve steps v <- A v / ||A v|| on a stored triangle with dbcsr_matvec and torch vector operations only; the same steps in numpy on the
    desymmetrized dense matrix.  The Rayleigh quotient of a unit vector lies below the Gershgorin norm."""
    M, F, _, _ = host_matrix("symmetric", "float64", "S")
    D = F.astype(np.float64)
    dM = to_dev(M)
    dM.symmetry = "S"
    n = full_len(M.row_sizes)
    v = np.abs(random_vector(n, np.float64, 31))
    v /= np.linalg.norm(v)
    dv = on_device(v)
    dw = torch.empty_like(dv)
    for _ in range(12):
        w = D @ v
        v = w / np.linalg.norm(w)
        dbcsr_matvec(dM, dv, dw, engine=eng)
        torch.div(dw, torch.linalg.vector_norm(dw), out=dv)
    rq = float(torch.dot(dv, dbcsr_matvec(dM, dv, dw, engine=eng)))
    torch.cuda.synchronize()
    err = float(np.max(np.abs(dv.cpu().numpy() - v)))
    ger = dbcsr_gershgorin_norm(dM, engine=eng)
    print("power iteration: max element error %.3e; Rayleigh quotient %.6f (numpy %.6f), Gershgorin norm %.6f" % (err, rq, float(v @ (D @ v)), ger))
    assert err <= 1e-10
    assert abs(rq - float(v @ (D @ v))) <= 1e-10 * ger and abs(rq) <= ger
