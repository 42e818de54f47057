"""The block-sparse matrix times several dense vectors on the device, Y <- alpha op(A) X + beta Y (dbcsr_amd/operations.py: dbcsr_multivec;
dbcsr_amd_bcsr_multivec of include/dbcsr_amd_mm.h; kernels algebra_multivec_rows / _cols / _combine of dbcsr_amd/csrc/mm_multivec.h) for float64, float32
and complex128.

Reference and bars are those of tests/test_gpu_matvec.py, applied per column: numpy long double on the dense (desymmetrized) scatter;
|got - ref| <= (n_i + 6) u w_i for real data, (n_i + 12) u w_i for complex data, plus the reference's own n_i eps_ld w_i, plus 2^-24 |ref| for float32,
with u = 2^-53, n_i the stored elements of full row i of op(A) and w_i = |alpha| sum_j |a_ij| |x_jv| + |beta| |y_iv|.  The bars are derived there for ANY
order of summation, so they hold for these kernels unchanged; nothing is compared against the code's own output except the bits of a second call.

Right-hand sides: 1 and 3 (less than a tile of 16: one, and odd), 16 (one tile), 17 (a tile and a one-column tile), 37 (three tiles of one workgroup,
the last one partial; and once 70, five tiles in two workgroups) -- each as a contiguous (n, nrhs) tensor (ld = nrhs) and as a view with ld = nrhs + 3 that starts one element into its
allocation (not 16-byte aligned for real data), whose padding columns and surroundings hold a canary that must keep its bits.
Matrices: those of tests/test_gpu_matrix_norms.py / test_gpu_matvec.py (every one a few hundred full rows)."""
import ctypes as C

import numpy as np
import pytest
import torch

import dbcsr_amd
from dbcsr_amd import lib as L
from dbcsr_amd import operations as OPS
from dbcsr_amd.matrix import StreamHandle
from dbcsr_amd.multiply import MultiplyEngine, _z, dbcsr_multiply
from dbcsr_amd.operations import dbcsr_matvec, dbcsr_multivec
from tests.gpu_util import dev_to_bcsr, to_dev
from tests.test_gpu_matrix_norms import (DTYPES, IDS, TORCH, base, dense, full_len, hole_positions, is_complex, misaligned, product_bar, random_vector,
                                         same_bits, subset, typed, with_holes)
from tests.test_gpu_matvec import (TRIANGLE_IDS, TRIANGLES, Poisoned, dense_parts, host_matrix, lengths, reference, scalars, scaled_in_own_precision,
                                   within)

pytestmark = pytest.mark.gpu

NRHS = [1, 3, 16, 17, 37]
CANARY = -77.25


@pytest.fixture(scope="module")
def eng():
    return MultiplyEngine()


def random_vectors(n, nrhs, dtype, seed):
    return np.ascontiguousarray(random_vector(n * nrhs, dtype, seed).reshape(n, nrhs))


def reference_columns(parts, trans, alpha, beta, x, y0):
    """(ref, bar) of alpha op(F) X + beta Y0, column by column: test_gpu_matvec.reference for every right-hand side"""
    cols = [reference(parts, trans, alpha, beta, x[:, v], None if y0 is None else y0[:, v]) for v in range(x.shape[1])]
    return np.stack([c[0] for c in cols], axis=1), np.stack([c[1] for c in cols], axis=1)


def within_columns(got, ref, bar, what):
    assert got.shape == ref.shape
    within(got.reshape(-1), ref.reshape(-1), bar.reshape(-1), what)


class Dev:
    """a host matrix of right-hand sides on the device: contiguous, or (view) with ld = nrhs + 3 one element into an allocation full of canaries"""

    def __init__(self, a, view=False, extra_rows=0):
        n, nrhs = a.shape
        tdt = TORCH[a.dtype]
        self.view = view
        if not view:
            self.big = torch.full(((n + extra_rows) * nrhs,), CANARY, dtype=tdt, device="cuda")
            self.ld, start = nrhs, 0
        else:
            self.ld, start = nrhs + 3, 1
            self.big = torch.full((1 + (n + extra_rows) * self.ld + 2,), CANARY, dtype=tdt, device="cuda")
        self.t = self.big[start:start + n * self.ld].view(n, self.ld)[:, :nrhs]
        if a.size:
            self.t.copy_(torch.as_tensor(a))
        own = np.zeros(self.big.numel(), bool)
        own[start:start + n * self.ld].reshape(n, self.ld)[:, :nrhs] = True
        self.own = own
        assert self.t.data_ptr() == self.big.data_ptr() + start * self.big.element_size()
        assert not view or n < 2 or (self.t.stride(0) == self.ld and (is_complex(a.dtype) or self.t.data_ptr() % 16 != 0))

    def host(self):
        return self.t.cpu().numpy()

    def canaries_kept(self):
        """every element of the allocation outside the (n, nrhs) window still holds the canary, bit for bit"""
        b = self.big.cpu().numpy()
        return same_bits(b[~self.own], np.full(int((~self.own).sum()), CANARY, b.dtype))


def check_product(eng, M, dM, parts, symmetry, trans, nrhs, view=False):
    """one product with general scalars against the reference; the same bits from a second call; X unchanged; nothing written outside Y's window"""
    dtype = M.data.dtype
    dM.symmetry = symmetry
    n_x, n_y = lengths(M, trans)
    alpha, beta = scalars(dtype)
    x, y0 = random_vectors(n_x, nrhs, dtype, 41), random_vectors(n_y, nrhs, dtype, 42)
    dx, dy = Dev(x, view), Dev(y0, view)
    out = dbcsr_multivec(dM, dx.t, dy.t, alpha, beta, trans, engine=eng)
    torch.cuda.synchronize()
    assert out is dy.t and same_bits(dx.host(), x) and dx.canaries_kept() and dy.canaries_kept()
    got = dy.host()
    ref, bar = reference_columns(parts, trans, alpha, beta, x, y0)
    within_columns(got, ref, bar, "multivec %s, symmetry %s, nrhs %d%s" % (trans, symmetry, nrhs, ", a view" if view else ""))
    dy2 = Dev(y0, view)
    dbcsr_multivec(dM, dx.t, dy2.t, alpha, beta, trans, engine=eng)
    torch.cuda.synchronize()
    assert same_bits(dy2.host(), got), "the same bits on every call"
    return got


def c_multivec(eng, dM, trans, alpha, beta, kind, nrhs, x, n_x, ldx, y, n_y, ldy, code=None):
    d = dM.desc()
    return eng.L.dbcsr_amd_bcsr_multivec(eng.h, dM.dtype_code if code is None else code, trans.encode(), _z(alpha), C.byref(d), kind, nrhs,
                                         x.data_ptr() if x is not None else None, n_x, ldx, _z(beta), y.data_ptr() if y is not None else None, n_y, ldy,
                                         StreamHandle().ptr)


# ---- 1. every matrix, op, type and count of right-hand sides -------------------------------------------------------------------------------------
@pytest.mark.parametrize("trans", ["N", "T", "C"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("which", ["mixed", "tiny", "tall70", "tall67", "gappy"])
def test_multivec(eng, which, dtype, trans):
    M, *parts = host_matrix(which, np.dtype(dtype).name, "N")
    dM = to_dev(M)
    for nrhs in NRHS:
        for view in (False, True):
            check_product(eng, M, dM, tuple(parts), "N", trans, nrhs, view)


@pytest.mark.parametrize("which,dtype,trans", [("mixed", np.float64, "N"), ("mixed", np.float32, "T"), ("tall70", np.complex128, "C")],
                         ids=["mixed_fp64_N", "mixed_fp32_T", "tall70_z64_C"])
def test_more_right_hand_sides_than_one_workgroup_takes(eng, which, dtype, trans):
    """70 right-hand sides are five tiles: a workgroup of four waves and a second one whose last three waves have no tile and only help to load
    the blocks -- the one path of the kernels that the counts up to 37 do not reach"""
    M, *parts = host_matrix(which, np.dtype(dtype).name, "N")
    check_product(eng, M, to_dev(M), tuple(parts), "N", trans, 70, view=True)


@pytest.mark.parametrize("trans", ["N", "T", "C"])
@pytest.mark.parametrize("dtype,symmetry", TRIANGLES, ids=TRIANGLE_IDS)
def test_multivec_of_a_stored_triangle(eng, dtype, symmetry, trans):
    """the product is that of the desymmetrized matrix (formed in numpy)"""
    M, *parts = host_matrix("symmetric", np.dtype(dtype).name, symmetry)
    dM = to_dev(M)
    for nrhs in (3, 17):
        check_product(eng, M, dM, tuple(parts), symmetry, trans, nrhs, view=nrhs == 17)


# ---- 2. operands like any other ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_multivec_of_an_operand_with_holes(eng, dtype):
    hB, dB = with_holes(eng, typed(base("mixed"), dtype, 1), dtype)
    holes = hole_positions(hB)
    assert holes.size > 0
    dB.data[torch.as_tensor(holes[:: max(1, holes.size // 7)], device="cuda")] = 1e30   # a hole is not the matrix': it must not count
    torch.cuda.synchronize()
    parts = dense_parts(hB, "N")
    for trans in ("N", "T", "C"):
        check_product(eng, hB, dB, parts, "N", trans, 17)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("which", ["mixed", "tall70"])
def test_multivec_of_a_misaligned_data_area(eng, which, dtype):
    M, *parts = host_matrix(which, np.dtype(dtype).name, "N")
    dM = misaligned(to_dev(M))
    for trans in ("N", "T"):
        check_product(eng, M, dM, tuple(parts), "N", trans, 17, view=True)


def test_multivec_of_a_misaligned_stored_triangle(eng):
    M, *parts = host_matrix("symmetric", "float64", "S")
    check_product(eng, M, misaligned(to_dev(M)), tuple(parts), "S", "N", 17, view=True)


# ---- 3. the window of Y and the lengths are kept --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,symmetry,trans", [(np.float64, "N", "N"), (np.float32, "N", "T"), (np.complex128, "N", "C"), (np.float64, "S", "N"),
                                                  (np.complex128, "K", "T")], ids=["fp64_N", "fp32_T", "z64_C", "fp64_S_N", "z64_K_T"])
@pytest.mark.parametrize("nrhs", [3, 17])
def test_rows_and_padding_outside_the_window_are_never_touched(eng, dtype, symmetry, trans, nrhs):
    """through the C entry, on views with ld = nrhs + 3: a Y with four rows more than the full length keeps them; n_y three short leaves the last three
    rows of a full-length Y alone and gives the others the bits of the full call; n_x three short with NaN in the rows behind it: no NaN comes out,
    the product is that of X with zeros there.  Padding columns and the elements around every view keep their canary."""
    M, *parts = host_matrix("mixed" if symmetry == "N" else "symmetric", np.dtype(dtype).name, symmetry)
    parts = tuple(parts)
    dM = to_dev(M)
    kind = -1 if symmetry == "N" else L.SYMMETRY_KIND[symmetry]
    n_x, n_y = lengths(M, trans)
    alpha, beta = scalars(dtype)
    x, y0 = random_vectors(n_x, nrhs, dtype, 43), random_vectors(n_y, nrhs, dtype, 44)
    dx, full = Dev(x, True), Dev(y0, True)
    assert c_multivec(eng, dM, trans, alpha, beta, kind, nrhs, dx.t, n_x, dx.ld, full.t, n_y, full.ld) == 0
    torch.cuda.synchronize()
    ref, bar = reference_columns(parts, trans, alpha, beta, x, y0)
    within_columns(full.host(), ref, bar, "the C entry")
    assert full.canaries_kept() and dx.canaries_kept()
    # a longer Y: its rows behind the full length stay
    more = np.concatenate([y0, random_vectors(4, nrhs, dtype, 45)])
    longer = Dev(more, True)
    assert c_multivec(eng, dM, trans, alpha, beta, kind, nrhs, dx.t, n_x, dx.ld, longer.t, n_y + 4, longer.ld) == 0
    torch.cuda.synchronize()
    got = longer.host()
    assert same_bits(got[n_y:], more[n_y:]) and same_bits(got[:n_y], full.host()) and longer.canaries_kept()
    # n_y three short: the rows at and behind it are canary rows of the allocation
    short = Dev(y0[:n_y - 3], True, extra_rows=3)
    assert c_multivec(eng, dM, trans, alpha, beta, kind, nrhs, dx.t, n_x, dx.ld, short.t, n_y - 3, short.ld) == 0
    torch.cuda.synchronize()
    assert same_bits(short.host(), full.host()[:n_y - 3]) and short.canaries_kept()
    # n_x three short: the rows behind it hold NaN and are not read
    xn = x.copy()
    xn[-3:] = np.nan
    dy = Dev(y0, True)
    assert c_multivec(eng, dM, trans, alpha, beta, kind, nrhs, Dev(xn, True).t, n_x - 3, nrhs + 3, dy.t, n_y, dy.ld) == 0
    torch.cuda.synchronize()
    got = dy.host()
    assert not np.any(np.isnan(got)) and dy.canaries_kept()
    xz = x.copy()
    xz[-3:] = 0
    ref, bar = reference_columns(parts, trans, alpha, beta, xz, y0)
    within_columns(got, ref, bar, "n_x short")


# ---- 4. zero scalars, an empty matrix, no right-hand side -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,symmetry", [(np.float64, "N"), (np.float32, "N"), (np.complex128, "N"), (np.float64, "S"), (np.complex128, "H")],
                         ids=["fp64", "fp32", "z64", "fp64_S", "z64_H"])
def test_zero_scalars(eng, dtype, symmetry):
    M, *parts = host_matrix("mixed" if symmetry == "N" else "symmetric", np.dtype(dtype).name, symmetry)
    parts = tuple(parts)
    dM = to_dev(M)
    dM.symmetry = symmetry
    alpha, beta = scalars(dtype)
    tdt = TORCH[np.dtype(dtype)]
    nrhs = 17
    for trans in ("N", "C"):
        n_x, n_y = lengths(M, trans)
        x, y0 = random_vectors(n_x, nrhs, dtype, 46), random_vectors(n_y, nrhs, dtype, 47)
        dx = Dev(x)
        # beta == 0: Y is not read
        dy = torch.full((n_y, nrhs), float("nan"), dtype=tdt, device="cuda")
        dbcsr_multivec(dM, dx.t, dy, alpha, 0.0, trans, engine=eng)
        torch.cuda.synchronize()
        got = dy.cpu().numpy()
        assert not np.any(np.isnan(got))
        ref, bar = reference_columns(parts, trans, alpha, 0.0, x, None)
        within_columns(got, ref, bar, "beta == 0, %s" % trans)
        # vecs_out=None: the same product into a new (n_y, nrhs) tensor of the matrix' type, on its device
        new = dbcsr_multivec(dM, dx.t, None, alpha, 0.0, trans, engine=eng)
        torch.cuda.synchronize()
        assert new.dtype == tdt and new.is_cuda and new.shape == (n_y, nrhs) and new.is_contiguous() and same_bits(new.cpu().numpy(), got)
        # alpha == 0: A and X are not read, Y <- beta Y in the data's precision
        dy = Dev(y0, True)
        dnan = torch.full((n_x, nrhs), float("nan"), dtype=tdt, device="cuda")
        dbcsr_multivec(dM, dnan, dy.t, 0.0, beta, trans, engine=eng)
        torch.cuda.synchronize()
        assert same_bits(dy.host(), scaled_in_own_precision(beta, y0).astype(dtype)), "alpha == 0: beta Y, bit for bit"
        assert dy.canaries_kept()
        # both zero: zeros
        dbcsr_multivec(dM, dnan, dy.t, 0.0, 0.0, trans, engine=eng)
        torch.cuda.synchronize()
        assert not np.any(dy.host()) and dy.canaries_kept()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_empty_matrix_and_no_right_hand_side(eng, dtype):
    M = typed(subset(base("mixed"), lambda r, c: False), dtype)
    dM = to_dev(M)
    alpha, beta = scalars(dtype)
    for trans in ("N", "T"):
        n_x, n_y = lengths(M, trans)
        x, y0 = random_vectors(n_x, 3, dtype, 48), random_vectors(n_y, 3, dtype, 49)
        dy = Dev(y0, True)
        dbcsr_multivec(dM, Dev(x).t, dy.t, alpha, beta, trans, engine=eng)
        torch.cuda.synchronize()
        assert same_bits(dy.host(), scaled_in_own_precision(beta, y0).astype(dtype)) and dy.canaries_kept()
        out = dbcsr_multivec(dM, Dev(x).t, trans=trans, engine=eng)
        torch.cuda.synchronize()
        assert out.shape == (n_y, 3) and not np.any(out.cpu().numpy())
    # nrhs == 0: returns, and writes nothing
    F = typed(base("mixed"), dtype, 1)
    dF = to_dev(F)
    n_x, n_y = lengths(F, "N")
    tdt = TORCH[np.dtype(dtype)]
    out = dbcsr_multivec(dF, torch.empty((n_x, 0), dtype=tdt, device="cuda"), engine=eng)
    assert out.shape == (n_y, 0)
    guard = Dev(random_vectors(n_y, 3, dtype, 50))
    before = guard.host().copy()
    xs = Dev(random_vectors(n_x, 3, dtype, 51))
    assert c_multivec(eng, dF, "N", alpha, beta, -1, 0, xs.t, n_x, 3, guard.t, n_y, 3) == 0
    assert c_multivec(eng, dF, "N", alpha, beta, -1, 3, xs.t, n_x, 3, guard.t, 0, 3) == 0
    torch.cuda.synchronize()
    assert same_bits(guard.host(), before)


# ---- 5. agreement with the matrix-vector product -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,symmetry,trans", [(np.float64, "N", "N"), (np.float32, "N", "T"), (np.complex128, "N", "C"), (np.float64, "S", "N"),
                                                  (np.complex128, "H", "C")], ids=["fp64_N", "fp32_T", "z64_C", "fp64_S_N", "z64_H_C"])
def test_every_column_agrees_with_the_matvec(eng, dtype, symmetry, trans):
    """column v of the result and dbcsr_matvec of column v lie within their bars of the same reference, so within the sum of the two of each other"""
    M, *parts = host_matrix("mixed" if symmetry == "N" else "symmetric", np.dtype(dtype).name, symmetry)
    dM = to_dev(M)
    dM.symmetry = symmetry
    n_x, n_y = lengths(M, trans)
    alpha, beta = scalars(dtype)
    nrhs = 17
    x, y0 = random_vectors(n_x, nrhs, dtype, 52), random_vectors(n_y, nrhs, dtype, 53)
    got = dbcsr_multivec(dM, Dev(x).t, Dev(y0).t, alpha, beta, trans, engine=eng).cpu().numpy()
    ref, bar = reference_columns(tuple(parts), trans, alpha, beta, x, y0)
    within_columns(got, ref, bar, "multivec")
    for v in (0, 7, 15, 16):
        one = dbcsr_matvec(dM, torch.as_tensor(x[:, v].copy()).cuda(), torch.as_tensor(y0[:, v].copy()).cuda(), alpha, beta, trans, engine=eng).cpu().numpy()
        within(one, ref[:, v], bar[:, v], "matvec of column %d" % v)
        assert np.all(np.abs(got[:, v].astype(ref.dtype) - one.astype(ref.dtype)).astype(np.float64) <= 2 * bar[:, v])


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_call(monkeypatch):
    bad = Poisoned()
    monkeypatch.setattr(OPS, "default_engine", lambda: bad)   # (and no engine of its own is made either)
    A = base("mixed")
    dA = to_dev(A)
    rows, cols = full_len(A.row_sizes), full_len(A.col_sizes)
    x = torch.ones((cols, 3), dtype=torch.float64, device="cuda")
    y = torch.ones((rows, 3), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):
        dbcsr_multivec(dA, y, x, engine=bad)   # the rows' length for the columns
    with pytest.raises(ValueError):
        dbcsr_multivec(dA, x, y[:-1].contiguous(), engine=bad)
    with pytest.raises(ValueError):
        dbcsr_multivec(dA, x, y, trans="T", engine=bad)   # op(A) has the other shape
    with pytest.raises(ValueError):
        dbcsr_multivec(dA, x, y[:, :2].contiguous(), engine=bad)   # another count of right-hand sides
    with pytest.raises(ValueError):
        dbcsr_multivec(dA, x[:, 0], y[:, 0], engine=bad)   # 1-D: dbcsr_matvec's operands
    with pytest.raises(TypeError):
        dbcsr_multivec(dA, x.float(), y, engine=bad)
    with pytest.raises(TypeError):
        dbcsr_multivec(dA, x, y.to(torch.complex128), engine=bad)
    with pytest.raises(TypeError):
        dbcsr_multivec(dA, np.ones((cols, 3)), y, engine=bad)
    with pytest.raises(ValueError):
        dbcsr_multivec(dA, x.cpu(), y, engine=bad)   # wrong device type
    with pytest.raises(ValueError):
        dbcsr_multivec(dA, x, y.cpu(), engine=bad)
    with pytest.raises(ValueError):
        dbcsr_multivec(dA, torch.ones((cols, 6), dtype=torch.float64, device="cuda")[:, ::2], y, engine=bad)   # stride(1) != 1
    with pytest.raises(ValueError):
        dbcsr_multivec(dA, x, torch.ones((3, rows), dtype=torch.float64, device="cuda").t(), engine=bad)   # column by column
    with pytest.raises(ValueError):
        dbcsr_multivec(dA, torch.ones(3 * cols, dtype=torch.float64, device="cuda").as_strided((cols, 3), (2, 1)), y, engine=bad)   # stride(0) < nrhs
    for trans in ("X", "n", "", None):
        with pytest.raises(ValueError):
            dbcsr_multivec(dA, x, y, trans=trans, engine=bad)
    with pytest.raises(ValueError):
        dbcsr_multivec(dA, x, beta=0.5, engine=bad)   # beta != 0 without vecs_out
    with pytest.raises(ValueError):
        dbcsr_multivec(dA, x, beta=0.5)   # (nor is the default engine asked for)
    with pytest.raises(TypeError):
        dbcsr_multivec(dA, x, y, alpha=1j, engine=bad)
    with pytest.raises(TypeError):
        dbcsr_multivec(dA, x, y, beta=0.5 + 0j, engine=bad)
    # overlap: the same window, windows that share one element, columns of one basis that interleave without a common element still overlap as ranges
    Sq = to_dev(base("square"))
    n = full_len(base("square").row_sizes)
    big = torch.ones(2 * n * 3 + 8, dtype=torch.float64, device="cuda")
    first, second = big[:3 * n].view(n, 3), big[3 * n:6 * n].view(n, 3)
    with pytest.raises(ValueError):
        dbcsr_multivec(Sq, first, first, engine=bad)
    with pytest.raises(ValueError):
        dbcsr_multivec(Sq, first, big[3 * n - 1:6 * n - 1].view(n, 3), engine=bad)
    with pytest.raises(ValueError):
        dbcsr_multivec(Sq, big[1:3 * n + 1].view(n, 3), first, engine=bad)
    basis = big[:6 * n].view(n, 6)
    with pytest.raises(ValueError):
        dbcsr_multivec(Sq, basis[:, :3], basis[:, 3:], engine=bad)
    # symmetry
    Sq.symmetry = "X"
    with pytest.raises(ValueError):
        dbcsr_multivec(Sq, first, second, engine=bad)
    Sq.symmetry = "H"   # real data: 'S' and 'A'
    with pytest.raises(ValueError):
        dbcsr_multivec(Sq, first, second, engine=bad)
    tri = to_dev(subset(A, lambda r, c: r <= c))
    tri.symmetry = "S"
    with pytest.raises(ValueError):
        dbcsr_multivec(tri, x, y, engine=bad)   # a matrix with symmetry that is not square
    torch.cuda.synchronize()
    assert not np.any(big.cpu().numpy() != 1.0) and not np.any(y.cpu().numpy() != 1.0)
    assert dbcsr_amd.dbcsr_multivec is dbcsr_multivec and "dbcsr_multivec" in dbcsr_amd.__all__


def test_c_abi_answers(eng):
    A, Sq = base("mixed"), base("square")
    dA, dS = to_dev(A), to_dev(Sq)
    n = full_len(Sq.row_sizes)
    k = 3
    big = torch.ones(2 * n * k, dtype=torch.float64, device="cuda")
    x, y = big[:n * k].view(n, k), big[n * k:].view(n, k)
    for code in (L.dbcsr_type_complex_4, 2, 99):
        assert c_multivec(eng, dS, "N", 1.0, 0.0, -1, k, x, n, k, y, n, k, code=code) == -10
    assert c_multivec(eng, dS, "N", 1.0, 0.0, -1, k, None, n, k, y, n, k) == -1
    assert c_multivec(eng, dS, "N", 1.0, 0.0, -1, k, x, n, k, None, n, k) == -1
    d = dS.desc()
    st = StreamHandle().ptr
    f64 = L.dbcsr_type_real_8
    call = eng.L.dbcsr_amd_bcsr_multivec
    assert call(None, f64, b"N", _z(1.0), C.byref(d), -1, k, x.data_ptr(), n, k, _z(0.0), y.data_ptr(), n, k, st) == -1
    assert call(eng.h, f64, b"N", None, C.byref(d), -1, k, x.data_ptr(), n, k, _z(0.0), y.data_ptr(), n, k, st) == -1
    assert call(eng.h, f64, b"N", _z(1.0), None, -1, k, x.data_ptr(), n, k, _z(0.0), y.data_ptr(), n, k, st) == -1
    assert call(eng.h, f64, b"N", _z(1.0), C.byref(d), -1, k, x.data_ptr(), n, k, None, y.data_ptr(), n, k, st) == -1
    for kind in (4, -2):
        assert c_multivec(eng, dS, "N", 1.0, 0.0, kind, k, x, n, k, y, n, k) == -1
    for trans in ("X", "n"):
        assert c_multivec(eng, dS, trans, 1.0, 0.0, -1, k, x, n, k, y, n, k) == -1
    assert c_multivec(eng, dS, "N", 1.0, 0.0, -1, -1, x, n, k, y, n, k) == -1      # nrhs < 0
    assert c_multivec(eng, dS, "N", 1.0, 0.0, -1, k, x, n, k - 1, y, n, k) == -1   # ldx < nrhs
    assert c_multivec(eng, dS, "N", 1.0, 0.0, -1, k, x, n, k, y, n, k - 1) == -1   # ldy < nrhs
    assert c_multivec(eng, dS, "N", 1.0, 0.0, -1, k, x, -1, k, y, n, k) == -1
    # element ranges that intersect: the same, by one element from either side, two column slices of one basis; ranges that touch do not
    assert c_multivec(eng, dS, "N", 1.0, 0.0, -1, k, x, n, k, x, n, k) == -1
    assert c_multivec(eng, dS, "N", 1.0, 0.0, -1, k, x, n, k, big[n * k - 1:2 * n * k - 1], n, k) == -1
    assert c_multivec(eng, dS, "N", 1.0, 0.0, -1, k, big[1:n * k + 1], n, k, x, n, k) == -1
    assert c_multivec(eng, dS, "N", 1.0, 0.0, -1, k, big[:], n, 2 * k, big[k:], n, 2 * k) == -1
    # a stored triangle needs a square block structure
    xa = torch.ones((full_len(A.col_sizes), k), dtype=torch.float64, device="cuda")
    ya = torch.ones((full_len(A.row_sizes), k), dtype=torch.float64, device="cuda")
    assert c_multivec(eng, dA, "N", 1.0, 0.0, 0, k, xa, xa.shape[0], k, ya, ya.shape[0], k) == -1
    torch.cuda.synchronize()
    assert not np.any(big.cpu().numpy() != 1.0) and not np.any(ya.cpu().numpy() != 1.0)
    assert c_multivec(eng, dS, "N", 1.0, 0.0, -1, k, x, n, k, y, n, k) == 0   # (and the ranges that touch are served)
    # an empty matrix: 0, Y <- beta Y
    dE = to_dev(subset(Sq, lambda r, c: False))
    ye = torch.full((n, k), 3.0, dtype=torch.float64, device="cuda")
    assert c_multivec(eng, dE, "N", 1.0, 0.5, -1, k, x, n, k, ye, n, k) == 0
    torch.cuda.synchronize()
    assert not np.any(ye.cpu().numpy() != 1.5)


# ---- 7. between multiplies -----------------------------------------------------------------------------------------------------------------------------
def test_multivec_between_multiplies_keeps_the_plan(monkeypatch):
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
    x = Dev(random_vectors(full_len(sizes), 17, np.float64, 54)).t
    tensors = [(m.row_p, m.col_i, m.blk_p, m.data) for m in (dA, dC)]
    stamps = (dA.index_stamp(), dC.index_stamp())
    for trans in ("N", "T"):
        dbcsr_multivec(dA, x, trans=trans, engine=eng)   # of its operand ...
        dbcsr_multivec(dC, x, trans=trans, engine=eng)   # ... and of its result
    dA.symmetry = "S"
    dbcsr_multivec(dA, x, engine=eng)   # (both passes: the per-column lists are built in the algebra's own buffers)
    dA.symmetry = "N"
    assert (dA.index_stamp(), dC.index_stamp()) == stamps
    assert all(a is b for m, t in zip((dA, dC), tensors) for a, b in zip((m.row_p, m.col_i, m.blk_p, m.data), t))
    dbcsr_multiply("N", "N", 1.0, dA, dB, 0.0, dC, engine=eng)
    assert eng.plan_stats() == (1, 1), "a multiply after matrix times vectors must reuse its plan"
    torch.cuda.synchronize()
    assert same_bits(dev_to_bcsr(dA).data, A.data)
    product_bar(dev_to_bcsr(dC), 1.0, dense(A), dense(B))


# ---- 8. end to end -------------------------------------------------------------------------------------------------------------------------------------
def test_subspace_iteration_on_the_device(eng):
    """five steps X <- A X, every column normalised, with 5 vectors on the 'S' triangle: dbcsr_multivec and torch only; the same steps in numpy on the
    desymmetrized dense matrix.  The project's 1e-10 by maximum element (the columns have unit norm)."""
    M, F, _, _ = host_matrix("symmetric", "float64", "S")
    D = F.astype(np.float64)
    dM = to_dev(M)
    dM.symmetry = "S"
    n = full_len(M.row_sizes)
    X = np.abs(random_vectors(n, 5, np.float64, 55))
    X /= np.linalg.norm(X, axis=0)
    dX = torch.as_tensor(X.copy()).cuda()
    dY = torch.empty_like(dX)
    for _ in range(5):
        Y = D @ X
        X = Y / np.linalg.norm(Y, axis=0)
        dbcsr_multivec(dM, dX, dY, engine=eng)
        torch.div(dY, torch.linalg.vector_norm(dY, dim=0), out=dX)
    torch.cuda.synchronize()
    err = float(np.max(np.abs(dX.cpu().numpy() - X)))
    print("subspace iteration: max element error %.3e" % err)
    assert err <= 1e-10


def test_on_a_stream_of_its_own(eng):
    M, *parts = host_matrix("mixed", "float64", "N")
    dM = to_dev(M)
    n_x, n_y = lengths(M, "N")
    x = random_vectors(n_x, 17, np.float64, 56)
    dx = torch.as_tensor(x.copy()).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        out = dbcsr_multivec(dM, dx, alpha=-1.3, trans="N", engine=eng, stream=s)
    s.synchronize()
    ref, bar = reference_columns(tuple(parts), "N", -1.3, 0.0, x, None)
    within_columns(out.cpu().numpy(), ref, bar, "on a stream of its own")
    again = dbcsr_multivec(dM, dx, alpha=-1.3, trans="N", engine=eng)
    torch.cuda.synchronize()
    assert same_bits(again.cpu().numpy(), out.cpu().numpy())
