"""The rank-k update on the stored pattern, A_IJ <- beta A_IJ + alpha X_I op(Y_J) for every stored block (dbcsr_amd/operations.py: dbcsr_rank_update;
dbcsr_amd_bcsr_rank_update of include/dbcsr_amd_mm.h; kernels algebra_rank_update_blocks / _scale of dbcsr_amd/csrc/mm_rank_update.h) for float64,
float32 and complex128.

Reference and bar, per stored element, in numpy long double (complex long double) on the dense scatter:
    ref = beta a_ij + alpha sum_v x_iv op(y_jv)           w = |beta| |a_ij| + |alpha| sum_v |x_iv| |y_jv|
    bar = (nrhs + c) 2^-53 w + nrhs eps_ld w              c = 6 for real data, 12 for complex data; + 2^-24 |ref| for float32
The constants are those tests/test_gpu_matvec.py derives for ANY order of summation, with the nrhs terms of the sum in place of the row's elements: one
rounding per product (none for float32 data), nrhs - 1 for the sum, three for alpha s + beta a, two for the second-order terms; a complex product is
within 3 u of the product of the moduli, and there are three of them.  nrhs eps_ld w is the reference's own error.  Nothing is compared against the
code's own output except the bits of a second call.

The kernel stages no chunk of nrhs (every lane walks its row of X and of Y from global memory, 16 summed indices per step, complex data 8), so the one
long sum is nrhs = 520.  Matrices: those of tests/test_gpu_matrix_norms.py (blocks of 1, 3, 4, 5, 7, 13, 23, 32, 67, 70, empty block rows and columns,
rectangular blocks) and `tiles` (blocks of 16, 32, 33 and 80: exact tiles of the 16 x 16 MFMA, one element over, five tiles)."""
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
from dbcsr_amd.operations import dbcsr_dot, dbcsr_multivec, dbcsr_rank_update
from oracle import oracle as O
from tests import far_arena as FA
from tests.gpu_util import dev_to_bcsr, to_dev
from tests.test_gpu_matrix_norms import (base, dense, hole_positions, misaligned, pattern_mask, random_vector, same_bits, subset, symmetric_base, typed,  # noqa: F401
                                         with_holes)
from tests.test_gpu_matvec import EPS_LD, U53, scalars, scaled_in_own_precision, within
from tests.test_gpu_multivec import Dev, random_vectors

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32, np.complex128]
IDS = ["fp64", "fp32", "z64"]
TORCH = {np.dtype(np.float64): torch.float64, np.dtype(np.float32): torch.float32, np.dtype(np.complex128): torch.complex128}
MATRICES = ["mixed", "tiny", "tall70", "tall67", "gappy", "tiles"]
NRHS = [1, 3, 4, 5, 16, 17, 37, 131]
LONG_NRHS = 520   # (no staged chunk of nrhs: the issue's default)
TILE_SIZES = (16, 32, 33, 80)


@pytest.fixture(scope="module")
def eng():
    return MultiplyEngine()


# ---- host helpers (tests/test_rank_update_cpu.py checks them without a GPU) ------------------------------------------------------------------------------
def is_complex(dtype):
    return np.dtype(dtype).kind == "c"


def wide(dtype):
    return np.clongdouble if is_complex(dtype) else np.longdouble


@functools.lru_cache(maxsize=None)
def tiles():
    """Ten block rows and columns of the sizes 16, 32, 33, 80, 16, 32, 33, 80, 16, 32 (322 + 48 full rows), half of the blocks stored: every size is the
    row count of a stored block and the column count of one; a block of 80 x 80 (five tiles by five), one of 33 rows and one of 33 columns (one element
    over two tiles), one of 16 x 16 and one of 32 x 32 (exact tiles) are stored, and so are rectangular blocks."""
    sizes = O.make_block_sizes(370, [1, 16, 1, 32, 1, 33, 1, 80])
    return O.make_random_matrix(sizes, sizes, 0.5, O.RANDMAT_SEED_INIT + 61)


def matrix(which):
    return tiles() if which == "tiles" else base(which)


def parts_of(M):
    """(the dense scatter in long double, its moduli in float64, the pattern of stored elements)"""
    F = dense(M)
    return F.astype(wide(M.data.dtype)), np.abs(F).astype(np.float64), pattern_mask(M)


@functools.lru_cache(maxsize=None)
def host_matrix(which, dtype_name):
    M = typed(matrix(which), np.dtype(dtype_name), 1)
    return (M,) + parts_of(M)


def inputs(M, nrhs, seed=61):
    """X (full rows x nrhs) and Y (full columns x nrhs) of the matrix' data type"""
    dtype = M.data.dtype
    return random_vectors(int(M.row_sizes.sum()), nrhs, dtype, seed), random_vectors(int(M.col_sizes.sum()), nrhs, dtype, seed + 1)


def op_rows(y, trans):
    return y.conj() if trans == "C" and is_complex(y.dtype) else y


def reference(F, absF, alpha, beta, x, y, trans):
    """(ref in long double, bar in float64) for every element of the dense matrix; beta == 0: F is not looked at"""
    dtype, nrhs, W = x.dtype, x.shape[1], wide(x.dtype)
    ref = alpha * (x.astype(W) @ op_rows(y, trans).astype(W).T)
    w = abs(alpha) * (np.abs(x).astype(np.float64) @ np.abs(y).astype(np.float64).T)
    if beta != 0:
        ref = ref + beta * F
        w = w + abs(beta) * absF
    bar = (nrhs + (12 if is_complex(dtype) else 6)) * U53 * w + nrhs * EPS_LD * w
    if dtype == np.float32:
        bar = bar + 2.0 ** -24 * np.abs(ref).astype(np.float64)
    return ref, bar


def in_double(M, alpha, beta, x, y, trans):
    """the same update block by block in float64 / complex128 (np.einsum), rounded to the data's type once: the data area of the result"""
    out = M.data.copy()
    ro, co = np.concatenate([[0], np.cumsum(M.row_sizes)]), np.concatenate([[0], np.cumsum(M.col_sizes)])
    rows = M.rows()
    D = np.complex128 if is_complex(M.data.dtype) else np.float64
    xs, ys = x.astype(D), op_rows(y, trans).astype(D)
    for b in range(M.nblks):
        r, c = int(rows[b]), int(M.col_i[b])
        m, n = int(M.row_sizes[r]), int(M.col_sizes[c])
        s = np.einsum("iv,jv->ij", xs[ro[r]:ro[r + 1]], ys[co[c]:co[c + 1]])
        a = M.data[M.blk_p[b]:M.blk_p[b] + m * n].astype(D).reshape(n, m).T
        out[M.blk_p[b]:M.blk_p[b] + m * n] = (alpha * s + beta * a).T.reshape(-1).astype(M.data.dtype)
    return out


def with_data(M, data):
    return O.Bcsr(M.row_sizes, M.col_sizes, M.row_p, M.col_i, M.blk_p, data)


def stored_within(got_data, M, ref, bar, mask, what):
    within(dense(with_data(M, got_data))[mask], ref[mask], bar[mask], what)


# ---- device helpers -------------------------------------------------------------------------------------------------------------------------------------
def check_update(eng, M, dM, parts, trans, nrhs, view=False, alpha=None, beta=None, y_is_x=False, seed=61):
    """one update with general scalars against the reference; the same bits from a second call on the same A; X and Y unchanged bit for bit; their
    canaries kept.  Leaves dM's data as it found it."""
    F, absF, mask = parts
    dtype = M.data.dtype
    if alpha is None:
        alpha, beta = scalars(dtype)
    x, y = inputs(M, nrhs, seed)
    dx = Dev(x, view)
    dy = None if y_is_x else Dev(y, view)
    before = dM.data.clone()
    assert dbcsr_rank_update(dM, dx.t, None if y_is_x else dy.t, alpha, beta, trans, engine=eng) is None
    torch.cuda.synchronize()
    got = dM.data.cpu().numpy()
    ref, bar = reference(F, absF, alpha, beta, x, x if y_is_x else y, trans)
    stored_within(got, M, ref, bar, mask, "rank update %s, nrhs %d%s" % (trans, nrhs, ", views" if view else ""))
    dM.data.copy_(before)
    dbcsr_rank_update(dM, dx.t, None if y_is_x else dy.t, alpha, beta, trans, engine=eng)
    torch.cuda.synchronize()
    assert same_bits(dM.data.cpu().numpy(), got), "the same bits on every call"
    assert same_bits(dx.host(), x) and dx.canaries_kept()
    assert y_is_x or (same_bits(dy.host(), y) and dy.canaries_kept())
    dM.data.copy_(before)
    return got


def c_update(eng, dM, trans, alpha, beta, nrhs, x, n_x, ldx, y, n_y, ldy, code=None):
    d = dM.desc()
    return eng.L.dbcsr_amd_bcsr_rank_update(eng.h, dM.dtype_code if code is None else code, trans.encode(), _z(alpha), nrhs,
                                            x.data_ptr() if x is not None else None, n_x, ldx, y.data_ptr() if y is not None else None, n_y, ldy,
                                            _z(beta), C.byref(d), StreamHandle().ptr)


# ---- 1. every matrix, type and nrhs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trans", ["T", "C"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("which", MATRICES)
def test_rank_update(eng, which, dtype, trans):
    M, *parts = host_matrix(which, np.dtype(dtype).name)
    dM = to_dev(M)
    for nrhs in NRHS:
        check_update(eng, M, dM, tuple(parts), trans, nrhs)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_long_sum(eng, dtype):
    """nrhs = 520: the kernel stages no chunk of nrhs, a lane takes 4 (complex data: 2) consecutive indices per step of 16 (8) -- 32 (65) steps"""
    M, *parts = host_matrix("mixed", np.dtype(dtype).name)
    check_update(eng, M, to_dev(M), tuple(parts), "C", LONG_NRHS)


# ---- 2. views ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("which", MATRICES)
def test_views_and_a_misaligned_data_area(eng, which, dtype):
    """X and Y with ld = nrhs + 3 one element into an allocation of canaries, A's data area one element into its allocation"""
    M, *parts = host_matrix(which, np.dtype(dtype).name)
    dM = misaligned(to_dev(M))
    for trans in ("T", "C"):
        for nrhs in (3, 17, 37):
            check_update(eng, M, dM, tuple(parts), trans, nrhs, view=True)


# ---- 3. an operand with holes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_an_operand_with_holes(eng, dtype):
    hB, dB = with_holes(eng, typed(base("mixed"), dtype, 1), dtype)
    holes = hole_positions(hB)
    assert holes.size > 0
    before = dB.data.cpu().numpy()
    index = (dB.row_p, dB.col_i, dB.blk_p)
    copies = [t.clone() for t in index]
    stamp = dB.index_stamp()
    alpha, beta = scalars(dtype)
    x, y = inputs(hB, 17)
    dbcsr_rank_update(dB, Dev(x).t, Dev(y).t, alpha, beta, "C", engine=eng)
    torch.cuda.synchronize()
    got = dB.data.cpu().numpy()
    F, absF, mask = parts_of(hB)
    ref, bar = reference(F, absF, alpha, beta, x, y, "C")
    stored_within(got, hB, ref, bar, mask, "an operand with holes")
    assert same_bits(got[holes], before[holes]), "the holes keep their bits"
    assert dB.index_stamp() == stamp and all(a is b for a, b in zip((dB.row_p, dB.col_i, dB.blk_p), index))
    assert all(torch.equal(a, b) for a, b in zip(index, copies))


# ---- 4. zeros are true zeros ------------------------------------------------------------------------------------------------------------------------------
def blocks_of_line(M, line, axis):
    """mask of the dense matrix: the stored elements of block row (axis 0) / block column (axis 1) `line`"""
    off = np.concatenate([[0], np.cumsum(M.row_sizes if axis == 0 else M.col_sizes)])
    m = np.zeros_like(pattern_mask(M))
    if axis == 0:
        m[off[line]:off[line + 1], :] = True
    else:
        m[:, off[line]:off[line + 1]] = True
    return m & pattern_mask(M), off


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("axis", [0, 1], ids=["X_rows", "Y_rows"])
def test_rows_of_the_neighbouring_block_never_enter(eng, dtype, axis):
    """(a) X holds NaN in every row of block row I + 1: every block of block row I is finite and within the bar -- for a block row of 13 rows followed
    by one of 5, and for the last block row, behind which the tensor ends.  (b) the same for Y and block columns (23 columns followed by 4)."""
    M, F, absF, _ = host_matrix("mixed", np.dtype(dtype).name)
    sizes = M.row_sizes if axis == 0 else M.col_sizes
    nb = len(sizes)
    first = next(i for i in range(nb - 1) if sizes[i] == (13 if axis == 0 else 23) and sizes[i + 1] == (5 if axis == 0 else 4)
                 and blocks_of_line(M, i, axis)[0].any())
    alpha, beta = scalars(dtype)
    dM = to_dev(M)
    before = dM.data.clone()
    for line in (first, nb - 1):
        mask, off = blocks_of_line(M, line, axis)
        assert mask.any()
        for nrhs in (5, 17):
            x, y = inputs(M, nrhs)
            poisoned = (x if axis == 0 else y).copy()
            if line + 1 < nb:
                poisoned[off[line + 1]:off[line + 2]] = np.nan
            dx, dy = Dev(poisoned if axis == 0 else x), Dev(poisoned if axis == 1 else y)
            dM.data.copy_(before)
            dbcsr_rank_update(dM, dx.t, dy.t, alpha, beta, "C", engine=eng)
            torch.cuda.synchronize()
            got = dM.data.cpu().numpy()
            G = dense(with_data(M, got))
            assert np.all(np.isfinite(G[mask])), "a row of the neighbouring block entered the product"
            ref, bar = reference(F, absF, alpha, beta, x, y, "C")
            within(G[mask], ref[mask], bar[mask], "line %d of axis %d, nrhs %d" % (line, axis, nrhs))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_padding_columns_never_enter(eng, dtype):
    """(c) nrhs = 5 in a view with ld = 8 whose padding columns, and the elements around it, hold NaN"""
    M, *parts = host_matrix("mixed", np.dtype(dtype).name)
    F, absF, mask = parts
    alpha, beta = scalars(dtype)
    x, y = inputs(M, 5)

    def nan_view(a):
        n = a.shape[0]
        big = torch.full((1 + n * 8 + 2,), float("nan"), dtype=TORCH[a.dtype], device="cuda")
        t = big[1:1 + n * 8].view(n, 8)[:, :5]
        t.copy_(torch.as_tensor(a))
        return t

    dM = to_dev(M)
    dbcsr_rank_update(dM, nan_view(x), nan_view(y), alpha, beta, "C", engine=eng)
    torch.cuda.synchronize()
    got = dM.data.cpu().numpy()
    assert np.all(np.isfinite(got.view(np.float64 if is_complex(dtype) else got.dtype)))
    ref, bar = reference(F, absF, alpha, beta, x, y, "C")
    stored_within(got, M, ref, bar, mask, "NaN in the padding columns")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("nrhs", [5, 6])
def test_an_aligned_column_slice_of_a_wider_basis(eng, dtype, nrhs):
    """basis[:, :nrhs] of an aligned (n, 8) allocation (a fresh torch allocation is 16-byte aligned, and ld = 8 elements is a multiple of 16 bytes in
    every type): the rows are read with 16-byte loads up to the last whole run and element by element behind it -- the one combination of the kernel's
    two load forms that neither a contiguous tensor with such an nrhs nor a view one element into its allocation reaches.  The padding columns hold NaN."""
    M, F, absF, mask = host_matrix("mixed", np.dtype(dtype).name)
    alpha, beta = scalars(dtype)
    x, y = inputs(M, nrhs)

    def slice_of(a):
        basis = torch.full((a.shape[0], 8), float("nan"), dtype=TORCH[a.dtype], device="cuda")
        assert basis.data_ptr() % 16 == 0
        basis[:, :nrhs].copy_(torch.as_tensor(a))
        return basis[:, :nrhs]

    dM = to_dev(M)
    dbcsr_rank_update(dM, slice_of(x), slice_of(y), alpha, beta, "C", engine=eng)
    torch.cuda.synchronize()
    got = dM.data.cpu().numpy()
    assert np.all(np.isfinite(got.view(np.float64 if is_complex(dtype) else got.dtype)))
    ref, bar = reference(F, absF, alpha, beta, x, y, "C")
    stored_within(got, M, ref, bar, mask, "an aligned slice with ld = 8, nrhs %d" % nrhs)


# ---- 5. scalars -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_special_scalars(eng, dtype):
    M, F, absF, mask = host_matrix("mixed", np.dtype(dtype).name)
    alpha, beta = scalars(dtype)
    tdt = TORCH[np.dtype(dtype)]
    x, y = inputs(M, 17)
    dx, dy = Dev(x), Dev(y)
    dM = to_dev(M)
    # beta == 0: A's values are not read
    dM.data.fill_(float("nan"))
    dbcsr_rank_update(dM, dx.t, dy.t, alpha, 0.0, "C", engine=eng)
    torch.cuda.synchronize()
    got = dM.data.cpu().numpy()
    assert np.all(np.isfinite(got.view(np.float64 if is_complex(dtype) else got.dtype)))
    ref, bar = reference(F, absF, alpha, 0.0, x, y, "C")
    stored_within(got, M, ref, bar, mask, "beta == 0")
    # alpha == 0: X and Y are not read, A <- beta A in the data's own precision
    xn = torch.full(x.shape, float("nan"), dtype=tdt, device="cuda")
    yn = torch.full(y.shape, float("nan"), dtype=tdt, device="cuda")
    dM.data.copy_(torch.as_tensor(M.data))
    dbcsr_rank_update(dM, xn, yn, 0.0, beta, "C", engine=eng)
    torch.cuda.synchronize()
    assert same_bits(dM.data.cpu().numpy(), scaled_in_own_precision(beta, M.data).astype(dtype)), "alpha == 0: beta A, bit for bit"
    # alpha == 0 and beta == 1: A keeps its bits
    dM.data.copy_(torch.as_tensor(M.data))
    dbcsr_rank_update(dM, xn, yn, 0.0, 1.0, "C", engine=eng)
    torch.cuda.synchronize()
    assert same_bits(dM.data.cpu().numpy(), M.data)
    # nrhs == 0: as alpha == 0
    dbcsr_rank_update(dM, xn[:, :0], yn[:, :0], alpha, beta, "C", engine=eng)
    torch.cuda.synchronize()
    assert same_bits(dM.data.cpu().numpy(), scaled_in_own_precision(beta, M.data).astype(dtype)), "nrhs == 0: beta A, bit for bit"
    # both zero: zeros
    dbcsr_rank_update(dM, xn, yn, 0.0, 0.0, "C", engine=eng)
    torch.cuda.synchronize()
    assert not np.any(dM.data.cpu().numpy())


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
def test_plain_accumulation_of_x_x_transposed(eng, dtype):
    """beta = 1, alpha = 1, Y = X (vecs_y=None) on real data"""
    M = typed(base("square"), dtype, 1)
    check_update(eng, M, to_dev(M), parts_of(M), "T", 17, alpha=1.0, beta=1.0, y_is_x=True)


# ---- 6. symmetry ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,symmetry", [(np.float64, "S"), (np.float32, "S"), (np.complex128, "H")], ids=["fp64_S", "fp32_S", "z64_H"])
def test_stored_triangle(eng, dtype, symmetry):
    """the stored triangle is updated block by block against X X^T / X X^H: the update of the full symmetric / hermitian matrix"""
    M = typed(symmetric_base(symmetry), dtype, 3)
    dM = to_dev(M)
    dM.symmetry = symmetry
    trans = "C" if symmetry == "H" else "T"
    for nrhs in (5, 37):
        check_update(eng, M, dM, parts_of(M), trans, nrhs, alpha=-1.3, beta=0.6, y_is_x=True)


class Poisoned:
    """an engine that must not be used: any attribute access raises"""

    def __getattr__(self, name):
        raise AssertionError("the engine was used (%s)" % name)


def test_refusals_come_before_any_call(monkeypatch):
    bad = Poisoned()
    monkeypatch.setattr(OPS, "default_engine", lambda: bad)   # (and no engine of its own is made either)
    A = base("mixed")
    dA = to_dev(A)
    rows, cols = int(A.row_sizes.sum()), int(A.col_sizes.sum())
    x = torch.ones((rows, 3), dtype=torch.float64, device="cuda")
    y = torch.ones((cols, 3), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):
        dbcsr_rank_update(dA, y, x, engine=bad)   # the columns' length for the rows
    with pytest.raises(ValueError):
        dbcsr_rank_update(dA, x, y[:-1].contiguous(), engine=bad)
    with pytest.raises(ValueError):
        dbcsr_rank_update(dA, x, y[:, :2].contiguous(), engine=bad)   # another nrhs
    with pytest.raises(ValueError):
        dbcsr_rank_update(dA, x, engine=bad)   # Y = X needs equal row and column block sizes
    with pytest.raises(ValueError):
        dbcsr_rank_update(dA, x[:, 0], y[:, 0], engine=bad)   # 1-D
    with pytest.raises(TypeError):
        dbcsr_rank_update(dA, x.float(), y, engine=bad)
    with pytest.raises(TypeError):
        dbcsr_rank_update(dA, x, y.to(torch.complex128), engine=bad)
    with pytest.raises(TypeError):
        dbcsr_rank_update(dA, np.ones((rows, 3)), y, engine=bad)
    with pytest.raises(ValueError):
        dbcsr_rank_update(dA, x.cpu(), y, engine=bad)
    with pytest.raises(ValueError):
        dbcsr_rank_update(dA, torch.ones((rows, 6), dtype=torch.float64, device="cuda")[:, ::2], y, engine=bad)   # stride(1) != 1
    with pytest.raises(ValueError):
        dbcsr_rank_update(dA, torch.ones(3 * rows, dtype=torch.float64, device="cuda").as_strided((rows, 3), (2, 1)), y, engine=bad)   # stride(0) < nrhs
    for trans in ("N", "t", "", None):
        with pytest.raises(ValueError):
            dbcsr_rank_update(dA, x, y, trans=trans, engine=bad)
    with pytest.raises(TypeError):
        dbcsr_rank_update(dA, x, y, alpha=1j, engine=bad)
    with pytest.raises(TypeError):
        dbcsr_rank_update(dA, x, y, beta=0.5 + 0j, engine=bad)
    with pytest.raises(ValueError):
        dbcsr_rank_update(dA, x, y, trans="N")   # (a refusal does not ask for the default engine either)
    # X or Y inside the matrix' data area
    n = dA.data.numel()
    assert n >= 3 * max(rows, cols)
    with pytest.raises(ValueError):
        dbcsr_rank_update(dA, dA.data[:3 * rows].view(rows, 3), y, engine=bad)
    with pytest.raises(ValueError):
        dbcsr_rank_update(dA, x, dA.data[n - 3 * cols:].view(cols, 3), engine=bad)
    # symmetry
    S = symmetric_base("S")
    ns = int(S.row_sizes.sum())
    xs, ys = torch.ones((ns, 3), dtype=torch.float64, device="cuda"), torch.ones((ns, 3), dtype=torch.float64, device="cuda")
    dS = to_dev(S)
    for sym in ("A", "K", "X"):
        dS.symmetry = sym
        with pytest.raises(ValueError):
            dbcsr_rank_update(dS, xs, engine=bad)
    dS.symmetry = "S"
    with pytest.raises(ValueError):
        dbcsr_rank_update(dS, xs, ys, engine=bad)   # X Y^T is not symmetric
    with pytest.raises(ValueError):
        dbcsr_rank_update(dS, xs, xs, engine=bad)   # (not even when it is the same tensor: vecs_y=None says so)
    dS.symmetry = "H"   # real data: 'S'
    with pytest.raises(ValueError):
        dbcsr_rank_update(dS, xs, engine=bad)
    dH = to_dev(typed(S, np.complex128, 3))
    dH.symmetry = "H"
    zs = torch.ones((ns, 3), dtype=torch.complex128, device="cuda")
    with pytest.raises(ValueError):
        dbcsr_rank_update(dH, zs, trans="T", engine=bad)   # X X^T is not hermitian
    with pytest.raises(ValueError):
        dbcsr_rank_update(dH, zs, alpha=0.7 - 0.4j, trans="C", engine=bad)
    with pytest.raises(ValueError):
        dbcsr_rank_update(dH, zs, beta=0.7j, trans="C", engine=bad)
    with pytest.raises(ValueError):
        dbcsr_rank_update(dH, zs, zs.clone(), trans="C", engine=bad)
    tri = to_dev(typed(base("mixed"), np.float64, 1))
    tri.symmetry = "S"
    with pytest.raises(ValueError):
        dbcsr_rank_update(tri, x, engine=bad)   # a matrix with symmetry that is not square
    torch.cuda.synchronize()
    assert same_bits(dA.data.cpu().numpy(), A.data) and same_bits(dS.data.cpu().numpy(), S.data)
    assert dbcsr_amd.dbcsr_rank_update is dbcsr_rank_update and "dbcsr_rank_update" in dbcsr_amd.__all__


# ---- 7. the two halves agree with the mathematics ------------------------------------------------------------------------------------------------------------
def pattern_sum(M, x):
    """(sum over the stored elements of a_ij (conj(X) X^T)_ij in long double, sum |a_ij| sum_v |x_iv| |x_jv|): for real data sum a_ij (X X^T)_ij"""
    F, absF, mask = parts_of(M)
    W = wide(M.data.dtype)
    G = x.conj().astype(W) @ x.astype(W).T
    absG = np.abs(x).astype(np.float64) @ np.abs(x).astype(np.float64).T
    return (F * G)[mask].sum(), float((absF * absG)[mask].sum()), int(mask.sum())


@pytest.mark.parametrize("dtype", [np.float64, np.complex128], ids=["fp64", "z64"])
def test_the_two_halves_agree(eng, dtype):
    """P = A's pattern filled with X X^H by dbcsr_rank_update(beta = 0, alpha = 1, X, None, trans "C"); for real data that is X X^T.  Then
    sum_pattern a_ij conj(p_ij) = sum_iv conj(x_iv) (A X)_iv -- for real data sum_pattern a_ij (X X^T)_ij = dbcsr_dot(A, P) = sum X o dbcsr_multivec(A, X) --
    and each side lies within (elements + nrhs + 12) 2^-53 sum |a| |x| |x| of that sum formed in long double from the inputs.  (For complex data
    conj(X) X^T = conj(X X^H) is the matrix for which the identity holds; the complex dot is not offered, so that side is summed here, in long double,
    from the P the device made.)"""
    M = typed(base("square"), dtype, 1)
    nrhs = 17
    x = random_vectors(int(M.row_sizes.sum()), nrhs, dtype, 71)
    ref, scale, elements = pattern_sum(M, x)
    bar = (elements + nrhs + 12) * U53 * scale
    dA, dP, dx = to_dev(M), to_dev(M), Dev(x)
    dP.data.fill_(float("nan"))
    dbcsr_rank_update(dP, dx.t, None, 1.0, 0.0, "C", engine=eng)
    ax = dbcsr_multivec(dA, dx.t, engine=eng)
    torch.cuda.synchronize()
    W = wide(dtype)
    p = dP.data.cpu().numpy()
    sides = {"sum a conj(p)": (M.data.astype(W) * p.conj().astype(W)).sum(), "sum conj(X) o (A X)": (x.conj().astype(W) * ax.cpu().numpy().astype(W)).sum()}
    if not is_complex(dtype):
        sides["dbcsr_dot(A, P)"] = dbcsr_dot(dA, dP, engine=eng)
    for what, got in sides.items():
        err = float(abs(W(got) - ref))
        print("%s: error %.3e against a bar of %.3e" % (what, err, bar))
        assert err <= bar, what


# ---- 8. plans stay ------------------------------------------------------------------------------------------------------------------------------------------
def test_rank_update_between_multiplies_keeps_the_plan(monkeypatch):
    monkeypatch.delenv("DBCSR_AMD_MM_PLAN", raising=False)
    eng = MultiplyEngine()
    sizes = O.make_block_sizes(200, [1, 13, 1, 5, 1, 7])
    A = typed(O.make_random_matrix(sizes, sizes, 0.5, O.RANDMAT_SEED_INIT + 31), np.float64, 5)
    B = typed(O.make_random_matrix(sizes, sizes, 0.6, O.RANDMAT_SEED_INIT + 32), np.float64, 6)
    dA, dB = to_dev(A), to_dev(B)
    dC = to_dev(subset(A, lambda r, c: False))
    dbcsr_multiply("N", "N", 1.0, dA, dB, 0.0, dC, engine=eng)
    assert eng.plan_stats() == (0, 1)
    x, y = inputs(A, 17)
    tensors = (dA.row_p, dA.col_i, dA.blk_p, dA.data)
    stamp = dA.index_stamp()
    dbcsr_rank_update(dA, Dev(x).t, Dev(y).t, -1.3, 0.6, engine=eng)
    assert dA.index_stamp() == stamp and all(a is b for a, b in zip((dA.row_p, dA.col_i, dA.blk_p, dA.data), tensors))
    dbcsr_multiply("N", "N", 1.0, dA, dB, 0.0, dC, engine=eng)
    assert eng.plan_stats() == (1, 1), "a multiply after a rank update of its operand must reuse its plan"
    torch.cuda.synchronize()
    updated = dev_to_bcsr(dA)
    F, absF, mask = parts_of(A)
    ref, bar = reference(F, absF, -1.3, 0.6, x, y, "T")
    stored_within(updated.data, A, ref, bar, mask, "the operand between the multiplies")
    got = dev_to_bcsr(dC)
    R, scale = dense(updated) @ dense(B), np.abs(dense(updated)) @ np.abs(dense(B))
    pm = pattern_mask(got)
    assert np.all(np.abs(dense(got) - R)[pm] <= 1e-10 * scale[pm]) and not np.any(R[~pm])


# ---- 9. C-ABI answers -------------------------------------------------------------------------------------------------------------------------------------
CANARY = -77.25


def test_c_abi_answers(eng):
    Sq = typed(base("square"), np.float64, 1)
    n = int(Sq.row_sizes.sum())
    k = 3
    dS = to_dev(Sq)
    dS.data.fill_(CANARY)
    big = torch.full((2 * n * k,), CANARY, dtype=torch.float64, device="cuda")
    x, y = big[:n * k].view(n, k), big[n * k:].view(n, k)
    for code in (L.dbcsr_type_complex_4, 2, 99):
        assert c_update(eng, dS, "T", 1.0, 1.0, k, x, n, k, y, n, k, code=code) == -10
    assert c_update(eng, dS, "T", 1.0, 1.0, k, None, n, k, y, n, k) == -1
    assert c_update(eng, dS, "T", 1.0, 1.0, k, x, n, k, None, n, k) == -1
    d = dS.desc()
    st = StreamHandle().ptr
    f64 = L.dbcsr_type_real_8
    call = eng.L.dbcsr_amd_bcsr_rank_update
    assert call(None, f64, b"T", _z(1.0), k, x.data_ptr(), n, k, y.data_ptr(), n, k, _z(1.0), C.byref(d), st) == -1
    assert call(eng.h, f64, b"T", None, k, x.data_ptr(), n, k, y.data_ptr(), n, k, _z(1.0), C.byref(d), st) == -1
    assert call(eng.h, f64, b"T", _z(1.0), k, x.data_ptr(), n, k, y.data_ptr(), n, k, None, C.byref(d), st) == -1
    assert call(eng.h, f64, b"T", _z(1.0), k, x.data_ptr(), n, k, y.data_ptr(), n, k, _z(1.0), None, st) == -1
    for trans in ("N", "X", "t"):
        assert c_update(eng, dS, trans, 1.0, 1.0, k, x, n, k, y, n, k) == -1
    assert c_update(eng, dS, "T", 1.0, 1.0, -1, x, n, k, y, n, k) == -1      # nrhs < 0
    assert c_update(eng, dS, "T", 1.0, 1.0, k, x, n, k - 1, y, n, k) == -1   # ldx < nrhs
    assert c_update(eng, dS, "T", 1.0, 1.0, k, x, n, k, y, n, k - 1) == -1   # ldy < nrhs
    assert c_update(eng, dS, "T", 1.0, 1.0, k, x, -1, k, y, n, k) == -1
    assert c_update(eng, dS, "T", 1.0, 1.0, k, x, n, k, y, -1, k) == -1
    # an empty matrix: 0, nothing written (nor read: null tensors are not asked about)
    dE = to_dev(subset(Sq, lambda r, c: False))
    assert c_update(eng, dE, "T", 1.0, 0.5, k, x, n, k, y, n, k) == 0
    # alpha == 0 and beta == 1: 0, nothing launched; null tensors are legal where they would not be read
    assert c_update(eng, dS, "T", 0.0, 1.0, k, None, n, k, None, n, k) == 0
    assert c_update(eng, dS, "T", 1.0, 1.0, 0, None, n, 0, None, n, 0) == 0
    torch.cuda.synchronize()
    assert not np.any(big.cpu().numpy() != CANARY) and not np.any(dS.data.cpu().numpy() != CANARY), "a refusal wrote something"
    # y == x is legal
    dS.data.copy_(torch.as_tensor(Sq.data))
    xv = random_vectors(n, k, np.float64, 81)
    dx = Dev(xv, True)
    assert c_update(eng, dS, "T", -1.3, 0.6, k, dx.t, n, dx.ld, dx.t, n, dx.ld) == 0
    torch.cuda.synchronize()
    F, absF, mask = parts_of(Sq)
    ref, bar = reference(F, absF, -1.3, 0.6, xv, xv, "T")
    full = dS.data.cpu().numpy()
    stored_within(full, Sq, ref, bar, mask, "y == x through the C entry")
    assert dx.canaries_kept()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("short", ["n_x", "n_y"])
def test_a_short_tensor_leaves_its_elements_unwritten(eng, dtype, short):
    """n_x (n_y) seven short, the rows behind it full of NaN: the elements of A in those rows (columns) keep their canary, every other stored element
    has the bits of the full call, and nothing else is written"""
    M = typed(base("mixed"), dtype, 1)
    rows, cols = int(M.row_sizes.sum()), int(M.col_sizes.sum())
    alpha, beta = scalars(dtype)
    x, y = inputs(M, 17)
    dM = to_dev(M)
    assert c_update(eng, dM, "C", alpha, beta, 17, Dev(x).t, rows, 17, Dev(y).t, cols, 17) == 0
    torch.cuda.synchronize()
    full = dense(with_data(M, dM.data.cpu().numpy()))
    xs, ys = x.copy(), y.copy()
    (xs if short == "n_x" else ys)[-7:] = np.nan
    dM.data.fill_(CANARY)
    dx, dy = Dev(xs, True), Dev(ys, True)
    assert c_update(eng, dM, "C", alpha, 0.0, 17, dx.t, rows - (7 if short == "n_x" else 0), dx.ld, dy.t, cols - (7 if short == "n_y" else 0), dy.ld) == 0
    dM2 = to_dev(M)
    assert c_update(eng, dM2, "C", alpha, beta, 17, dx.t, rows - (7 if short == "n_x" else 0), dx.ld, dy.t, cols - (7 if short == "n_y" else 0), dy.ld) == 0
    torch.cuda.synchronize()
    mask = pattern_mask(M)
    behind = np.zeros_like(mask)
    if short == "n_x":
        behind[rows - 7:, :] = True
    else:
        behind[:, cols - 7:] = True
    assert (mask & behind).any()
    G = dense(with_data(M, dM.data.cpu().numpy()))
    assert np.all(G[mask & behind] == CANARY), "an element whose row of X / Y lies behind the tensor was written"
    assert not np.any(G[mask & ~behind] == CANARY) and np.all(np.isfinite(G[mask]))
    G2 = dense(with_data(M, dM2.data.cpu().numpy()))
    assert same_bits(G2[mask & ~behind], full[mask & ~behind]) and same_bits(G2[mask & behind], dense(M)[mask & behind])
    assert dx.canaries_kept() and dy.canaries_kept()


# ---- 10. far offsets and special values ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def arena():
    a = FA.arena()
    yield a
    if a is not None:
        a.release()
        del a
    torch.cuda.empty_cache()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_rank_update_of_a_far_matrix(eng, arena, dtype):
    """A's blocks placed around 2^29, 2^31, 2^32, ... elements of one large allocation, one block straddling each boundary (tests/far_arena.py)"""
    from tests.test_gpu_far_offsets import one_far
    M, F, absF, mask = host_matrix("mixed", np.dtype(dtype).name)
    far, dM = one_far(arena, M, dtype, "blocks", who=1 if is_complex(dtype) else 0)
    blk_p = dM.blk_p.cpu().numpy()
    boundary = 2 ** 31 if is_complex(dtype) else 2 ** 32
    assert FA.straddlers(M, blk_p, boundary).size > 0, "a block straddles 2^%d elements" % (31 if is_complex(dtype) else 32)
    alpha, beta = scalars(dtype)
    x, y = inputs(M, 17)
    dx, dy = Dev(x, True), Dev(y, True)
    dbcsr_rank_update(dM, dx.t, dy.t, alpha, beta, "C", engine=eng)
    torch.cuda.synchronize()
    ref, bar = reference(F, absF, alpha, beta, x, y, "C")
    stored_within(FA.blocks_to_host(dM).data, M, ref, bar, mask, "a far matrix")
    assert far.guards_kept() and dx.canaries_kept() and dy.canaries_kept()


def classes(a):
    """0 finite, 1 +Inf, 2 -Inf, 3 NaN per element (a complex element: the pair of its parts)"""
    def one(r):
        return np.where(np.isnan(r), 3, np.where(np.isposinf(r), 1, np.where(np.isneginf(r), 2, 0)))
    a = np.asarray(a)
    return one(a.real) * 4 + one(a.imag) if a.dtype.kind == "c" else one(a)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_special_values_keep_their_class(eng, dtype):
    """X holds +Inf, -Inf and NaN at chosen places (rows of four different block rows, nrhs = 5): the class of every stored element is the
    reference's.  X and Y have no zeros, so an infinity meets no 0; where +Inf and -Inf meet in one sum, and where a complex product subtracts two
    infinities, both sides give NaN -- numpy forms complex products from the four real ones, as the kernel does."""
    M, F, absF, mask = host_matrix("mixed", np.dtype(dtype).name)
    alpha, beta = scalars(dtype)
    x, y = inputs(M, 5)
    ro = np.concatenate([[0], np.cumsum(M.row_sizes)])
    x[ro[1], 0] = np.inf
    x[ro[3] + 2, 2] = -np.inf
    x[ro[5] + 1, 4] = np.nan
    x[ro[7], 1], x[ro[7], 3] = np.inf, -np.inf   # (both in one row: NaN where Y gives them opposite signs)
    dM = to_dev(M)
    dbcsr_rank_update(dM, Dev(x).t, Dev(y).t, alpha, beta, "C", engine=eng)
    torch.cuda.synchronize()
    got = dM.data.cpu().numpy()
    if is_complex(dtype):   # (the parts scattered one by one: 1j * Inf, as dense() forms a complex matrix, is NaN + Inf j)
        G = np.empty(mask.shape, np.complex128)
        G.real, G.imag = dense(with_data(M, np.ascontiguousarray(got.real))), dense(with_data(M, np.ascontiguousarray(got.imag)))
    else:
        G = dense(with_data(M, got))
    with np.errstate(invalid="ignore", over="ignore"):
        ref, _ = reference(F, absF, alpha, beta, x, y, "C")
    want = classes(ref)[mask]
    assert len(set(want.tolist())) >= 4, "finite, infinite of both signs and NaN all occur"
    assert np.array_equal(classes(G)[mask], want)
