"""A block diagonal applied to a matrix in place (dbcsr_amd/operations.py: dbcsr_scale_by_block_diag; dbcsr_amd_bcsr_block_diag_multiply of
include/dbcsr_amd_mm.h; kernels block_scale_left / _right / _zero of dbcsr_amd/csrc/mm_block_scale.h) for float64, float32 and complex128.

Reference and bar, per stored element, in numpy long double (complex long double) on the dense scatter (left shown; right likewise, d then the
dimension of the block column's diagonal block):
    ref = alpha sum_k op(D)_ik a_kj          w = |alpha| sum_k |d_ik| |a_kj|
    bar = (d + c) 2^-53 w + d eps_ld w       c = 6 for real data, 12 for complex data; + 2^-24 |ref| for float32
The constants are those tests/test_gpu_matvec.py derives for a sum of d terms in ANY order: one rounding per product (none for float32 data), d - 1 for
the sum, the scaling by alpha, the rounding to the data's type and the second-order terms; a complex product is within 3 u of the product of the moduli.
d eps_ld w is the reference's own error.  A block row of diag without a diagonal block has ref = w = bar = 0: the result must be zero exactly, and the
tests ask for +0.0 by its bits.  Nothing is compared against the code's own output except the bits of a second call.

side="both" is two passes: T = alpha op(D) A, then T op'(D) with op' = op followed by the conjugate transpose.  The first pass leaves an error of at most
bar_left (its rounding included) in every element of T; the second pass multiplies that error by |op'(D)| -- bar_left @ |op'(D)| -- and adds its own
bar_right(w2), w2 = |T| @ |op'(D)| formed from the exact T (the computed T differs from it by bar_left, a second-order term that the c of the bar covers).
Two-pass bar = bar_right(w2) + bar_left @ |op'(D)|.  A twin element of an expanded stored triangle is the (conjugate) transpose of a stored one -- an
exact operation -- and carries the bar of the element it mirrors.

Matrices: those of tests/test_gpu_matrix_norms.py and `tiles` of tests/test_gpu_rank_update.py, and `edge` (blocks of 15, 16, 17, 33, 64, 96: exact tiles
of the 16 x 16 MFMA, one under, one over, and the largest diagonal block allowed -- six tiles, the accumulator limit)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from dbcsr_amd.matrix import DbcsrMatrix, StreamHandle
from dbcsr_amd.multiply import MultiplyEngine, dbcsr_multiply
from dbcsr_amd.operations import dbcsr_get_block_diag, dbcsr_invert_block_diag, dbcsr_scale_by_block_diag
from oracle import oracle as O
from tests import far_arena as FA
from tests.gpu_util import dev_to_bcsr, to_dev
from tests.test_gpu_matrix_norms import (base, blocks_of, dense, desymmetrized_dense, from_blocks, hole_positions, pattern_mask, same_bits, subset,
                                         symmetric_base, typed, with_holes)
from tests.test_gpu_matvec import EPS_LD, U53, scalars, within
from tests.test_gpu_rank_update import tiles

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32, np.complex128]
IDS = ["fp64", "fp32", "z64"]
MATRICES = ["mixed", "tiny", "gappy", "tall70", "tall67", "tiles", "edge"]
EDGE_SIZES = (15, 16, 17, 33, 64, 96)
CANARY = -77.25
GUARD = 64


@pytest.fixture(scope="module")
def eng():
    return MultiplyEngine()


# ---- host helpers (tests/test_block_scale_cpu.py checks them without a GPU) ----------------------------------------------------------------------------
def is_complex(dtype):
    return np.dtype(dtype).kind == "c"


def wide(dtype):
    return np.clongdouble if is_complex(dtype) else np.longdouble


@functools.lru_cache(maxsize=None)
def edge():
    """Twelve block rows and columns of the sizes 15, 16, 17, 33, 64, 96 (twice), half of the blocks stored: every size is the row count of a stored
    block and the column count of one; a block of 96 x 96 (six tiles by six) is stored, and so are rectangular blocks."""
    sizes = O.make_block_sizes(2 * sum(EDGE_SIZES), [1, 15, 1, 16, 1, 17, 1, 33, 1, 64, 1, 96])
    return O.make_random_matrix(sizes, sizes, 0.5, O.RANDMAT_SEED_INIT + 73)


def matrix(which):
    return tiles() if which == "tiles" else edge() if which == "edge" else base(which)


@functools.lru_cache(maxsize=None)
def host_matrix(which, dtype_name):
    """(the host matrix, its dense scatter in long double, the pattern of stored elements): formed once"""
    M = typed(matrix(which), np.dtype(dtype_name), 1)
    return M, dense(M).astype(wide(M.data.dtype)), pattern_mask(M)


def no_diag_block(r):
    return r % 5 == 3


def uniform(rng, n, cplx):
    x = rng.uniform(-1.0, 1.0, n)
    return x + 1j * rng.uniform(-1.0, 1.0, n) if cplx else x


def diag_blocks(sizes, dtype, seed=5):
    """{(r, c): data} of a square matrix on `sizes`: a random diagonal block in every block row but those of no_diag_block, and a few blocks off the
    diagonal, which must be ignored"""
    rng = np.random.default_rng([seed, len(sizes), int(is_complex(dtype))])
    n = len(sizes)
    blocks = {}
    for r in range(n):
        if not no_diag_block(r):
            blocks[(r, r)] = uniform(rng, int(sizes[r]) ** 2, is_complex(dtype)).astype(dtype)
        if r % 4 == 0 and n > 1:
            c = (r + 1) % n
            blocks[(r, c)] = uniform(rng, int(sizes[r]) * int(sizes[c]), is_complex(dtype)).astype(dtype)
    return blocks


@functools.lru_cache(maxsize=None)
def _diag_for(key, dtype_name):
    sizes = np.frombuffer(key, np.int32)
    return from_blocks(sizes, sizes, diag_blocks(sizes, np.dtype(dtype_name)), np.dtype(dtype_name))


def diag_for(M, side, dtype):
    """the square operand on M's row block sizes (left) or column block sizes (right)"""
    sizes = np.ascontiguousarray(M.row_sizes if side == "left" else M.col_sizes, np.int32)
    return _diag_for(sizes.tobytes(), np.dtype(dtype).name)


def op_of(B, trans):
    """op of a block-diagonal dense matrix ('J': the conjugate alone)"""
    return B if trans == "N" else B.T if trans == "T" else B.conj().T if trans == "C" else B.conj()


def dagger(trans, dtype):
    """op' = op followed by the conjugate transpose (real data: the transpose)"""
    if is_complex(dtype):
        return {"N": "C", "C": "N", "T": "J"}[trans]
    return "T" if trans == "N" else "N"


def blockdiag_dense(D, trans):
    """op(blockdiag(D)) in long double, its moduli in float64, and the dimension of the diagonal block of every full row (0: none stored)"""
    only = subset(D, lambda r, c: r == c)
    B = op_of(dense(only).astype(wide(D.data.dtype)), trans)
    dims = np.concatenate([np.full(int(n), 0 if (r, r) not in blocks_of(only) else int(n)) for r, n in enumerate(D.row_sizes)]) if D.nbr else np.zeros(0, int)
    return B, np.abs(B).astype(np.float64), dims.astype(np.float64)


def bar_of(w, ref, d, dtype):
    bar = (d + (12 if is_complex(dtype) else 6)) * U53 * w + d * EPS_LD * w
    if np.dtype(dtype) == np.float32:
        bar = bar + 2.0 ** -24 * np.abs(ref).astype(np.float64)
    return bar


def block_product(B, F, offsets, left):
    """B @ F (left) or F @ B (right) for a block-diagonal B: block row by block row (block column by block column), without the zeros of B"""
    out = np.zeros(F.shape, np.result_type(B.dtype, F.dtype))
    for a, b in zip(offsets[:-1], offsets[1:]):
        if left:
            out[a:b] = B[a:b, a:b] @ F[a:b]
        else:
            out[:, a:b] = F[:, a:b] @ B[a:b, a:b]
    return out


def reference(F, D, side, trans, alpha, dtype):
    """(ref in long double, bar in float64) for every element of the dense matrix F (long double): one pass, side left or right"""
    B, absB, dims = blockdiag_dense(D, trans)
    off = np.concatenate([[0], np.cumsum(D.row_sizes)])
    left = side == "left"
    ref = alpha * block_product(B, F, off, left)
    w = abs(alpha) * block_product(absB, np.abs(F).astype(np.float64), off, left)
    d = dims[:, None] if left else dims[None, :]
    return ref, bar_of(w, ref, d, dtype)


def reference_both(F, D, trans, alpha, dtype):
    """(ref, two-pass bar) of alpha op(D) F op(D)^+ (the module's text)"""
    T, bar_left = reference(F, D, "left", trans, alpha, dtype)
    ref, bar_right = reference(T, D, "right", dagger(trans, dtype), 1.0, dtype)
    _, absB, _ = blockdiag_dense(D, dagger(trans, dtype))
    off = np.concatenate([[0], np.cumsum(D.row_sizes)])
    return ref, bar_right + block_product(absB, bar_left, off, False)


def with_data(M, data):
    return O.Bcsr(M.row_sizes, M.col_sizes, M.row_p, M.col_i, M.blk_p, data)


def in_double(M, D, side, trans, alpha):
    """the same pass block by block in float64 / complex128 (np.einsum), rounded to the data's type once: the data area of the result"""
    out = M.data.copy()
    rows = M.rows()
    W = np.complex128 if is_complex(M.data.dtype) else np.float64
    have = blocks_of(D)
    for b in range(M.nblks):
        r, c = int(rows[b]), int(M.col_i[b])
        m, n = int(M.row_sizes[r]), int(M.col_sizes[c])
        a = M.data[M.blk_p[b]:M.blk_p[b] + m * n].astype(W).reshape(n, m).T
        i = r if side == "left" else c
        if (i, i) not in have:
            res = np.zeros((m, n), W)
        else:
            k = m if side == "left" else n
            d = op_of(have[(i, i)].astype(W).reshape(k, k).T, trans)
            res = alpha * (np.einsum("ik,kj->ij", d, a) if side == "left" else np.einsum("ik,kj->ij", a, d))
        out[M.blk_p[b]:M.blk_p[b] + m * n] = res.T.reshape(-1).astype(M.data.dtype)
    return out


def zeroed_mask(M, D, side):
    """the elements of M's data area in blocks whose diagonal block D lacks"""
    out = np.zeros(M.data.size, bool)
    rows = M.rows()
    have = blocks_of(D)
    for b in range(M.nblks):
        i = int(rows[b]) if side == "left" else int(M.col_i[b])
        if (i, i) not in have:
            out[M.blk_p[b]:M.blk_p[b] + int(M.row_sizes[rows[b]]) * int(M.col_sizes[M.col_i[b]])] = True
    return out


def positive_zero(x):
    return same_bits(np.ascontiguousarray(x), np.zeros(x.shape, x.dtype))


def stored_within(got_data, M, ref, bar, mask, what):
    within(dense(with_data(M, got_data))[mask], ref[mask], bar[mask], what)


def alpha_of(dtype):
    return scalars(dtype)[0]


# ---- device helpers -----------------------------------------------------------------------------------------------------------------------------------------
def run(eng, M, D, side, trans, alpha, dM=None, dD=None, **kw):
    """the data area of the result of one call on fresh copies (or on dM / dD)"""
    dM = to_dev(M) if dM is None else dM
    dD = to_dev(D) if dD is None else dD
    assert dbcsr_scale_by_block_diag(dM, dD, side, trans, alpha, engine=eng, **kw) is None
    torch.cuda.synchronize()
    return dM.data.cpu().numpy()


def placed(dM):
    """the same matrix with its data area GUARD + 1 elements into an allocation full of canaries"""
    n = dM.data.numel()
    big = torch.full((n + 2 * GUARD + 4,), CANARY, dtype=dM.data.dtype, device=dM.data.device)
    view = big[GUARD + 1:GUARD + 1 + n]
    view.copy_(dM.data)
    return DbcsrMatrix(dM.row_blk_size, dM.col_blk_size, dM.row_p, dM.col_i, dM.blk_p, view, nze=dM.nze), big


# ---- 1. left and right against the reference ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trans", ["N", "T", "C"])
@pytest.mark.parametrize("side", ["left", "right"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("which", MATRICES)
def test_one_side_against_the_reference(eng, which, dtype, side, trans):
    M, F, mask = host_matrix(which, np.dtype(dtype).name)
    D = diag_for(M, side, dtype)
    alpha = alpha_of(dtype)
    got = run(eng, M, D, side, trans, alpha)
    ref, bar = reference(F, D, side, trans, alpha, dtype)
    stored_within(got, M, ref, bar, mask, "%s %s %s" % (which, side, trans))
    zero = zeroed_mask(M, D, side)
    assert which == "tall67" or zero.any()   # (tall67 has three block rows: none of them is one without a diagonal block)
    assert positive_zero(got[zero]), "a block whose diagonal block is missing becomes +0.0"
    assert same_bits(run(eng, M, D, side, trans, alpha), got), "the same bits on every call"


# ---- 2. identity blocks ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", ["left", "right"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("which", MATRICES)
def test_identity_blocks_change_no_value(eng, which, dtype, side):
    M, _, _ = host_matrix(which, np.dtype(dtype).name)
    assert not np.any(np.signbit(M.data.real) & (M.data.real == 0)) and not np.any(np.signbit(M.data.imag) & (M.data.imag == 0)), "no -0 in the input"
    sizes = M.row_sizes if side == "left" else M.col_sizes
    I = from_blocks(sizes, sizes, {(r, r): np.eye(int(n)).reshape(-1) for r, n in enumerate(sizes)}, np.dtype(dtype))
    for trans in ("N", "C"):
        got = run(eng, M, I, side, trans, 1.0)
        assert np.array_equal(got, M.data), "every stored value compares equal to what it was"


# ---- 3. an independent device path ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("which", ["gappy", "tiles"])
def test_the_general_multiply_agrees(eng, which, dtype):
    """dbcsr_multiply(blockdiag(D), A) onto A's pattern: both results within their bars of the same reference (the multiply's: the project's 1e-10 by
    maximum element, 1e-5 for float32, whose multiply sums in float32)"""
    M, F, mask = host_matrix(which, np.dtype(dtype).name)
    D = diag_for(M, "left", dtype)
    alpha = alpha_of(dtype)
    ref, bar = reference(F, D, "left", "N", alpha, dtype)
    stored_within(run(eng, M, D, "left", "N", alpha), M, ref, bar, mask, "in place")
    dC = to_dev(with_data(M, np.zeros(M.data.size, M.data.dtype)))
    dbcsr_multiply("N", "N", alpha, to_dev(subset(D, lambda r, c: r == c)), to_dev(M), 0.0, dC, retain_sparsity=True, engine=eng)
    torch.cuda.synchronize()
    Cm = dev_to_bcsr(dC)
    assert np.array_equal(Cm.row_p, M.row_p) and np.array_equal(Cm.col_i, M.col_i)
    tol = (1e-5 if np.dtype(dtype) == np.float32 else 1e-10) * float(np.max(np.abs(ref[mask])))
    assert float(np.max(np.abs(dense(Cm).astype(ref.dtype) - ref)[mask])) <= tol


# ---- 4. missing diagonal blocks ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", ["left", "right"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_nan_under_a_missing_diagonal_block_does_not_survive(eng, dtype, side):
    M, _, mask = host_matrix("edge", np.dtype(dtype).name)
    D = diag_for(M, side, dtype)
    zero = zeroed_mask(M, D, side)
    assert zero.any() and not zero.all()
    data = M.data.copy()
    data[zero] = np.nan
    P = with_data(M, data)
    alpha = alpha_of(dtype)
    got = run(eng, P, D, side, "N", alpha)
    assert positive_zero(got[zero])
    clean = with_data(M, np.where(zero, 0, M.data).astype(M.data.dtype))
    ref, bar = reference(dense(clean).astype(wide(dtype)), D, side, "N", alpha, dtype)
    stored_within(got, M, ref, bar, mask, "poisoned %s" % side)


# ---- 5. blocks of diag off the diagonal are not read --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", ["left", "right"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_blocks_off_the_diagonal_of_diag_are_not_read(eng, dtype, side):
    M, _, _ = host_matrix("tiles", np.dtype(dtype).name)
    D = diag_for(M, side, dtype)
    assert any(r != c for r, c in blocks_of(D))
    alpha = alpha_of(dtype)
    got = run(eng, M, D, side, "T", alpha)
    dD = to_dev(D)
    only = dbcsr_get_block_diag(dD, engine=eng)
    assert only.nblks < dD.nblks
    assert same_bits(run(eng, M, D, side, "T", alpha, dD=only), got)
    poisoned = {k: (np.full(v.size, np.nan, v.dtype) if k[0] != k[1] else v) for k, v in blocks_of(D).items()}
    assert same_bits(run(eng, M, from_blocks(D.row_sizes, D.col_sizes, poisoned, D.data.dtype), side, "T", alpha), got)


# ---- 6. nothing else is written ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", ["left", "right", "both"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_holes_guards_and_indices_keep_their_bits(eng, dtype, side):
    dtype = np.dtype(dtype)
    M0 = typed(matrix("gappy"), dtype, 1)
    M, dH = with_holes(eng, M0, dtype)
    holes = hole_positions(M)
    assert holes.size > 0
    dM, big = placed(dH)
    D = diag_for(M, "left", dtype)
    dD, dbig = placed(to_dev(D))
    before, dbefore = big.cpu().numpy().copy(), dbig.cpu().numpy().copy()
    index = [t.clone() for m in (dM, dD) for t in (m.row_p, m.col_i, m.blk_p, m.row_blk_size, m.col_blk_size)]
    stamps = dM.index_stamp(), dD.index_stamp()
    alpha = -1.3 if side == "both" else alpha_of(dtype)
    dbcsr_scale_by_block_diag(dM, dD, side, "N", alpha, engine=eng)
    torch.cuda.synchronize()
    assert (dM.index_stamp(), dD.index_stamp()) == stamps
    now = [t for m in (dM, dD) for t in (m.row_p, m.col_i, m.blk_p, m.row_blk_size, m.col_blk_size)]
    assert all(torch.equal(a, b) for a, b in zip(index, now))
    assert same_bits(dbig.cpu().numpy(), dbefore), "diag is only read"
    after = big.cpu().numpy()
    used = np.ones(M.data.size, bool)
    used[holes] = False
    inside = np.zeros(after.size, bool)
    inside[GUARD + 1:GUARD + 1 + M.data.size] = used
    assert same_bits(after[~inside], before[~inside]), "holes and guards keep their bits"
    H = dev_to_bcsr(dM)
    F, mask = dense(M).astype(wide(dtype)), pattern_mask(M)
    ref, bar = reference_both(F, D, "N", alpha, dtype) if side == "both" else reference(F, D, side, "N", alpha, dtype)
    stored_within(H.data, M, ref, bar, mask, "with holes, %s" % side)


def test_a_multiply_reuses_its_plan_afterwards(monkeypatch):
    monkeypatch.delenv("DBCSR_AMD_MM_PLAN", raising=False)
    eng = MultiplyEngine()
    M, _, _ = host_matrix("gappy", "float64")
    D = diag_for(M, "left", np.float64)
    dA, dB, dD = to_dev(M), to_dev(M), to_dev(D)
    dC = to_dev(subset(M, lambda r, c: False))
    dbcsr_multiply("N", "N", 1.0, dA, dB, 0.0, dC, engine=eng)
    reused, built = eng.plan_stats()
    for side in ("left", "right", "both"):
        dbcsr_scale_by_block_diag(dA, dD, side, engine=eng)
    dbcsr_multiply("N", "N", 1.0, dA, dB, 0.0, dC, engine=eng)
    assert eng.plan_stats() == (reused + 1, built), "a multiply after the call must reuse its plan"
    torch.cuda.synchronize()
    got, ref = dense(dev_to_bcsr(dC)), dense(dev_to_bcsr(dA)) @ dense(M)
    assert np.max(np.abs(got - ref)) <= 1e-10 * np.max(np.abs(ref))


# ---- 7. both sides -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trans", ["N", "T", "C"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("which", ["gappy", "edge"])
def test_both_is_left_then_right(eng, which, dtype, trans):
    M, F, mask = host_matrix(which, np.dtype(dtype).name)
    D = diag_for(M, "left", dtype)
    alpha = alpha_of(dtype)
    got = run(eng, M, D, "both", trans, alpha)
    dM, dD = to_dev(M), to_dev(D)
    dbcsr_scale_by_block_diag(dM, dD, "left", trans, alpha, engine=eng)
    rc = eng.L.dbcsr_amd_bcsr_block_diag_multiply(eng.h, dM.dtype_code, b"R", dagger(trans, dtype).encode(), (C.c_double * 2)(1.0, 0.0),
                                                  C.byref(dD.desc()), C.byref(dM.desc()), 96, StreamHandle().ptr)
    assert rc == 0
    torch.cuda.synchronize()
    assert same_bits(dM.data.cpu().numpy(), got), "bit for bit the left call followed by the right call with op'"
    if dagger(trans, dtype) != "J":
        dM = to_dev(M)
        dbcsr_scale_by_block_diag(dM, dD, "left", trans, alpha, engine=eng)
        assert same_bits(run(eng, M, D, "right", dagger(trans, dtype), 1.0, dM=dM, dD=dD), got)
    ref, bar = reference_both(F, D, trans, alpha, dtype)
    stored_within(got, M, ref, bar, mask, "both %s %s" % (which, trans))


@pytest.mark.parametrize("trans", ["N", "T", "C"])
@pytest.mark.parametrize("dtype,symmetry", [(np.float64, "S"), (np.float32, "S"), (np.complex128, "H")], ids=["fp64_S", "fp32_S", "z64_H"])
def test_a_congruence_of_a_stored_triangle(eng, dtype, symmetry, trans):
    M = typed(symmetric_base(symmetry), np.dtype(dtype), 3)
    D = diag_for(M, "left", dtype)
    alpha = -1.3
    as_n = run(eng, M, D, "both", trans, alpha)
    dM = to_dev(M)
    dM.symmetry = symmetry
    got = run(eng, M, D, "both", trans, alpha, dM=dM)
    assert same_bits(got, as_n), "the stored triangle has the bits of the same triangle run as an 'N' matrix"
    full = desymmetrized_dense(M, symmetry).astype(wide(dtype))
    ref, bar = reference_both(full, D, trans, alpha, dtype)
    stored = pattern_mask(M)
    bar = np.where(stored, bar, bar.T)   # (a twin carries the bar of the element it mirrors)
    within(desymmetrized_dense(with_data(M, got), symmetry)[pattern_mask(M, symmetry)], ref[pattern_mask(M, symmetry)], bar[pattern_mask(M, symmetry)],
           "congruence %s %s" % (symmetry, trans))


# ---- 8. alpha == 0 ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", ["left", "right", "both"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_alpha_zero_reads_nothing(eng, dtype, side):
    M, _, _ = host_matrix("edge", np.dtype(dtype).name)
    D = diag_for(M, "left", dtype)
    nan = lambda X: with_data(X, np.full(X.data.size, np.nan, X.data.dtype))
    got = run(eng, nan(M), nan(D), side, "N", 0.0)
    assert positive_zero(got), "every element of every stored block is +0.0"


# ---- 9. an Inf stays in its column (left) / row (right) --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", ["left", "right"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_an_inf_stays_in_its_column_or_row(eng, dtype, side):
    M, _, mask = host_matrix("tiles", np.dtype(dtype).name)
    D = diag_for(M, side, dtype)
    have = blocks_of(D)
    rows = M.rows()
    b = next(b for b in range(M.nblks) if ((int(rows[b]),) * 2 if side == "left" else (int(M.col_i[b]),) * 2) in have
             and M.row_sizes[rows[b]] == 33 and M.col_sizes[M.col_i[b]] >= 32)
    m, n = int(M.row_sizes[rows[b]]), int(M.col_sizes[M.col_i[b]])
    k, j = (20, 18)   # (row, column) of the Inf inside the block: second tile of either dimension
    data = M.data.copy()
    data[M.blk_p[b] + j * m + k] = np.inf
    alpha = alpha_of(dtype)
    got = run(eng, with_data(M, data), D, side, "N", alpha)
    blk = got[M.blk_p[b]:M.blk_p[b] + m * n].reshape(n, m).T
    bad = ~np.isfinite(blk)
    allowed = np.zeros((m, n), bool)
    if side == "left":
        allowed[:, j] = True
    else:
        allowed[k, :] = True
    assert bad.any() and not np.any(bad & ~allowed), "only the Inf's column (left) / row (right) of its block may be non-finite"
    clean = M.data.copy()
    ref, bar = reference(dense(with_data(M, clean)).astype(wide(dtype)), D, side, "N", alpha, dtype)
    G = dense(with_data(M, np.where(np.isfinite(got), got, 0).astype(got.dtype)))
    touched = np.zeros(M.data.size, bool)
    idx = np.arange(m * n).reshape(n, m).T[allowed]
    touched[M.blk_p[b] + idx] = True
    untouched = dense(with_data(M, (~touched).astype(np.float64))) != 0
    within(G[mask & untouched], ref[mask & untouched], bar[mask & untouched], "everything else, %s" % side)


# ---- 10. on a side stream -----------------------------------------------------------------------------------------------------------------------------------------
def test_on_a_stream_of_its_own(eng):
    M, _, _ = host_matrix("gappy", "float64")
    D = diag_for(M, "left", np.float64)

    def sequence(stream):
        dA, dB, dD = to_dev(M), to_dev(M), to_dev(D)
        dC = to_dev(subset(M, lambda r, c: False))
        torch.cuda.synchronize()
        if stream is None:
            dbcsr_scale_by_block_diag(dA, dD, "both", "T", 0.7, engine=eng)
            dbcsr_multiply("N", "N", 1.0, dA, dB, 0.0, dC, engine=eng)
        else:
            with torch.cuda.stream(stream):
                dbcsr_scale_by_block_diag(dA, dD, "both", "T", 0.7, engine=eng, stream=stream)
                dbcsr_multiply("N", "N", 1.0, dA, dB, 0.0, dC, engine=eng)   # (on the current stream: the side stream)
            stream.synchronize()
        torch.cuda.synchronize()
        return dA.data.cpu().numpy(), dev_to_bcsr(dC).data

    a0, c0 = sequence(None)
    a1, c1 = sequence(torch.cuda.Stream())
    assert same_bits(a0, a1) and same_bits(c0, c1), "the same bits on a side stream as on the default stream"


# ---- 11. composition: blockdiag(S)^-1 S ------------------------------------------------------------------------------------------------------------------------------
COMPOSE_SIZES = (5, 13, 16, 17, 23, 33, 64, 96)


@functools.lru_cache(maxsize=None)
def spd_matrix(dtype_name):
    """diagonal blocks of the family spd of tests/test_gpu_block_inverse.py (condition numbers <= 10^3), every block off the diagonal uniform in [-1, 1]"""
    from tests.test_gpu_block_inverse import block, column_major
    dtype = np.dtype(dtype_name)
    sizes = np.asarray(COMPOSE_SIZES, np.int32)
    rng = np.random.default_rng(11)
    blocks = {}
    for r in range(len(sizes)):
        for c in range(len(sizes)):
            if r == c:
                blocks[(r, c)] = column_major(block("spd", int(sizes[r]), dtype.name))
            elif rng.random() < 0.6:
                blocks[(r, c)] = uniform(rng, int(sizes[r]) * int(sizes[c]), is_complex(dtype)).astype(dtype)
    return from_blocks(sizes, sizes, blocks, dtype)


def identity_margin(n, dtype):
    """How far a diagonal block of blockdiag(S)^-1 S may be from the identity: d 2^-40 for float64 / complex128 data (condition numbers <= 10^3: the
    inverse's own bar, K d 2^-53 w, is far below).  float32 data cannot meet that: every element of the inverse is rounded to 2^-24 |x_ik|, and the d
    terms x_ik s_ki of a diagonal element carry that rounding with |x_ik| <= ||X||_2 <= 2 (the family's eigenvalues are >= 1/2) and |s_ki| <= 2, the
    result one more -- d 2^-22.  tests/test_block_scale_cpu.py checks that plain arithmetic uses less than half of either."""
    return n * (2.0 ** -40 if np.dtype(dtype) != np.float32 else 2.0 ** -22)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_preconditioned_operator(eng, dtype):
    S = spd_matrix(np.dtype(dtype).name)
    dS = to_dev(S)
    dD = dbcsr_get_block_diag(dS, engine=eng)
    assert dbcsr_invert_block_diag(dD, engine=eng) == (0, -1)
    dA = dS.copy()
    dbcsr_scale_by_block_diag(dA, dD, "left", engine=eng)
    torch.cuda.synchronize()
    D = dev_to_bcsr(dD)
    got = dA.data.cpu().numpy()
    ref, bar = reference(dense(S).astype(wide(dtype)), D, "left", "N", 1.0, dtype)
    stored_within(got, S, ref, bar, pattern_mask(S), "D^-1 S")
    for (r, c), v in blocks_of(with_data(S, got)).items():
        if r == c:
            n = int(S.row_sizes[r])
            assert np.max(np.abs(v.reshape(n, n).T - np.eye(n))) <= identity_margin(n, dtype), (r, n)


# ---- 12. far offsets --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def arena():
    a = FA.arena()
    yield a
    if a is not None:
        a.release()
        del a
    torch.cuda.empty_cache()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_far_matrix(eng, arena, dtype):
    """the matrix' blocks placed around 2^29, 2^31, 2^32, ... elements of one large allocation (tests/far_arena.py)"""
    from tests.test_gpu_far_offsets import one_far
    M, F, mask = host_matrix("mixed", np.dtype(dtype).name)
    far, dM = one_far(arena, M, dtype, "blocks", who=1 if is_complex(dtype) else 0)
    blk_p = dM.blk_p.cpu().numpy()
    assert np.any(blk_p >= 2 ** 32)
    alpha = alpha_of(dtype)
    for side in ("left", "right"):
        before = FA.blocks_to_host(dM)
        D = diag_for(M, side, dtype)
        dbcsr_scale_by_block_diag(dM, to_dev(D), side, "C", alpha, engine=eng)
        torch.cuda.synchronize()
        ref, bar = reference(dense(with_data(M, before.data)).astype(wide(dtype)), D, side, "C", alpha, dtype)
        stored_within(FA.blocks_to_host(dM).data, M, ref, bar, mask, "a far matrix, %s" % side)
    assert far.guards_kept()


# ---- 13. refusals ------------------------------------------------------------------------------------------------------------------------------------------------------
def refusal_cases(dev):
    """[(error, matrix, diag, side, trans, alpha)] on tensors of the device `dev` ("cuda" / "cpu"); shared with tests/test_block_scale_cpu.py"""
    def mat(M, symmetry="N"):
        t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(dev)
        return DbcsrMatrix(t(M.row_sizes, torch.int32), t(M.col_sizes, torch.int32), t(M.row_p, torch.int32), t(M.col_i, torch.int32), t(M.blk_p, torch.int64),
                           torch.as_tensor(M.data).to(dev), symmetry=symmetry)

    G = typed(base("gappy"), np.float64, 1)
    Dg = diag_for(G, "left", np.float64)
    R = typed(base("mixed"), np.float64, 1)     # rectangular: 230 x 260
    Dr, Dc = diag_for(R, "left", np.float64), diag_for(R, "right", np.float64)
    Z, Dz = typed(base("gappy"), np.complex128, 1), diag_for(G, "left", np.complex128)
    sizes = np.asarray([5, 97], np.int32)
    big = from_blocks(sizes, sizes, {(0, 0): np.eye(5).reshape(-1), (1, 1): np.eye(97).reshape(-1)}, np.float64)
    g = mat(G)
    shared = torch.as_tensor(np.concatenate([G.data, Dg.data])).to(dev)
    g_in, d_in = mat(G), mat(Dg)
    g_in.data, d_in.data = shared[:G.data.size], shared[G.data.size - 1:G.data.size - 1 + Dg.data.size]
    cases = [
        (TypeError, mat(G), mat(diag_for(G, "left", np.float32)), "left", "N", 1.0),
        (ValueError, mat(G), mat(R), "left", "N", 1.0),                       # diag not square in block structure
        (ValueError, mat(R), mat(Dc), "left", "N", 1.0),                      # diag's sizes are not the row sizes
        (ValueError, mat(R), mat(Dr), "right", "N", 1.0),                     # ... not the column sizes
        (ValueError, mat(R), mat(Dr), "both", "N", 1.0),
        (ValueError, mat(G), mat(Dg), "middle", "N", 1.0),
        (ValueError, mat(G), mat(Dg), "left", "X", 1.0),
        (TypeError, mat(G), mat(Dg), "left", "N", 1.0 + 2.0j),
        (ValueError, g, g, "left", "N", 1.0),                                 # diag is matrix
        (ValueError, g_in, d_in, "left", "N", 1.0),                           # two views of one allocation that share an element
        (NotImplementedError, mat(big), mat(big.__class__(big.row_sizes, big.col_sizes, big.row_p, big.col_i, big.blk_p, big.data.copy())), "left", "N", 1.0),
        (ValueError, mat(G, "A"), mat(Dg), "both", "N", 1.0),
        (ValueError, mat(Z, "K"), mat(Dz), "both", "N", 1.0),
        (ValueError, mat(Z, "S"), mat(Dz), "both", "N", 1.0),                 # 'S' of complex data
        (ValueError, mat(G), mat(Dg, "A"), "left", "N", 1.0),
        (ValueError, mat(Z), mat(Dz, "K"), "left", "N", 1.0),
        (ValueError, mat(G, "S"), mat(Dg), "left", "N", 1.0),                 # a stored triangle takes both sides only
        (ValueError, mat(G, "S"), mat(Dg), "right", "N", 1.0),
        (ValueError, mat(Z, "H"), mat(Dz), "both", "N", 1.0 + 2.0j),          # 'H' takes a real alpha
    ]
    return cases


class Refuses:
    def __getattr__(self, name):
        raise AssertionError("the library was called (%s)" % name)


def check_refusals(eng, dev):
    for error, m, d, side, trans, alpha in refusal_cases(dev):
        before, stamp = m.data.clone(), m.index_stamp()
        with pytest.raises(error):
            dbcsr_scale_by_block_diag(m, d, side, trans, alpha, engine=eng)
        assert m.index_stamp() == stamp and torch.equal(m.data, before), (error, side, trans)


def test_refusals_come_before_any_call(monkeypatch):
    eng = MultiplyEngine()
    monkeypatch.setattr(eng, "L", Refuses())
    check_refusals(eng, "cuda")


def test_c_abi_answers(eng):
    M, _, _ = host_matrix("gappy", "float64")
    dM, dD = to_dev(M), to_dev(diag_for(M, "left", np.float64))
    one = (C.c_double * 2)(1.0, 0.0)

    def call(side=b"L", trans=b"N", alpha=one, diag=dD, m=dM, max_dim=96, code=None, handle=None):
        rc = eng.L.dbcsr_amd_bcsr_block_diag_multiply(eng.h if handle is None else handle, dM.dtype_code if code is None else code, side, trans, alpha,
                                                      C.byref(diag.desc()) if diag is not None else None, C.byref(m.desc()) if m is not None else None,
                                                      max_dim, StreamHandle().ptr)
        torch.cuda.synchronize()
        return rc

    before = dM.data.clone()
    assert call(side=b"B") == -1 and call(trans=b"X") == -1 and call(alpha=None) == -1 and call(diag=None) == -1 and call(m=None) == -1
    assert call(max_dim=-1) == -1 and call(max_dim=97) == -11 and call(code=99) == -10 and call(diag=dM) == -1
    rect = to_dev(typed(base("mixed"), np.float64, 1))
    assert call(diag=rect) == -1 and call(m=rect) == -1
    assert torch.equal(dM.data, before), "a refused call writes nothing"
    assert call(trans=b"J") == 0 and not torch.equal(dM.data, before)
