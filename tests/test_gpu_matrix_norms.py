"""Norms and vectors on the device (dbcsr_amd/operations.py: dbcsr_norm, dbcsr_gershgorin_norm, dbcsr_maxabs_norm, dbcsr_get_diag, dbcsr_set_diag,
dbcsr_scale_by_vector; the "Norms and vectors" entries of include/dbcsr_amd_mm.h; kernels of dbcsr_amd/csrc/mm_algebra.h) for float64, float32 and
complex128.

Reference: numpy on the dense scatter of the matrix (for a stored triangle: of the desymmetrized matrix), in float64.

Bars, derived (u = 2^-53: sums are carried in double for every data type):
  row / column sums  n non-negative terms: |got - ref| <= (n + 4) u ref, ref = math.fsum of the terms formed in float64 (any summation order in double
                     is within (n - 1) u; a term x * x of float64 data carries one rounding, float32 products are exact).  A complex |x| is the root of
                     re^2 + im^2 and carries 2 u of its own: (n + 6) u.  A complex |x|^2 is two terms.  n = the stored elements of the row / column.
  gershgorin         the maximum is 1-Lipschitz: the largest of the rows' bars.
  column norm        the root adds one u: relative (n + 5) u.
  maxabs             real data: exactly the largest |x| of the elements the index names; complex: relative 4 u (|x|^2 within 2 u, the root halves that and
                     adds one u, numpy's own |x| one more).
  get_diag           bit-identical to the dense diagonal, zero where a diagonal block is missing.
  set_diag           the diagonal elements of the diagonal blocks present equal the vector bit for bit, every other element of the data area (holes
                     included) is unchanged bit for bit, the index tensors are the same objects with the same stamp.
  scale_by_vector    real data: bit-identical to a * v formed in the data's precision (one rounding); complex: <= 4 u |a| |v|.  Left then right with one
                     vector on a square matrix: within 2 (complex: 8) units of the data's precision of |d_i a_ij d_j|.
  sign iteration     the project's 1e-10 by maximum element against the same iteration in numpy (the sign matrix has unit scale).
Matrices: the smallest that reach every branch of the kernels -- the oracle's generator with the mixes [1, 13, 1, 5] x [1, 23, 1, 4] at 230 x 260 (fewer
than 64 lanes busy per block row, odd element counts, blocks that start at odd elements), tiny blocks ([1, 1, 1, 3], 76 block columns, fill 0.9), blocks of
70 and of 67 rows / columns (more than 64 element rows: for float64 / float32 70 still has a period of 35 and takes the 16-byte form, 67 and complex 70 take
the form for tall blocks; more than 64 columns: two passes of the column sums; more than 1024 elements: several staged pieces), stored triangles, an operand
with holes, a data area that is not 16-byte aligned, an empty matrix, and one with empty block rows / columns and missing diagonal blocks."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import dbcsr_amd
from dbcsr_amd import lib as L
from dbcsr_amd.matrix import DbcsrMatrix, StreamHandle
from dbcsr_amd.multiply import MultiplyEngine, dbcsr_multiply
from dbcsr_amd.operations import (dbcsr_add, dbcsr_add_on_diag, dbcsr_frobenius_norm, dbcsr_get_diag, dbcsr_gershgorin_norm, dbcsr_maxabs_norm,
                                  dbcsr_norm, dbcsr_norm_column, dbcsr_norm_frobenius, dbcsr_norm_gershgorin, dbcsr_norm_maxabsnorm, dbcsr_scale,
                                  dbcsr_scale_by_vector, dbcsr_set_diag)
from oracle import oracle as O
from tests.gpu_util import dev_to_bcsr, to_dev

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32, np.complex128]
IDS = ["fp64", "fp32", "z64"]
U53 = 2.0 ** -53
TORCH = {np.dtype(np.float64): torch.float64, np.dtype(np.float32): torch.float32, np.dtype(np.complex128): torch.complex128}


def unit(dtype):
    return 2.0 ** -24 if np.dtype(dtype) == np.float32 else U53


def is_complex(dtype):
    return np.dtype(dtype).kind == "c"


@pytest.fixture(scope="module")
def eng():
    return MultiplyEngine()


# ---- host helpers (as tests/test_gpu_matrix_ops.py has them) ------------------------------------------------------------------------------------
def blocks_of(M):
    rows = M.rows()
    out = {}
    for b in range(M.nblks):
        r, c = int(rows[b]), int(M.col_i[b])
        ne = int(M.row_sizes[r]) * int(M.col_sizes[c])
        out[(r, c)] = M.data[M.blk_p[b]:M.blk_p[b] + ne]
    return out


def from_blocks(rs, cs, blocks, dtype):
    """packed matrix of the blocks given: sorted block columns per row, blk_p the running sum of the block sizes"""
    keys = sorted(blocks)
    rr = np.asarray([k[0] for k in keys], np.int64)
    cc = np.asarray([k[1] for k in keys], np.int32)
    nze = np.asarray([int(rs[r]) * int(cs[c]) for r, c in keys], np.int64)
    blk_p = np.concatenate([[0], np.cumsum(nze)[:-1]]).astype(np.int64) if keys else np.zeros(0, np.int64)
    data = np.concatenate([np.asarray(blocks[k], dtype) for k in keys]) if keys else np.zeros(0, dtype)
    row_p = np.zeros(len(rs) + 1, np.int64)
    np.add.at(row_p, rr + 1, 1)
    return O.Bcsr(rs, cs, np.cumsum(row_p).astype(np.int32), cc, blk_p, data.astype(dtype))


def typed(M, dtype, seed=7):
    """the oracle's float64 matrix in another data type; complex: uniform(-1, 1) imaginary parts laid over it, and signs on the real parts"""
    if is_complex(dtype):
        rng = np.random.default_rng(seed)
        data = M.data * rng.choice([-1.0, 1.0], M.data.size) + 1j * rng.uniform(-1.0, 1.0, M.data.size)
    else:
        data = M.data - 0.4   # (both signs)
    return O.Bcsr(M.row_sizes, M.col_sizes, M.row_p, M.col_i, M.blk_p, data.astype(dtype))


def dense(M):
    if M.data.dtype.kind == "c":
        re = O.Bcsr(M.row_sizes, M.col_sizes, M.row_p, M.col_i, M.blk_p, np.ascontiguousarray(M.data.real))
        im = O.Bcsr(M.row_sizes, M.col_sizes, M.row_p, M.col_i, M.blk_p, np.ascontiguousarray(M.data.imag))
        return re.to_dense() + 1j * im.to_dense()
    return M.to_dense()


def same_bits(x, y):
    return x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


def subset(M, keep):
    """M without the blocks for which keep(r, c) is false (packed again)"""
    return from_blocks(M.row_sizes, M.col_sizes, {k: v for k, v in blocks_of(M).items() if keep(*k)}, M.data.dtype)


def desymmetrized_dense(M, symmetry):
    """the full matrix of a stored triangle, in numpy: block (c, r) = twin of block (r, c)"""
    D = dense(M)
    off = dense(subset(M, lambda r, c: r != c))
    T = off.T
    if symmetry in ("H", "K"):
        T = T.conj()
    return D + (T if symmetry in ("S", "H") else -T)


def pattern_mask(M, symmetry="N"):
    ones = O.Bcsr(M.row_sizes, M.col_sizes, M.row_p, M.col_i, M.blk_p, np.ones(M.data.size))
    return (dense(ones) if symmetry == "N" else desymmetrized_dense(ones, "S")) != 0


def from_dense(D, rs, cs, dtype):
    """every block of the dense matrix, stored (a full pattern)"""
    ro, co = np.concatenate([[0], np.cumsum(rs)]), np.concatenate([[0], np.cumsum(cs)])
    blocks = {(r, c): D[ro[r]:ro[r + 1], co[c]:co[c + 1]].T.reshape(-1) for r in range(len(rs)) for c in range(len(cs))}
    return from_blocks(rs, cs, blocks, dtype)


# ---- the matrices (float64 from the oracle's generator; typed() per test) -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def base(which):
    if which == "mixed":
        return O.perf_case(230, 260, 200, 0.5, 0.5, 0.7, [1, 13, 1, 5], [1, 23, 1, 4], [1, 7, 1, 32])[2]
    if which == "tiny":
        M = O.perf_case(150, 150, 150, 0.1, 0.1, 0.1, [1, 1, 1, 3], [1, 1, 1, 3], [1, 1, 1, 3])[2]
        assert M.nbc >= 70 and np.max(np.diff(M.row_p)) > 64 and np.array_equal(M.row_sizes, M.col_sizes)
        return M
    if which in ("tall70", "tall67"):
        big = 70 if which == "tall70" else 67
        sizes = O.make_block_sizes(3 * big + 6 if big == 70 else 2 * big + 3, [1, big, 1, 3])
        assert sizes.max() == big and sizes.min() == 3 and len(sizes) in (3, 5)
        M = O.make_random_matrix(sizes, sizes, 0.2, O.RANDMAT_SEED_INIT + 51)
        b = blocks_of(M)
        assert any(sizes[r] == big and sizes[c] == big for r, c in b) and any(sizes[r] == 3 and sizes[c] == big for r, c in b)
        return M
    if which == "square":
        sizes = O.make_block_sizes(200, [1, 13, 1, 5, 1, 7])
        M = O.make_random_matrix(sizes, sizes, 0.5, O.RANDMAT_SEED_INIT + 31)
        have = {r for r, c in blocks_of(M) if r == c}
        assert 0 < len(have) < M.nbr
        return M
    if which == "gappy":
        sizes = O.make_block_sizes(200, [1, 13, 1, 5, 1, 7])
        full = O.make_random_matrix(sizes, sizes, 0.3, O.RANDMAT_SEED_INIT + 52)
        M = subset(full, lambda r, c: r % 5 not in (1, 2) and c % 7 != 3 and not (r == c and r % 3 == 0))
        b = blocks_of(M)
        assert sum(1 for r in range(M.nbr) if M.row_p[r] == M.row_p[r + 1]) >= 3, "several block rows are empty"
        assert sum(1 for c in range(M.nbc) if not any(k[1] == c for k in b)) >= 3, "several block columns are empty"
        rows_with_blocks = [r for r in range(M.nbr) if M.row_p[r] < M.row_p[r + 1]]
        assert sum(1 for r in rows_with_blocks if (r, r) not in b) >= 3 and any((r, r) in b for r in rows_with_blocks), "diagonal blocks missing, and present"
        return M
    raise KeyError(which)


def symmetric_base(symmetry):
    sizes = O.make_block_sizes(200, [1, 13, 1, 5, 1, 7])
    return O.make_random_matrix_symmetric(sizes, 0.6, O.RANDMAT_SEED_INIT + 21, "S" if symmetry in ("S", "H") else "A")


def misaligned(dM):
    """the same matrix with its data area starting one element into a larger tensor: not 16-byte aligned for float64 and float32 (an element of complex128
    is 16 bytes: its view stays aligned, and is one more matrix whose data area does not start its allocation)"""
    big = torch.empty(dM.data.numel() + 3, dtype=dM.data.dtype, device=dM.data.device)
    view = big[1:1 + dM.data.numel()]
    view.copy_(dM.data)
    assert dM.data.is_complex() or view.data_ptr() % 16 != 0
    return DbcsrMatrix(dM.row_blk_size, dM.col_blk_size, dM.row_p, dM.col_i, dM.blk_p, view, nze=dM.nze)


def with_holes(eng, M, dtype):
    """(host matrix with the device's index, device matrix): the result of an in-place filter -- M's blocks where they were, holes between them"""
    extra = {k: (v * 1e-9).astype(dtype) for k, v in blocks_of(typed(O.make_random_matrix(M.row_sizes, M.col_sizes, 0.5, O.RANDMAT_SEED_INIT + 11), dtype, 2)).items()
             if k not in blocks_of(M)}
    assert extra
    full = dict(blocks_of(M))
    full.update(extra)
    dfull = to_dev(from_blocks(M.row_sizes, M.col_sizes, full, dtype))
    dB = eng.filtered(dfull, 1e-6, in_place=True)
    torch.cuda.synchronize()
    assert not dB.packed and dB.data is dfull.data and dB.nblks == M.nblks
    return dev_to_bcsr(dB), dB


def hole_positions(M):
    used = np.zeros(M.data.size, bool)
    rows = M.rows()
    for b in range(M.nblks):
        ne = int(M.row_sizes[rows[b]]) * int(M.col_sizes[M.col_i[b]])
        used[M.blk_p[b]:M.blk_p[b] + ne] = True
    return np.flatnonzero(~used)


# ---- C-ABI callers --------------------------------------------------------------------------------------------------------------------------------
def full_len(sizes):
    return int(np.sum(sizes))


def vec_sums(eng, dM, axis, what, skip=0, n_out=None, out=None):
    """dbcsr_amd_bcsr_row_sums (axis 0: one value per full row) / _col_sums (axis 1) into a float64 device tensor"""
    n = int((dM.row_blk_size if axis == 0 else dM.col_blk_size).sum().item()) if n_out is None else n_out
    out = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda") if out is None else out
    d = dM.desc()
    st = StreamHandle().ptr
    if axis == 0:
        rc = eng.L.dbcsr_amd_bcsr_row_sums(eng.h, dM.dtype_code, C.byref(d), what, out.data_ptr(), n, st)
    else:
        rc = eng.L.dbcsr_amd_bcsr_col_sums(eng.h, dM.dtype_code, C.byref(d), what, skip, out.data_ptr(), n, st)
    assert rc == 0
    torch.cuda.synchronize()
    return out.cpu().numpy()


def real_terms(x):
    """the float64 terms of sum |x|^2: a complex element gives two"""
    x = np.asarray(x)
    if x.dtype.kind == "c":
        return np.concatenate([x.real.astype(np.float64) ** 2, x.imag.astype(np.float64) ** 2])
    return x.astype(np.float64) ** 2


def reference_sums(D, mask, axis, what):
    """(refs, bars) per full row (axis 0) / column (axis 1) of the dense matrix, over the stored elements"""
    if axis == 1:
        D, mask = D.T, mask.T
    refs, bars = np.zeros(D.shape[0]), np.zeros(D.shape[0])
    for i in range(D.shape[0]):
        x = D[i, mask[i]]
        if what == 0:
            terms, extra = np.abs(x).astype(np.float64), (6 if D.dtype.kind == "c" else 4)
        else:
            terms, extra = real_terms(x), 4
        refs[i] = math.fsum(terms.tolist())
        bars[i] = (terms.size + extra) * U53 * refs[i]
    return refs, bars


def check_vector(got, refs, bars, what):
    assert got.shape == refs.shape
    err = np.abs(got - refs)
    worst = int(np.argmax(err - bars)) if err.size else 0
    print("%s: worst element %d: error %.3e against a bar of %.3e" % (what, worst, float(err[worst]) if err.size else 0.0, float(bars[worst]) if err.size else 0.0))
    assert np.all(err <= bars), what


def check_everything_read_only(eng, M, dM, symmetry="N"):
    """row / column sums of |x| and |x|^2, gershgorin, maxabs and (symmetry 'N') the column norms of the device matrix dM = the host matrix M"""
    D, mask = dense(M), pattern_mask(M)
    named = np.concatenate(list(blocks_of(M).values()) or [np.zeros(0, M.data.dtype)])
    cplx = M.data.dtype.kind == "c"
    sums = {}
    for axis in (0, 1):
        for what in (0, 1):
            refs, bars = reference_sums(D, mask, axis, what)
            got = vec_sums(eng, dM, axis, what)
            check_vector(got, refs, bars, "sums of axis %d, what %d" % (axis, what))
            assert same_bits(vec_sums(eng, dM, axis, what), got), "the same bits on every call"
            sums[(axis, what)] = (refs, bars)
    # column sums without the diagonal blocks
    if M.nbr == M.nbc:
        off = subset(M, lambda r, c: r != c)
        refs, bars = reference_sums(dense(off), pattern_mask(off), 1, 0)
        check_vector(vec_sums(eng, dM, 1, 0, skip=1), refs, bars, "column sums off the block diagonal")
    # gershgorin
    dM.symmetry = symmetry
    if symmetry == "N":
        refs, bars = sums[(0, 0)]
    else:
        refs, bars = reference_sums(desymmetrized_dense(M, symmetry), pattern_mask(M, symmetry), 0, 0)
    got = dbcsr_gershgorin_norm(dM, engine=eng)
    ref, bar = (float(np.max(refs)), float(np.max(bars))) if refs.size else (0.0, 0.0)
    print("gershgorin: %.17g against %.17g, bar %.3e" % (got, ref, bar))
    assert isinstance(got, float) and abs(got - ref) <= bar
    assert dbcsr_gershgorin_norm(dM, engine=eng) == got and dbcsr_norm(dM, dbcsr_norm_gershgorin, engine=eng) == got
    # maxabs
    got = dbcsr_maxabs_norm(dM, engine=eng)
    ref = float(np.max(np.abs(named))) if named.size else 0.0
    print("maxabs: %.17g against %.17g" % (got, ref))
    if cplx:
        assert abs(got - ref) <= 4 * U53 * ref
    else:
        assert got == ref
    assert dbcsr_maxabs_norm(dM, engine=eng) == got and dbcsr_norm(dM, dbcsr_norm_maxabsnorm, engine=eng) == got
    assert dbcsr_norm(dM, dbcsr_norm_frobenius, engine=eng) == dbcsr_frobenius_norm(dM, engine=eng)
    # column norms
    if symmetry == "N":
        refs, _ = sums[(1, 1)]
        counts = real_terms(np.ones(1, M.data.dtype)).size * mask.sum(axis=0)
        got_t = dbcsr_norm(dM, dbcsr_norm_column, engine=eng)
        torch.cuda.synchronize()
        assert got_t.dtype == torch.float64 and got_t.is_cuda
        got = got_t.cpu().numpy()
        check_vector(got, np.sqrt(refs), (counts + 5) * U53 * np.sqrt(refs), "column norms")
        into = torch.full_like(got_t, float("nan"))
        assert dbcsr_norm(dM, dbcsr_norm_column, norm_vector=into, engine=eng) is into
        torch.cuda.synchronize()
        assert same_bits(into.cpu().numpy(), got)


# ---- 1. sums, norms --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("which", ["mixed", "tiny", "tall70", "tall67", "gappy"])
def test_sums_and_norms(eng, dtype, which):
    M = typed(base(which), dtype, 1)
    check_everything_read_only(eng, M, to_dev(M))


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("which", ["mixed", "tall70"])
def test_sums_and_norms_of_a_data_area_that_is_not_16_byte_aligned(eng, dtype, which):
    M = typed(base(which), dtype, 1)
    check_everything_read_only(eng, M, misaligned(to_dev(M)))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_sums_and_norms_of_an_operand_with_holes(eng, dtype):
    hB, dB = with_holes(eng, typed(base("mixed"), dtype, 1), dtype)
    holes = hole_positions(hB)
    assert holes.size > 0
    dB.data[torch.as_tensor(holes[:: max(1, holes.size // 7)], device="cuda")] = 1e30   # a hole is not the matrix': it must not count
    torch.cuda.synchronize()
    check_everything_read_only(eng, hB, dB)


@pytest.mark.parametrize("dtype,symmetry", [(np.float64, "S"), (np.float32, "S"), (np.float64, "A"), (np.complex128, "H"), (np.complex128, "K")],
                         ids=["fp64_S", "fp32_S", "fp64_A", "z64_H", "z64_K"])
def test_gershgorin_of_matrices_with_symmetry(eng, dtype, symmetry):
    """the value is that of the desymmetrized matrix (formed in numpy)"""
    X = typed(symmetric_base(symmetry), dtype, 3)
    assert any(r != c for r, c in blocks_of(X)) and any(r == c for r, c in blocks_of(X))
    dX = to_dev(X)
    check_everything_read_only(eng, X, dX, symmetry)
    with pytest.raises(NotImplementedError):
        dbcsr_norm(dX, dbcsr_norm_column, engine=eng)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_nan_is_not_dropped(eng, dtype):
    """a matrix that holds a NaN reports NaN, as its sums and its Frobenius norm do: the maxima do not skip it"""
    M = typed(base("mixed"), dtype, 1)
    M.data[M.data.size // 3] = np.nan
    dM = to_dev(M)
    assert math.isnan(dbcsr_maxabs_norm(dM, engine=eng)) and math.isnan(dbcsr_gershgorin_norm(dM, engine=eng)) and math.isnan(dbcsr_frobenius_norm(dM, engine=eng))
    dM.symmetry = "N"
    assert np.count_nonzero(np.isnan(vec_sums(eng, dM, 0, 0))) == 1 and np.count_nonzero(np.isnan(vec_sums(eng, dM, 1, 1))) == 1


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_empty_matrix(eng, dtype):
    M = typed(subset(base("square"), lambda r, c: False), dtype)
    dM = to_dev(M)
    assert dbcsr_maxabs_norm(dM, engine=eng) == 0.0 and dbcsr_gershgorin_norm(dM, engine=eng) == 0.0
    n = full_len(M.row_sizes)
    for axis in (0, 1):
        assert not np.any(vec_sums(eng, dM, axis, 0)) and not np.any(vec_sums(eng, dM, axis, 1))
    cn = dbcsr_norm(dM, dbcsr_norm_column, engine=eng)
    d = dbcsr_get_diag(dM, engine=eng)
    torch.cuda.synchronize()
    assert cn.numel() == n and not np.any(cn.cpu().numpy())
    assert d.numel() == n and d.dtype == TORCH[np.dtype(dtype)] and not np.any(d.cpu().numpy())
    v = torch.ones(n, dtype=d.dtype, device="cuda")
    dbcsr_set_diag(dM, v, engine=eng)
    dbcsr_scale_by_vector(dM, v, "left", engine=eng)
    torch.cuda.synchronize()
    assert dM.nblks == 0


# ---- 2. the diagonal as a vector -----------------------------------------------------------------------------------------------------------------------
def random_vector(n, dtype, seed):
    rng = np.random.default_rng(seed)
    v = rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n)
    if is_complex(dtype):
        v = v + 1j * rng.uniform(-1.0, 1.0, n)
    return v.astype(dtype)


def diagonal_places(M):
    """positions in the data area of the diagonal elements of the diagonal blocks present, and their full-row indices"""
    ro = np.concatenate([[0], np.cumsum(M.row_sizes)])
    rows = M.rows()
    at, idx = [], []
    for b in range(M.nblks):
        r = int(rows[b])
        if int(M.col_i[b]) == r:
            m = int(M.row_sizes[r])
            at.append(M.blk_p[b] + np.arange(m) * (m + 1))
            idx.append(ro[r] + np.arange(m))
    cat = lambda xs: np.concatenate(xs).astype(np.int64) if xs else np.zeros(0, np.int64)
    return cat(at), cat(idx)


def check_diag(eng, M, dM, symmetry="N"):
    dtype = M.data.dtype
    dM.symmetry = symmetry
    n = full_len(M.row_sizes)
    got_t = dbcsr_get_diag(dM, engine=eng)
    torch.cuda.synchronize()
    got = got_t.cpu().numpy()
    assert got_t.dtype == TORCH[np.dtype(dtype)] and same_bits(got, np.ascontiguousarray(np.diagonal(dense(M))).astype(dtype))
    assert same_bits(dbcsr_get_diag(dM, engine=eng).cpu().numpy(), got)
    at, idx = diagonal_places(M)
    assert at.size and at.size < n
    v = random_vector(n, dtype, 4)
    before = (dM.index_stamp(), dM.row_p, dM.col_i, dM.blk_p, dM.data)
    area = dM.data.cpu().numpy().copy()
    dbcsr_set_diag(dM, torch.as_tensor(v).cuda(), engine=eng)
    torch.cuda.synchronize()
    assert dM.index_stamp() == before[0] and dM.row_p is before[1] and dM.col_i is before[2] and dM.blk_p is before[3] and dM.data is before[4]
    after = dM.data.cpu().numpy()
    assert same_bits(after[at], v[idx]), "the diagonal elements of the diagonal blocks present are the vector's"
    area[at] = v[idx]
    assert same_bits(after, area), "every other element of the data area is unchanged"
    again = dbcsr_get_diag(dM, engine=eng).cpu().numpy()
    want = np.zeros(n, dtype)
    want[idx] = v[idx]
    assert same_bits(again, want), "no block was created: zero where a diagonal block is missing"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("which", ["square", "tiny", "tall70", "gappy"])
def test_get_and_set_diag(eng, dtype, which):
    M = typed(base(which), dtype, 1)
    if which == "tall70":   # (the generator gave it every diagonal block: one of 70 x 70 and one of 3 x 3 stay)
        M = subset(M, lambda r, c: (r, c) != (2, 2))
    check_diag(eng, M, to_dev(M))


@pytest.mark.parametrize("dtype,symmetry", [(np.float64, "S"), (np.complex128, "H")], ids=["fp64_S", "z64_H"])
def test_get_and_set_diag_of_a_stored_triangle(eng, dtype, symmetry):
    X = typed(symmetric_base(symmetry), dtype, 3)
    X = subset(X, lambda r, c: not (r == c and r % 4 == 1))
    check_diag(eng, X, to_dev(X), symmetry)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_diag_of_an_operand_with_holes_and_a_misaligned_one(eng, dtype):
    hB, dB = with_holes(eng, typed(base("square"), dtype, 1), dtype)
    check_diag(eng, hB, dB)
    M = typed(base("square"), dtype, 1)
    check_diag(eng, M, misaligned(to_dev(M)))


# ---- 3. scale by vector --------------------------------------------------------------------------------------------------------------------------------
def scaled_area(M, v, side):
    """(the data area after the scaling, formed block by block in the data's own precision; |a| |v| per element) -- holes stay as they are"""
    ro, co = np.concatenate([[0], np.cumsum(M.row_sizes)]), np.concatenate([[0], np.cumsum(M.col_sizes)])
    area, scale = M.data.copy(), np.zeros(M.data.size)
    rows = M.rows()
    for b in range(M.nblks):
        r, c = int(rows[b]), int(M.col_i[b])
        m, n = int(M.row_sizes[r]), int(M.col_sizes[c])
        blk = M.data[M.blk_p[b]:M.blk_p[b] + m * n].reshape(n, m)   # [j][i]
        f = v[co[c]:co[c] + n][:, None] if side == "right" else v[ro[r]:ro[r] + m][None, :]
        area[M.blk_p[b]:M.blk_p[b] + m * n] = (blk * f).astype(M.data.dtype).reshape(-1)
        scale[M.blk_p[b]:M.blk_p[b] + m * n] = (np.abs(blk) * np.abs(f)).reshape(-1)
    return area, scale


def check_scale_by_vector(eng, M, dM):
    dtype = M.data.dtype
    cur = O.Bcsr(M.row_sizes, M.col_sizes, M.row_p, M.col_i, M.blk_p, dM.data.cpu().numpy().copy())   # (the whole data area, holes included)
    before = (dM.index_stamp(), dM.row_p, dM.col_i, dM.blk_p, dM.data)
    for side, sizes, seed in (("right", M.col_sizes, 5), ("left", M.row_sizes, 6)):
        v = random_vector(full_len(sizes), dtype, seed)
        ref, scale = scaled_area(cur, v, side)
        dbcsr_scale_by_vector(dM, torch.as_tensor(v).cuda(), side, engine=eng)
        torch.cuda.synchronize()
        got = dM.data.cpu().numpy()
        if is_complex(dtype):
            err = np.abs(got - ref)
            print("scale_by_vector %s: worst error %.3e of its bar" % (side, float(np.max(err / np.maximum(4 * U53 * scale, 1e-300)))))
            assert np.all(err <= 4 * U53 * scale)
            untouched = np.ones(got.size, bool)
            untouched[scale != 0] = False
            assert same_bits(got[untouched], cur.data[untouched])
        else:
            assert same_bits(got, ref), side
        cur = O.Bcsr(M.row_sizes, M.col_sizes, M.row_p, M.col_i, M.blk_p, got.copy())
    assert dM.index_stamp() == before[0] and dM.row_p is before[1] and dM.col_i is before[2] and dM.blk_p is before[3] and dM.data is before[4]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("which", ["mixed", "tiny", "tall70", "gappy"])
def test_scale_by_vector(eng, dtype, which):
    M = typed(base(which), dtype, 1)
    check_scale_by_vector(eng, M, to_dev(M))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_scale_by_vector_with_holes_and_misaligned(eng, dtype):
    hB, dB = with_holes(eng, typed(base("mixed"), dtype, 1), dtype)
    check_scale_by_vector(eng, hB, dB)
    M = typed(base("mixed"), dtype, 1)
    check_scale_by_vector(eng, M, misaligned(to_dev(M)))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_scale_left_then_right_is_d_a_d(eng, dtype):
    M = typed(base("square"), dtype, 1)
    dM = to_dev(M)
    d = random_vector(full_len(M.row_sizes), dtype, 8)
    dv = torch.as_tensor(d).cuda()
    dbcsr_scale_by_vector(dM, dv, "left", engine=eng)
    dbcsr_scale_by_vector(dM, dv, "right", engine=eng)
    torch.cuda.synchronize()
    wide = np.complex128 if is_complex(dtype) else np.float64
    A, dw = dense(M).astype(wide), d.astype(wide)
    ref = dw[:, None] * A * dw[None, :]
    scale = np.abs(dw)[:, None] * np.abs(A) * np.abs(dw)[None, :]
    got = dense(dev_to_bcsr(dM)).astype(wide)
    k = 8 if is_complex(dtype) else 2
    err = np.abs(got - ref)
    print("D A D: worst error %.3e units" % float(np.max(err / np.maximum(unit(dtype) * scale, 1e-300))))
    assert np.all(err <= k * unit(dtype) * scale)


# ---- 4. behaviour --------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_call(eng):
    A = base("mixed")
    dA = to_dev(A)
    Sq = to_dev(base("square"))
    n = full_len(base("square").row_sizes)
    ok = torch.ones(n, dtype=torch.float64, device="cuda")
    calls = eng.plan_stats()
    with pytest.raises(ValueError):
        dbcsr_norm(dA, 5, engine=eng)
    with pytest.raises(ValueError):
        dbcsr_norm(dA, 0, engine=eng)
    with pytest.raises(ValueError):
        dbcsr_get_diag(dA, engine=eng)   # not square
    with pytest.raises(ValueError):
        dbcsr_set_diag(dA, ok, engine=eng)
    with pytest.raises(ValueError):
        dbcsr_set_diag(Sq, ok[:-1].contiguous(), engine=eng)   # wrong length
    with pytest.raises(TypeError):
        dbcsr_set_diag(Sq, ok.float(), engine=eng)   # wrong data type
    with pytest.raises(TypeError):
        dbcsr_set_diag(Sq, np.ones(n), engine=eng)
    with pytest.raises(ValueError):
        dbcsr_scale_by_vector(Sq, ok, "top", engine=eng)
    with pytest.raises(ValueError):
        dbcsr_scale_by_vector(Sq, ok[:-1].contiguous(), "left", engine=eng)
    with pytest.raises(TypeError):
        dbcsr_scale_by_vector(Sq, ok.to(torch.complex128), "right", engine=eng)
    with pytest.raises(ValueError):
        dbcsr_scale_by_vector(dA, torch.ones(full_len(A.row_sizes), dtype=torch.float64, device="cuda"), "right", engine=eng)   # the rows' length for the columns
    with pytest.raises(ValueError):
        dbcsr_norm(Sq, dbcsr_norm_column, norm_vector=torch.ones(n - 1, dtype=torch.float64, device="cuda"), engine=eng)
    with pytest.raises(TypeError):
        dbcsr_norm(Sq, dbcsr_norm_column, norm_vector=torch.ones(n, dtype=torch.float32, device="cuda"), engine=eng)
    S = to_dev(symmetric_base("S"))
    for sym in ("S", "A", "H", "K"):
        S.symmetry = sym
        with pytest.raises(NotImplementedError):
            dbcsr_norm(S, dbcsr_norm_column, engine=eng)
        with pytest.raises(ValueError):
            dbcsr_scale_by_vector(S, ok, "left", engine=eng)
    for sym in ("A", "K"):
        S.symmetry = sym
        with pytest.raises(ValueError):
            dbcsr_set_diag(S, ok, engine=eng)
    S.symmetry = "X"
    for call in (lambda: dbcsr_maxabs_norm(S, engine=eng), lambda: dbcsr_gershgorin_norm(S, engine=eng), lambda: dbcsr_get_diag(S, engine=eng)):
        with pytest.raises(ValueError):
            call()
    tri = to_dev(subset(A, lambda r, c: r <= c))
    tri.symmetry = "S"
    with pytest.raises(ValueError):
        dbcsr_gershgorin_norm(tri, engine=eng)   # a matrix with symmetry that is not square
    torch.cuda.synchronize()
    assert same_bits(dev_to_bcsr(dA).data, A.data) and same_bits(dev_to_bcsr(Sq).data, base("square").data) and eng.plan_stats() == calls
    assert (dbcsr_norm_frobenius, dbcsr_norm_maxabsnorm, dbcsr_norm_gershgorin, dbcsr_norm_column) == (1, 2, 3, 4)
    assert dbcsr_amd.dbcsr_norm is dbcsr_norm and dbcsr_amd.dbcsr_scale_by_vector is dbcsr_scale_by_vector and dbcsr_amd.dbcsr_norm_column == 4


def test_c_abi_answers(eng):
    """-10 for complex_4 and unknown type codes, -1 for NULL arguments, a `what` or `side` that does not exist and shapes that do not fit, 0 and zeros for
    an empty matrix"""
    A, Sq = base("mixed"), base("square")
    dA, dS = to_dev(A), to_dev(Sq)
    a, s = dA.desc(), dS.desc()
    st = StreamHandle().ptr
    Lb, h, f64 = eng.L, eng.h, L.dbcsr_type_real_8
    out = (C.c_double * 2)()
    n = full_len(Sq.row_sizes)
    vec = torch.ones(n, dtype=torch.float64, device="cuda")
    p = vec.data_ptr()
    for code in (L.dbcsr_type_complex_4, 2, 99):
        assert Lb.dbcsr_amd_bcsr_maxabs(h, code, C.byref(s), out, st) == -10
        assert Lb.dbcsr_amd_bcsr_row_sums(h, code, C.byref(s), 0, p, n, st) == -10
        assert Lb.dbcsr_amd_bcsr_col_sums(h, code, C.byref(s), 0, 0, p, n, st) == -10
        assert Lb.dbcsr_amd_bcsr_gershgorin(h, code, C.byref(s), 0, out, st) == -10
        assert Lb.dbcsr_amd_bcsr_get_diag(h, code, C.byref(s), p, n, st) == -10
        assert Lb.dbcsr_amd_bcsr_set_diag(h, code, C.byref(s), p, n, st) == -10
        assert Lb.dbcsr_amd_bcsr_scale_by_vector(h, code, C.byref(s), p, n, 0, st) == -10
    for hh, mm in ((None, C.byref(s)), (h, None)):
        assert Lb.dbcsr_amd_bcsr_maxabs(hh, f64, mm, out, st) == -1
        assert Lb.dbcsr_amd_bcsr_row_sums(hh, f64, mm, 0, p, n, st) == -1
        assert Lb.dbcsr_amd_bcsr_col_sums(hh, f64, mm, 0, 0, p, n, st) == -1
        assert Lb.dbcsr_amd_bcsr_gershgorin(hh, f64, mm, 0, out, st) == -1
        assert Lb.dbcsr_amd_bcsr_get_diag(hh, f64, mm, p, n, st) == -1
        assert Lb.dbcsr_amd_bcsr_set_diag(hh, f64, mm, p, n, st) == -1
        assert Lb.dbcsr_amd_bcsr_scale_by_vector(hh, f64, mm, p, n, 0, st) == -1
    assert Lb.dbcsr_amd_bcsr_maxabs(h, f64, C.byref(s), None, st) == -1
    assert Lb.dbcsr_amd_bcsr_gershgorin(h, f64, C.byref(s), 0, None, st) == -1
    assert Lb.dbcsr_amd_bcsr_row_sums(h, f64, C.byref(s), 0, None, n, st) == -1
    assert Lb.dbcsr_amd_bcsr_col_sums(h, f64, C.byref(s), 0, 0, None, n, st) == -1
    assert Lb.dbcsr_amd_bcsr_get_diag(h, f64, C.byref(s), None, n, st) == -1
    assert Lb.dbcsr_amd_bcsr_set_diag(h, f64, C.byref(s), None, n, st) == -1
    assert Lb.dbcsr_amd_bcsr_scale_by_vector(h, f64, C.byref(s), None, n, 0, st) == -1
    for what in (2, -1):
        assert Lb.dbcsr_amd_bcsr_row_sums(h, f64, C.byref(s), what, p, n, st) == -1
        assert Lb.dbcsr_amd_bcsr_col_sums(h, f64, C.byref(s), what, 0, p, n, st) == -1
    assert Lb.dbcsr_amd_bcsr_scale_by_vector(h, f64, C.byref(s), p, n, 2, st) == -1
    assert Lb.dbcsr_amd_bcsr_gershgorin(h, f64, C.byref(a), 1, out, st) == -1   # symmetric needs nblkrows == nblkcols
    assert Lb.dbcsr_amd_bcsr_get_diag(h, f64, C.byref(a), p, n, st) == -1
    assert Lb.dbcsr_amd_bcsr_set_diag(h, f64, C.byref(a), p, n, st) == -1
    torch.cuda.synchronize()
    assert same_bits(dev_to_bcsr(dS).data, Sq.data) and same_bits(vec.cpu().numpy(), np.ones(n))
    # an empty matrix: 0, scalars 0, vectors of the sums and of get_diag all zero
    dE = to_dev(subset(Sq, lambda r, c: False))
    e = dE.desc()
    out[0] = 7.0
    assert Lb.dbcsr_amd_bcsr_maxabs(h, f64, C.byref(e), out, st) == 0 and out[0] == 0.0
    out[0] = 7.0
    assert Lb.dbcsr_amd_bcsr_gershgorin(h, f64, C.byref(e), 1, out, st) == 0 and out[0] == 0.0
    for call in (lambda q: Lb.dbcsr_amd_bcsr_row_sums(h, f64, C.byref(e), 1, q, n, st), lambda q: Lb.dbcsr_amd_bcsr_col_sums(h, f64, C.byref(e), 0, 1, q, n, st),
                 lambda q: Lb.dbcsr_amd_bcsr_get_diag(h, f64, C.byref(e), q, n, st)):
        buf = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
        assert call(buf.data_ptr()) == 0
        torch.cuda.synchronize()
        assert not np.any(buf.cpu().numpy())
    assert Lb.dbcsr_amd_bcsr_set_diag(h, f64, C.byref(e), p, n, st) == 0 and Lb.dbcsr_amd_bcsr_scale_by_vector(h, f64, C.byref(e), p, n, 1, st) == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_wrong_length_never_leaves_the_vector(eng, dtype):
    """too short: the elements in front are the right ones and a guard element behind the vector stays; too long: zeros behind the full length"""
    M = typed(base("square"), dtype, 1)
    dM = to_dev(M)
    n = full_len(M.row_sizes)
    d = dM.desc()
    st = StreamHandle().ptr
    tdt = TORCH[np.dtype(dtype)]
    full = {"row": vec_sums(eng, dM, 0, 0), "col": vec_sums(eng, dM, 1, 1), "diag": dbcsr_get_diag(dM, engine=eng).cpu().numpy()}
    for k in (n - 5, 1, n + 9):
        for name in ("row", "col", "diag"):
            buf = torch.full((k + 1,), -77.0, dtype=torch.float64 if name != "diag" else tdt, device="cuda")
            if name == "row":
                rc = eng.L.dbcsr_amd_bcsr_row_sums(eng.h, dM.dtype_code, C.byref(d), 0, buf.data_ptr(), k, st)
            elif name == "col":
                rc = eng.L.dbcsr_amd_bcsr_col_sums(eng.h, dM.dtype_code, C.byref(d), 1, 0, buf.data_ptr(), k, st)
            else:
                rc = eng.L.dbcsr_amd_bcsr_get_diag(eng.h, dM.dtype_code, C.byref(d), buf.data_ptr(), k, st)
            assert rc == 0
            torch.cuda.synchronize()
            got = buf.cpu().numpy()
            assert got[k] == -77.0, "the guard element behind the vector"
            assert same_bits(got[:min(k, n)], full[name][:min(k, n)]) and not np.any(got[n:k])
    # a vector that is too short for set_diag / scale_by_vector: read below its length only; the elements it has no entry for stay as they are
    k = n - 5
    v = random_vector(n, dtype, 9)
    short = torch.as_tensor(v[:k].copy()).cuda()
    area = dM.data.cpu().numpy().copy()
    assert eng.L.dbcsr_amd_bcsr_set_diag(eng.h, dM.dtype_code, C.byref(d), short.data_ptr(), k, st) == 0
    torch.cuda.synchronize()
    at, idx = diagonal_places(M)
    area[at[idx < k]] = v[idx[idx < k]]
    assert same_bits(dM.data.cpu().numpy(), area)
    cur = O.Bcsr(M.row_sizes, M.col_sizes, M.row_p, M.col_i, M.blk_p, area)
    padded = v.copy()
    padded[k:] = 1
    ref, scale = scaled_area(cur, padded, "right")
    assert eng.L.dbcsr_amd_bcsr_scale_by_vector(eng.h, dM.dtype_code, C.byref(d), short.data_ptr(), k, 1, st) == 0
    torch.cuda.synchronize()
    got = dM.data.cpu().numpy()
    if is_complex(dtype):
        assert np.all(np.abs(got - ref) <= 4 * U53 * scale)
    else:
        assert same_bits(got, ref)


def product_bar(got, alpha, Ad, Bd, bar=1e-10):
    R, scale = alpha * (Ad @ Bd), abs(alpha) * (np.abs(Ad) @ np.abs(Bd))
    G = dense(got)
    mask = pattern_mask(got)
    assert np.all(np.abs(G - R)[mask] <= bar * scale[mask])
    assert not np.any(R[~mask]), "a block of the product is missing"


def test_norms_and_vectors_between_multiplies_keep_the_plan(monkeypatch):
    monkeypatch.delenv("DBCSR_AMD_MM_PLAN", raising=False)
    eng = MultiplyEngine()
    sizes = O.make_block_sizes(200, [1, 13, 1, 5, 1, 7])
    A = typed(O.make_random_matrix(sizes, sizes, 0.5, O.RANDMAT_SEED_INIT + 31), np.float64, 5)
    B = typed(O.make_random_matrix(sizes, sizes, 0.6, O.RANDMAT_SEED_INIT + 32), np.float64, 6)
    dA, dB = to_dev(A), to_dev(B)
    dC = to_dev(subset(A, lambda r, c: False))
    dbcsr_multiply("N", "N", 1.0, dA, dB, 0.0, dC, engine=eng)
    assert eng.plan_stats() == (0, 1)
    ones = torch.ones(full_len(sizes), dtype=torch.float64, device="cuda")
    for it in range(1, 3):
        stamps = (dA.index_stamp(), dC.index_stamp())
        dbcsr_gershgorin_norm(dC, engine=eng)
        dbcsr_gershgorin_norm(dA, engine=eng)
        dA.symmetry = "S"
        dbcsr_gershgorin_norm(dA, engine=eng)   # (row and column sums: the per-column lists are built in the algebra's own buffers)
        dA.symmetry = "N"
        dbcsr_maxabs_norm(dA, engine=eng)
        dbcsr_norm(dA, dbcsr_norm_column, engine=eng)
        dbcsr_set_diag(dA, dbcsr_get_diag(dA, engine=eng), engine=eng)
        dbcsr_scale_by_vector(dA, ones, "left", engine=eng)
        dbcsr_scale_by_vector(dA, ones, "right", engine=eng)
        assert (dA.index_stamp(), dC.index_stamp()) == stamps
        dbcsr_multiply("N", "N", 1.0, dA, dB, 0.0, dC, engine=eng)
        assert eng.plan_stats() == (it, 1), "a multiply after norms and vector operations must reuse its plan"
    torch.cuda.synchronize()
    assert same_bits(dev_to_bcsr(dA).data, A.data)   # (the diagonal read and written back, a vector of ones: not a bit changed)
    product_bar(dev_to_bcsr(dC), 1.0, dense(A), dense(B))


# ---- 5. a whole sign iteration on the device --------------------------------------------------------------------------------------------------------
def test_sign_iteration_on_the_device(eng):
    """X <- A / min(||A||_F, ||A||_gershgorin), then X <- X (3 I - X^2) / 2 with dbcsr_multiply, dbcsr_add_on_diag, dbcsr_scale, dbcsr_add only -- no
    matrix leaves the device before the end.  Reference: the same iteration in numpy with numpy's two norms; it must itself converge."""
    n = 96
    rng = np.random.default_rng(17)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam = 2.7 * rng.uniform(0.3, 1.0, n) * np.repeat([1.0, -1.0], n // 2)
    A = (Q * lam) @ Q.T
    A = 0.5 * (A + A.T)
    sizes = O.make_block_sizes(n, [1, 13, 1, 5, 1, 7])
    assert int(sizes.sum()) == n and len(set(sizes.tolist())) > 2
    hA = from_dense(A, sizes, sizes, np.float64)
    assert np.array_equal(dense(hA), A)
    # the reference, and its own convergence
    eye = np.eye(n)
    X = A / min(np.linalg.norm(A, "fro"), np.max(np.sum(np.abs(A), axis=1)))
    steps = None
    for k in range(1, 41):
        X = 0.5 * X @ (3.0 * eye - X @ X)
        if np.linalg.norm(X @ X - eye, "fro") < 1e-12:
            steps = k
            break
    assert steps is not None, "the reference iteration itself must reach ||X^2 - I||_F < 1e-12 within 40 steps"
    w, V = np.linalg.eigh(A)
    assert np.max(np.abs(X - (V * np.sign(w)) @ V.T)) < 1e-12
    # the device
    dX = to_dev(hA)
    fro, ger = dbcsr_frobenius_norm(dX, engine=eng), dbcsr_gershgorin_norm(dX, engine=eng)
    assert abs(fro - np.linalg.norm(A, "fro")) <= 1e-13 * fro and abs(ger - np.max(np.sum(np.abs(A), axis=1))) <= 1e-13 * ger
    dbcsr_scale(dX, 1.0 / min(fro, ger), engine=eng)
    empty = subset(hA, lambda r, c: False)
    for _ in range(steps):
        dY = to_dev(empty)
        dbcsr_multiply("N", "N", 1.0, dX, dX, 0.0, dY, engine=eng)     # Y = X X
        dbcsr_scale(dY, -1.0, engine=eng)                              # Y <- -Y
        dbcsr_add_on_diag(dY, 3.0, engine=eng)                         # Y <- 3 I - Y
        dN = to_dev(empty)
        dbcsr_multiply("N", "N", 0.5, dX, dY, 0.0, dN, engine=eng)     # X' = X Y / 2
        dX = dN
    torch.cuda.synchronize()
    got = dense(dev_to_bcsr(dX))
    err = float(np.max(np.abs(got - X)))
    print("sign iteration: %d steps, max element error %.3e" % (steps, err))
    assert err <= 1e-10
    # ... and dbcsr_add closes the loop on the device too: X^2 - I is small
    dY = to_dev(empty)
    dbcsr_multiply("N", "N", 1.0, dX, dX, 0.0, dY, engine=eng)
    dI = to_dev(empty)
    dbcsr_add_on_diag(dI, 1.0, engine=eng)
    dbcsr_add(dY, dI, 1.0, -1.0, engine=eng)
    assert dbcsr_frobenius_norm(dY, engine=eng) < 1e-10
