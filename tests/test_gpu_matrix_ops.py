"""Matrix algebra between multiplies on the device (dbcsr_amd/operations.py, the add / diag / trace / dot / norm2 entries of
include/dbcsr_amd_mm.h, kernels of dbcsr_amd/csrc/mm_algebra.h): dbcsr_add, dbcsr_scale, dbcsr_add_on_diag, dbcsr_trace, dbcsr_dot,
dbcsr_frobenius_norm for float64, float32 and complex128.

Reference for VALUES: numpy on the blocks / dense scatter (oracle.Bcsr.to_dense) in the data's own precision.  Reference for the INDEX:
the union pattern built here from the two indices -- sorted block columns per row, blk_p the running sum of the block sizes.

Bars, derived (u = 2^-53 for float64 / complex128, 2^-24 for float32):
  add, per element   |got - ref| <= 4u (|alpha| |a| + |beta| |b|), 8u with moduli for complex data: fl(fl(alpha a) + fl(beta b)) and the contracted
                     FMA form are both within 2u of that scale of the exact value, and so is the reference; rounding a double scalar to float32
                     adds u; the complex product a factor below 2.  A scalar that is exactly 1 multiplies nothing: with alpha = beta = 1 the
                     WHOLE result is compared bit for bit (a + b where both have the block, the source block where one has it).
  scale              <= 2u |alpha| |x| (4u complex); alpha = 1: bit-identical.
  trace, dot, norm^2 |got - ref| <= (n + 4) 2^-53 sum|term|, n terms, ref = math.fsum of the terms formed in float64 (float32 products are exact
                     in double; a complex |x|^2 is two terms): holds for any summation order in double.
  norm               root of that value, one more 2^-53 relative: (n + 5) 2^-53 * norm.
  multiply steps of the sign iteration: the project's 1e-10, against the dense product's own scale |alpha| (|A| |B|) per element (an iterate has
                     both signs: a strict relative error per element would measure cancellation, not the kernel).
Matrices: the oracle's generator (perf_case / make_random_matrix) with the block-size mixes [1, 13, 1, 5] x [1, 23, 1, 4] at 230 x 260, and one of
tiny blocks ([1, 1, 1, 3], 76 block columns, fill 0.9: a row's bitmap spans three words and holds more than 64 blocks)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from dbcsr_amd import lib as L
from dbcsr_amd.matrix import DbcsrMatrix, StreamHandle
from dbcsr_amd.multiply import MultiplyEngine, dbcsr_multiply
from dbcsr_amd.operations import dbcsr_add, dbcsr_add_on_diag, dbcsr_dot, dbcsr_frobenius_norm, dbcsr_scale, dbcsr_trace
from oracle import oracle as O
from tests.gpu_util import dev_to_bcsr, to_dev

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32, np.complex128]
IDS = ["fp64", "fp32", "z64"]
U53 = 2.0 ** -53


def unit(dtype):
    return 2.0 ** -24 if np.dtype(dtype) == np.float32 else U53


def factor(dtype):
    return 2.0 if np.dtype(dtype).kind == "c" else 1.0


@pytest.fixture(scope="module")
def eng():
    return MultiplyEngine()


# ---- host helpers: a matrix as a dict of blocks -------------------------------------------------------------------------------------------
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
    if np.dtype(dtype).kind == "c":
        rng = np.random.default_rng(seed)
        data = M.data * rng.choice([-1.0, 1.0], M.data.size) + 1j * rng.uniform(-1.0, 1.0, M.data.size)
    else:
        data = M.data - 0.4   # (both signs: sums cancel)
    return O.Bcsr(M.row_sizes, M.col_sizes, M.row_p, M.col_i, M.blk_p, data.astype(dtype))


def dense(M):
    if M.data.dtype.kind == "c":
        re = O.Bcsr(M.row_sizes, M.col_sizes, M.row_p, M.col_i, M.blk_p, np.ascontiguousarray(M.data.real))
        im = O.Bcsr(M.row_sizes, M.col_sizes, M.row_p, M.col_i, M.blk_p, np.ascontiguousarray(M.data.imag))
        return re.to_dense() + 1j * im.to_dense()
    return M.to_dense()


def same_bits(x, y):
    return x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


def same_index(got, ref):
    assert np.array_equal(got.row_p, ref.row_p), "row_p"
    assert np.array_equal(got.col_i, ref.col_i), "col_i"
    assert np.array_equal(got.blk_p, ref.blk_p), "blk_p"


def times(s, x, dtype):
    """s * x as the data type computes it; s == 1 multiplies nothing"""
    return x if s == 1 else (np.asarray(s, dtype) * x).astype(dtype)


def reference_add(A, B, alpha, beta):
    """(result, scale): alpha A + beta B on the union pattern in the data's own precision (beta == 0: A's pattern), and per element
    |alpha| |a| + |beta| |b|"""
    dtype = A.data.dtype
    ba, bb = blocks_of(A), ({} if beta == 0 else blocks_of(B))
    out, scale = {}, {}
    for k in set(ba) | set(bb):
        if k in ba and k in bb:
            out[k] = (times(alpha, ba[k], dtype) + times(beta, bb[k], dtype)).astype(dtype)
            scale[k] = abs(alpha) * np.abs(ba[k]) + abs(beta) * np.abs(bb[k])
        elif k in ba:
            out[k], scale[k] = times(alpha, ba[k], dtype), abs(alpha) * np.abs(ba[k])
        else:
            out[k], scale[k] = times(beta, bb[k], dtype), abs(beta) * np.abs(bb[k])
    return from_blocks(A.row_sizes, A.col_sizes, out, dtype), from_blocks(A.row_sizes, A.col_sizes, scale, np.float64).data


def check_add(eng, A, B, alpha, beta, expect_same=False, dA=None, dB=None):
    dA = to_dev(A) if dA is None else dA
    dB = to_dev(B) if dB is None else dB
    before = (dA.index_stamp(), dA.row_p, dA.col_i, dA.blk_p, dA.data)
    same = dbcsr_add(dA, dB, alpha, beta, engine=eng)
    torch.cuda.synchronize()
    assert same == expect_same
    if expect_same:   # in place: the same tensor objects, the same stamp
        assert dA.index_stamp() == before[0]
        assert dA.row_p is before[1] and dA.col_i is before[2] and dA.blk_p is before[3] and dA.data is before[4]
    got = dev_to_bcsr(dA)
    ref, scale = reference_add(A, B, alpha, beta)
    same_index(got, ref)
    assert dA.packed and got.data.size == ref.data.size
    dtype = A.data.dtype
    if alpha == 1 and (beta == 1 or beta == 0):
        assert same_bits(got.data, ref.data), "scalars of exactly 1: the result is a + b / the source block, bit for bit"
    err, lim = np.abs(got.data - ref.data), 4 * factor(dtype) * unit(dtype) * scale
    worst = int(np.argmax(err - lim)) if err.size else 0
    assert np.all(err <= lim), "worst element: error %.3e against a bar of %.3e" % (float(err[worst]), float(lim[worst]))
    return dA, got


def scalars(dtype):
    return (0.75 - 0.5j, -1.25 + 2j) if np.dtype(dtype).kind == "c" else (0.75, -1.25)


@functools.lru_cache(maxsize=None)
def base_pair():
    """two matrices of the same sizes with independent random patterns (fills 0.3 and 0.5)"""
    Cm = O.perf_case(230, 260, 200, 0.5, 0.5, 0.7, [1, 13, 1, 5], [1, 23, 1, 4], [1, 7, 1, 32])[2]
    B = O.make_random_matrix(Cm.row_sizes, Cm.col_sizes, 0.5, O.RANDMAT_SEED_INIT + 11)
    return Cm, B


@functools.lru_cache(maxsize=None)
def tiny_pair():
    Cm = O.perf_case(150, 150, 150, 0.1, 0.1, 0.1, [1, 1, 1, 3], [1, 1, 1, 3], [1, 1, 1, 3])[2]
    B = O.make_random_matrix(Cm.row_sizes, Cm.col_sizes, 0.1, O.RANDMAT_SEED_INIT + 12)
    assert Cm.nbc >= 70 and np.max(np.diff(Cm.row_p)) > 64
    return Cm, B


def subset(M, keep):
    """M without the blocks for which keep(r, c) is false (packed again)"""
    return from_blocks(M.row_sizes, M.col_sizes, {k: v for k, v in blocks_of(M).items() if keep(*k)}, M.data.dtype)


# ---- 1. add: patterns -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("which", ["mixed", "tiny"])
def test_add_independent_patterns(eng, dtype, which):
    A, B = (base_pair if which == "mixed" else tiny_pair)()
    A, B = typed(A, dtype, 1), typed(B, dtype, 2)
    only_a, only_b = set(blocks_of(A)) - set(blocks_of(B)), set(blocks_of(B)) - set(blocks_of(A))
    assert only_a and only_b and set(blocks_of(A)) & set(blocks_of(B))
    al, be = scalars(dtype)
    check_add(eng, A, B, al, be)
    check_add(eng, A, B, 1, 1)       # bit for bit, single-operand blocks included
    check_add(eng, A, B, 1, be)      # blocks A alone has: bit-identical copies ...
    _, got = check_add(eng, A, B, al, 1)
    bg, bb = blocks_of(got), blocks_of(B)
    assert all(same_bits(bg[k], bb[k]) for k in only_b)   # ... and those B alone has


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_add_identical_patterns_in_place(eng, dtype):
    A = typed(base_pair()[0], dtype, 1)
    B = O.Bcsr(A.row_sizes, A.col_sizes, A.row_p, A.col_i, A.blk_p, typed(base_pair()[0], dtype, 3).data[::-1].copy())
    al, be = scalars(dtype)
    check_add(eng, A, B, 1, 1, expect_same=True)
    check_add(eng, A, B, al, be, expect_same=True)
    check_add(eng, A, B, 0, be, expect_same=True)
    # the C ABI says so itself, and refuses nothing: same_pattern with the counts of A
    dA, dB = to_dev(A), to_dev(B)
    a, b = dA.desc(), dB.desc()
    row_p = torch.empty(dA.nblkrows + 1, dtype=torch.int32, device="cuda")
    nb, nz, same = C.c_int64(), C.c_int64(), C.c_int32()
    assert eng.L.dbcsr_amd_bcsr_add_count(eng.h, C.byref(a), C.byref(b), 0, row_p.data_ptr(), C.byref(nb), C.byref(nz), C.byref(same), StreamHandle().ptr) == 0
    assert (same.value, nb.value, nz.value) == (1, A.nblks, A.data.size)
    assert np.array_equal(row_p.cpu().numpy(), A.row_p)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_add_subsets_and_empty_operands(eng, dtype):
    A, B = typed(base_pair()[0], dtype, 1), typed(base_pair()[1], dtype, 2)
    al, be = scalars(dtype)
    part = subset(B, lambda r, c: (r + 2 * c) % 3 != 0)
    assert 0 < part.nblks < B.nblks
    check_add(eng, part, B, al, be)       # A inside B
    check_add(eng, B, part, al, be)       # B inside A
    check_add(eng, B, part, 1, 1)
    none = subset(A, lambda r, c: False)
    check_add(eng, none, B, al, be)       # A empty
    check_add(eng, none, B, 1, 1)
    check_add(eng, A, none, al, be)       # B empty
    check_add(eng, none, none, al, be, expect_same=True)   # both empty
    # empty block rows, in one operand, in the other and in both
    Ar = subset(A, lambda r, c: r % 4 not in (0, 1))
    Br = subset(B, lambda r, c: r % 4 not in (1, 2) and r < B.nbr - 2)
    check_add(eng, Ar, Br, al, be)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_add_zero_scalars(eng, dtype):
    A, B = typed(base_pair()[0], dtype, 1), typed(base_pair()[1], dtype, 2)
    al, be = scalars(dtype)
    _, got = check_add(eng, A, B, al, 0)          # beta == 0: A's pattern, B ignored
    assert got.nblks == A.nblks
    check_add(eng, A, B, 1, 0)
    _, got = check_add(eng, A, B, 0, be)          # alpha == 0: A's blocks stay stored
    assert set(blocks_of(got)) == set(blocks_of(A)) | set(blocks_of(B))
    _, got = check_add(eng, A, subset(B, lambda r, c: False), 0, be)
    assert got.nblks == A.nblks and not np.any(got.data)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_add_operand_with_holes(eng, dtype):
    """B = the result of an in-place filter: A's pattern, the kept blocks where they were, holes between them"""
    A = typed(base_pair()[0], dtype, 1)
    extra = {k: (v * 1e-9).astype(dtype) for k, v in blocks_of(typed(base_pair()[1], dtype, 2)).items() if k not in blocks_of(A)}
    full = dict(blocks_of(typed(base_pair()[0], dtype, 5)))
    full.update(extra)
    Bfull = from_blocks(A.row_sizes, A.col_sizes, full, dtype)
    dBfull = to_dev(Bfull)
    dB = eng.filtered(dBfull, 1e-6, in_place=True)
    torch.cuda.synchronize()
    assert not dB.packed and dB.data is dBfull.data and dB.nblks == A.nblks
    hB = dev_to_bcsr(dB)
    assert np.array_equal(hB.col_i, A.col_i) and np.array_equal(hB.row_p, A.row_p) and not np.array_equal(hB.blk_p, A.blk_p)
    Bpacked = from_blocks(A.row_sizes, A.col_sizes, blocks_of(hB), dtype)
    al, be = scalars(dtype)
    for x, y in ((al, be), (1, 1)):
        _, holes = check_add(eng, A, hB, x, y, dB=dB)                          # the per-block path ...
        _, packed = check_add(eng, A, Bpacked, x, y, expect_same=True)         # ... equals the flat pass bit for bit
        assert same_bits(holes.data, packed.data)
    # ... and the operand with holes on the left: the result is packed
    _, got = check_add(eng, hB, A, al, be, dA=DbcsrMatrix(dB.row_blk_size, dB.col_blk_size, dB.row_p, dB.col_i, dB.blk_p, dB.data, nze=dB.nze))
    # reductions go by the index too
    check_norm(eng, dB, real_terms(Bpacked.data))
    if np.dtype(dtype).kind != "c":
        check_sum(dbcsr_dot(dB, to_dev(A), engine=eng), Bpacked.data.astype(np.float64) * A.data.astype(np.float64))


def symmetric_pair(dtype, symmetry):
    sizes = O.make_block_sizes(200, [1, 13, 1, 5, 1, 7])
    kind = "S" if symmetry in ("S", "H") else "A"
    X = O.make_random_matrix_symmetric(sizes, 0.6, O.RANDMAT_SEED_INIT + 21, kind)
    Y = O.make_random_matrix_symmetric(sizes, 0.4, O.RANDMAT_SEED_INIT + 22, kind)
    return typed(X, dtype, 3), typed(Y, dtype, 4)


def desymmetrized_dense(M, symmetry):
    """the full matrix of a stored triangle, in numpy: block (c, r) = twin of block (r, c)"""
    D = dense(M)
    off = dense(subset(M, lambda r, c: r != c))
    T = off.T
    if symmetry in ("H", "K"):
        T = T.conj()
    return D + (T if symmetry in ("S", "H") else -T)


@pytest.mark.parametrize("dtype,symmetry", [(np.float64, "S"), (np.float32, "S"), (np.complex128, "H"), (np.complex128, "S")], ids=["fp64_S", "fp32_S", "z64_H", "z64_S"])
def test_add_matrices_with_symmetry(eng, dtype, symmetry):
    X, Y = symmetric_pair(dtype, symmetry)
    dX, dY = to_dev(X), to_dev(Y)
    dX.symmetry = dY.symmetry = symmetry
    al, be = (0.75, -1.25)   # (real scalars keep a hermitian matrix hermitian)
    check_add(eng, X, Y, al, be, dA=dX, dB=dY)   # stored triangles are added as they are
    assert dX.symmetry == symmetry
    got = dev_to_bcsr(dX)
    assert np.all(got.rows() <= got.col_i)


def test_add_refuses_mismatches_before_any_call(eng):
    A, B = base_pair()
    dA, dB = to_dev(A), to_dev(B)
    calls = eng.plan_stats()
    with pytest.raises(TypeError):
        dbcsr_add(dA, to_dev(typed(B, np.float32)), engine=eng)
    with pytest.raises(TypeError):
        dbcsr_add(dA, dB, 1.0 + 1j, 1.0, engine=eng)
    with pytest.raises(TypeError):
        dbcsr_add(dA, dB, 1.0, 2j, engine=eng)
    with pytest.raises(TypeError):
        dbcsr_scale(dA, 2j, engine=eng)
    S = to_dev(symmetric_pair(np.float64, "S")[0])
    S.symmetry = "S"
    N = to_dev(symmetric_pair(np.float64, "S")[1])
    with pytest.raises(ValueError, match="NYI"):
        dbcsr_add(N, S, engine=eng)
    other = O.make_random_matrix(A.row_sizes[::-1].copy(), A.col_sizes, 0.5, O.RANDMAT_SEED_INIT + 13)
    with pytest.raises(ValueError):
        dbcsr_add(dA, to_dev(other), engine=eng)
    fewer = O.make_random_matrix(A.row_sizes, A.col_sizes[:-1].copy(), 0.5, O.RANDMAT_SEED_INIT + 13)
    with pytest.raises(ValueError):
        dbcsr_add(dA, to_dev(fewer), engine=eng)
    for sym in ("A", "K"):
        S.symmetry = sym
        with pytest.raises(ValueError):
            dbcsr_add_on_diag(S, 1.0, engine=eng)
    with pytest.raises(ValueError):
        dbcsr_add_on_diag(dA, 1.0, engine=eng)   # not square
    Z = to_dev(typed(symmetric_pair(np.float64, "S")[0], np.complex128))
    with pytest.raises(NotImplementedError):
        dbcsr_dot(Z, Z, engine=eng)
    torch.cuda.synchronize()
    assert same_bits(dev_to_bcsr(dA).data, A.data) and eng.plan_stats() == calls


def test_c_abi_answers(eng):
    """-10 for complex_4 and unknown type codes (the complex dot included), -1 for NULL arguments, mismatched dimensions and an aliased dst"""
    A, B = base_pair()
    dA, dB = to_dev(A), to_dev(B)
    a, b = dA.desc(), dB.desc()
    st = StreamHandle().ptr
    Lb = eng.L
    one, out = (C.c_double * 2)(1.0, 0.0), (C.c_double * 2)()
    row_p = torch.empty(dA.nblkrows + 1, dtype=torch.int32, device="cuda")
    nb, nz, same = C.c_int64(), C.c_int64(), C.c_int32()
    count = lambda x, y: Lb.dbcsr_amd_bcsr_add_count(eng.h, x, y, 0, row_p.data_ptr(), C.byref(nb), C.byref(nz), C.byref(same), st)
    for code in (L.dbcsr_type_complex_4, 2, 99):
        assert Lb.dbcsr_amd_bcsr_trace(eng.h, code, C.byref(a), out, st) in (-10, -1)   # (this matrix is not square: -1 may come first)
        assert Lb.dbcsr_amd_bcsr_norm2(eng.h, code, C.byref(a), 0, out, st) == -10
        assert Lb.dbcsr_amd_bcsr_dot(eng.h, code, C.byref(a), C.byref(b), 0, out, st) == -10
        assert Lb.dbcsr_amd_bcsr_diag_fill(eng.h, code, one, C.byref(a), st) in (-10, -1)
        assert count(C.byref(a), C.byref(b)) == 0
        assert Lb.dbcsr_amd_bcsr_add_apply(eng.h, code, one, C.byref(a), one, C.byref(b), C.byref(a), st) == -10
    assert Lb.dbcsr_amd_bcsr_dot(eng.h, L.dbcsr_type_complex_8, C.byref(a), C.byref(b), 0, out, st) == -10
    assert count(None, C.byref(b)) == -1 and count(C.byref(a), None) == -1
    assert Lb.dbcsr_amd_bcsr_add_count(eng.h, C.byref(a), C.byref(b), 0, None, C.byref(nb), C.byref(nz), C.byref(same), st) == -1
    assert Lb.dbcsr_amd_bcsr_norm2(eng.h, L.dbcsr_type_real_8, None, 0, out, st) == -1
    assert Lb.dbcsr_amd_bcsr_norm2(None, L.dbcsr_type_real_8, C.byref(a), 0, out, st) == -1
    assert Lb.dbcsr_amd_bcsr_trace(eng.h, L.dbcsr_type_real_8, C.byref(a), None, st) == -1
    assert Lb.dbcsr_amd_bcsr_trace(eng.h, L.dbcsr_type_real_8, C.byref(a), out, st) == -1   # nblkrows != nblkcols
    dShort = to_dev(O.make_random_matrix(A.row_sizes[:-1].copy(), A.col_sizes, 0.5, O.RANDMAT_SEED_INIT + 13))
    short = dShort.desc()
    assert count(C.byref(a), C.byref(short)) == -1
    assert Lb.dbcsr_amd_bcsr_dot(eng.h, L.dbcsr_type_real_8, C.byref(a), C.byref(short), 0, out, st) == -1
    # a union add is not done in place; an apply without a count is refused
    assert count(C.byref(a), C.byref(b)) == 0 and same.value == 0
    assert Lb.dbcsr_amd_bcsr_add_apply(eng.h, L.dbcsr_type_real_8, one, C.byref(a), one, C.byref(b), C.byref(a), st) == -1
    assert Lb.dbcsr_amd_bcsr_add_apply(eng.h, L.dbcsr_type_real_8, one, C.byref(a), one, C.byref(b), C.byref(a), st) == -1
    torch.cuda.synchronize()
    assert same_bits(dev_to_bcsr(dA).data, A.data)


# ---- 2. scale ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_scale(eng, dtype):
    A = typed(base_pair()[0], dtype, 1)
    dA = to_dev(A)
    stamp = dA.index_stamp()
    dbcsr_scale(dA, 1, engine=eng)
    torch.cuda.synchronize()
    assert same_bits(dev_to_bcsr(dA).data, A.data)
    al = scalars(dtype)[1]
    dbcsr_scale(dA, al, engine=eng)
    torch.cuda.synchronize()
    got = dev_to_bcsr(dA)
    same_index(got, A)
    assert dA.index_stamp() == stamp
    ref = times(al, A.data, dtype)
    assert np.all(np.abs(got.data - ref) <= 2 * factor(dtype) * unit(dtype) * abs(al) * np.abs(A.data))


# ---- 3. reductions ----------------------------------------------------------------------------------------------------------------------------
def real_terms(x):
    """the float64 terms of sum |x|^2: a complex element gives two"""
    x = np.asarray(x)
    if x.dtype.kind == "c":
        return np.concatenate([x.real.astype(np.float64) ** 2, x.imag.astype(np.float64) ** 2])
    return x.astype(np.float64) ** 2


def check_sum(got, terms):
    terms = np.asarray(terms, np.float64)
    ref = math.fsum(terms.tolist())
    bar = (terms.size + 4) * U53 * math.fsum(np.abs(terms).tolist())
    assert abs(got - ref) <= bar, (got, ref, bar)
    return ref


def check_norm(eng, dM, terms):
    """the norm against the root of the exact sum, and twice the same bits"""
    got = dbcsr_frobenius_norm(dM, engine=eng)
    ref = math.sqrt(math.fsum(np.asarray(terms, np.float64).tolist()))
    assert abs(got - ref) <= (len(terms) + 5) * U53 * ref, (got, ref)
    out = (C.c_double * 2)()
    d = dM.desc()
    assert eng.L.dbcsr_amd_bcsr_norm2(eng.h, dM.dtype_code, C.byref(d), 0 if dM.symmetry == "N" else 1, out, StreamHandle().ptr) == 0
    check_sum(out[0], terms)
    assert dbcsr_frobenius_norm(dM, engine=eng) == got and math.sqrt(out[0]) == got
    return got


def square_pair(dtype):
    sizes = O.make_block_sizes(200, [1, 13, 1, 5, 1, 7])
    X = O.make_random_matrix(sizes, sizes, 0.5, O.RANDMAT_SEED_INIT + 31)
    Y = O.make_random_matrix(sizes, sizes, 0.6, O.RANDMAT_SEED_INIT + 32)
    return typed(X, dtype, 5), typed(Y, dtype, 6)


def check_trace(eng, dM, M):
    got = dbcsr_trace(dM, engine=eng)
    diag = np.concatenate([v.reshape(int(M.col_sizes[c]), int(M.row_sizes[r])).diagonal() for (r, c), v in sorted(blocks_of(M).items()) if r == c] or
                          [np.zeros(0, M.data.dtype)])
    if M.data.dtype.kind == "c":
        assert isinstance(got, complex)
        check_sum(got.real, diag.real)
        check_sum(got.imag, diag.imag)
    else:
        assert isinstance(got, float)
        check_sum(got, diag)
    again = dbcsr_trace(dM, engine=eng)
    assert again == got and math.copysign(1, again.real) == math.copysign(1, got.real)
    return got


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("which", ["mixed", "tiny"])
def test_trace_dot_norm(eng, dtype, which):
    if which == "mixed":
        X, Y = square_pair(dtype)
    else:
        X, Y = (typed(M, dtype, 8 + i) for i, M in enumerate(tiny_pair()))
    dX, dY = to_dev(X), to_dev(Y)
    assert any(r == c for r, c in blocks_of(X)) and any((r, r) not in blocks_of(X) for r in range(X.nbr))
    check_trace(eng, dX, X)
    check_norm(eng, dX, real_terms(X.data))
    if np.dtype(dtype).kind == "c":
        with pytest.raises(NotImplementedError):
            dbcsr_dot(dX, dY, engine=eng)
        return
    bx, by = blocks_of(X), blocks_of(Y)
    both = sorted(set(bx) & set(by))
    assert both and len(both) < min(len(bx), len(by))
    terms = np.concatenate([bx[k].astype(np.float64) * by[k].astype(np.float64) for k in both])
    got = dbcsr_dot(dX, dY, engine=eng)
    ref = check_sum(got, terms)
    assert abs(ref - np.sum(dense(X).astype(np.float64) * dense(Y).astype(np.float64))) <= 1e-9 * np.sum(np.abs(terms))   # = trace(X^T Y)
    assert dbcsr_dot(dX, dY, engine=eng) == got
    check_sum(dbcsr_dot(dX, dX, engine=eng), real_terms(X.data))
    empty = to_dev(subset(X, lambda r, c: False))
    assert dbcsr_dot(dX, empty, engine=eng) == 0.0 and dbcsr_trace(empty, engine=eng) == 0.0 and dbcsr_frobenius_norm(empty, engine=eng) == 0.0


@pytest.mark.parametrize("dtype,symmetry", [(np.float64, "S"), (np.float32, "S"), (np.float64, "A"), (np.complex128, "H"), (np.complex128, "K")],
                         ids=["fp64_S", "fp32_S", "fp64_A", "z64_H", "z64_K"])
def test_reductions_of_matrices_with_symmetry(eng, dtype, symmetry):
    """the value is that of the desymmetrized matrix (formed in numpy), within the same bars"""
    X, Y = symmetric_pair(dtype, symmetry)
    dX, dY = to_dev(X), to_dev(Y)
    dX.symmetry = dY.symmetry = symmetry
    full = desymmetrized_dense(X, symmetry)
    mask = desymmetrized_dense(O.Bcsr(X.row_sizes, X.col_sizes, X.row_p, X.col_i, X.blk_p, np.ones(X.data.size)), "S") != 0
    check_norm(eng, dX, real_terms(full[mask]))
    if symmetry == "S" and np.dtype(dtype).kind != "c":
        fy = desymmetrized_dense(Y, symmetry)
        my = desymmetrized_dense(O.Bcsr(Y.row_sizes, Y.col_sizes, Y.row_p, Y.col_i, Y.blk_p, np.ones(Y.data.size)), "S") != 0
        terms = (full.astype(np.float64) * fy.astype(np.float64))[mask & my]
        got = dbcsr_dot(dX, dY, engine=eng)
        check_sum(got, terms)
        assert dbcsr_dot(dX, dY, engine=eng) == got
        dY.symmetry = "N"
        with pytest.raises(ValueError):
            dbcsr_dot(dX, dY, engine=eng)
    if symmetry in ("S", "H"):
        check_trace(eng, dX, X)


# ---- 4. add_on_diag -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,symmetry", [(np.float64, "N"), (np.float32, "N"), (np.complex128, "N"), (np.float64, "S"), (np.complex128, "H")],
                         ids=["fp64", "fp32", "z64", "fp64_S", "z64_H"])
@pytest.mark.parametrize("diag", ["all", "some", "none"])
def test_add_on_diag(eng, dtype, symmetry, diag):
    X = square_pair(dtype)[0] if symmetry == "N" else symmetric_pair(dtype, symmetry)[0]
    blocks = {k: v for k, v in blocks_of(X).items() if k[0] != k[1] or diag == "all" or (diag == "some" and k[0] % 2)}
    if diag == "all":
        rng = np.random.default_rng(9)
        for r in range(X.nbr):
            blocks.setdefault((r, r), rng.uniform(-1, 1, int(X.row_sizes[r]) ** 2).astype(dtype))
    A = from_blocks(X.row_sizes, X.col_sizes, blocks, dtype)
    have = {r for r, c in blocks if r == c}
    assert {"all": len(have) == A.nbr, "some": 0 < len(have) < A.nbr, "none": not have}[diag]
    alpha = (3.0 if symmetry == "H" else 1.5 - 0.5j) if np.dtype(dtype).kind == "c" else -1.5
    dA = to_dev(A)
    dA.symmetry = symmetry
    before = (dA.index_stamp(), dA.row_p, dA.col_i, dA.blk_p)
    dbcsr_add_on_diag(dA, alpha, engine=eng)
    torch.cuda.synchronize()
    if diag == "all":   # nothing but the data area is written
        assert dA.index_stamp() == before[0] and dA.row_p is before[1] and dA.col_i is before[2] and dA.blk_p is before[3]
    got = dev_to_bcsr(dA)
    want = dict(blocks)
    for r in range(A.nbr):
        want.setdefault((r, r), np.zeros(int(A.row_sizes[r]) ** 2, dtype))
    same_index(got, from_blocks(A.row_sizes, A.col_sizes, want, dtype))   # the union with the diagonal
    assert dA.packed and dA.symmetry == symmetry
    u4 = 4 * factor(dtype) * unit(dtype)
    for (r, c), v in blocks_of(got).items():
        if r != c:
            assert same_bits(v, blocks[(r, c)])
            continue
        m = int(A.row_sizes[r])
        on = np.arange(m) * (m + 1)
        if (r, r) not in blocks:
            eye = np.zeros(m * m, dtype)
            eye[on] = alpha
            assert same_bits(v, eye), "a new diagonal block is alpha * I"
            continue
        old = blocks[(r, r)]
        off = np.ones(m * m, bool)
        off[on] = False
        assert same_bits(v[off], old[off]), "elements off the diagonal of a diagonal block stay as they are"
        ref = (old[on] + np.asarray(alpha, dtype)).astype(dtype)
        assert np.all(np.abs(v[on] - ref) <= u4 * (np.abs(old[on]) + abs(alpha)))


# ---- 5. plan reuse ----------------------------------------------------------------------------------------------------------------------------
def product_bar(got, alpha, Ad, Bd, bar=1e-10):
    R, scale = alpha * (Ad @ Bd), abs(alpha) * (np.abs(Ad) @ np.abs(Bd))
    G = dense(got)
    mask = dense(O.Bcsr(got.row_sizes, got.col_sizes, got.row_p, got.col_i, got.blk_p, np.ones(got.data.size))) != 0
    assert np.all(np.abs(G - R)[mask] <= bar * scale[mask])
    assert not np.any(R[~mask]), "a block of the product is missing"


def test_operations_between_multiplies_keep_the_plan(monkeypatch):
    monkeypatch.delenv("DBCSR_AMD_MM_PLAN", raising=False)
    eng = MultiplyEngine()
    A, B = square_pair(np.float64)
    dA, dB = to_dev(A), to_dev(B)
    dC = to_dev(subset(A, lambda r, c: False))
    dbcsr_multiply("N", "N", 1.0, dA, dB, 0.0, dC, engine=eng)
    assert eng.plan_stats() == (0, 1)
    torch.cuda.synchronize()
    assert all((r, r) in blocks_of(dev_to_bcsr(dC)) for r in range(dC.nblkrows))   # (add_on_diag below then writes the data area only)
    T = dC.copy()
    for it in range(1, 4):
        stamp = T.index_stamp()
        assert dbcsr_add(T, dC, 1.0, 0.5, engine=eng) is True      # same pattern: in place, no work area of the plan is touched
        assert T.index_stamp() == stamp
        dbcsr_trace(T, engine=eng)
        dbcsr_frobenius_norm(T, engine=eng)
        dbcsr_dot(T, dC, engine=eng)
        dbcsr_scale(T, 0.5, engine=eng)
        dbcsr_add_on_diag(T, 1.0, engine=eng)
        dbcsr_multiply("N", "N", 1.0, dA, dB, 0.0, dC, engine=eng)
        assert eng.plan_stats() == (it, 1), "a multiply after add / trace / norm must reuse its plan"
    torch.cuda.synchronize()
    product_bar(dev_to_bcsr(dC), 1.0, dense(A), dense(B))
    # a union add on an operand: a new index, a new plan, the right product
    extra = to_dev(subset(B, lambda r, c: (r, c) not in blocks_of(A) and (r + c) % 2 == 0))
    assert extra.nblks > 0
    assert dbcsr_add(dA, extra, 1.0, 2.0, engine=eng) is False
    hA = dev_to_bcsr(dA)
    assert hA.nblks == A.nblks + extra.nblks
    dbcsr_multiply("N", "N", 1.0, dA, dB, 0.0, dC, engine=eng)
    assert eng.plan_stats() == (3, 2)
    torch.cuda.synchronize()
    product_bar(dev_to_bcsr(dC), 1.0, dense(hA), dense(B))
    dbcsr_multiply("N", "N", 1.0, dA, dB, 0.0, dC, engine=eng)
    assert eng.plan_stats() == (4, 2)


# ---- 6. one loop that uses everything: three steps of the sign iteration X' = X (3 I - X^2) / 2 ---------------------------------------------------
def test_sign_iteration_step_by_step(eng):
    """every step against the same step done densely in numpy FROM THE DEVICE'S OWN previous iterate (downloaded each step)"""
    sizes = O.make_block_sizes(200, [1, 13, 1, 5, 1, 7])
    X0 = typed(O.make_random_matrix(sizes, sizes, 0.7, O.RANDMAT_SEED_INIT + 41), np.float64)
    X0.data[:] = X0.data / np.linalg.norm(dense(X0), 2)
    dX = to_dev(X0)
    n = int(sizes.sum())
    eye = np.eye(n)
    u = U53

    def check_elements(got, ref, scale, k):
        G = dense(got)
        mask = dense(O.Bcsr(got.row_sizes, got.col_sizes, got.row_p, got.col_i, got.blk_p, np.ones(got.data.size))) != 0
        assert np.all(np.abs(G - ref)[mask] <= k * u * scale[mask])
        assert not np.any(ref[~mask]), "an element of the result is not stored"

    for step in range(3):
        hX = dev_to_bcsr(dX)
        Xd = dense(hX)
        dY = to_dev(subset(hX, lambda r, c: False))
        dbcsr_multiply("N", "N", 1.0, dX, dX, 0.0, dY, engine=eng)                   # Y = X X
        torch.cuda.synchronize()
        hY = dev_to_bcsr(dY)
        product_bar(hY, 1.0, Xd, Xd)
        Yd = dense(hY)
        dR = dY.copy()
        dbcsr_add_on_diag(dR, -1.0, engine=eng)                                       # r = || Y - I ||_F
        torch.cuda.synchronize()
        hR = dev_to_bcsr(dR)
        assert all((r, r) in blocks_of(hR) for r in range(hR.nbr))
        check_elements(hR, Yd - eye, np.abs(Yd) + eye, 4)
        check_norm(eng, dR, real_terms(hR.data))
        dbcsr_scale(dY, -1.0, engine=eng)                                             # Y <- -Y
        torch.cuda.synchronize()
        check_elements(dev_to_bcsr(dY), -Yd, np.abs(Yd), 2)
        dbcsr_add_on_diag(dY, 3.0, engine=eng)                                        # Y <- 3 I - Y
        torch.cuda.synchronize()
        hY2 = dev_to_bcsr(dY)
        check_elements(hY2, 3.0 * eye - Yd, np.abs(Yd) + 3.0 * eye, 4)
        dN = to_dev(subset(hX, lambda r, c: False))
        dbcsr_multiply("N", "N", 0.5, dX, dY, 0.0, dN, engine=eng)                    # X' = X Y / 2
        torch.cuda.synchronize()
        hN = dev_to_bcsr(dN)
        product_bar(hN, 0.5, Xd, dense(hY2))
        check_trace(eng, dN, hN)
        dX = dN
