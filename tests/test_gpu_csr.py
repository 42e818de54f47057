"""Element CSR <-> block-sparse on the device (dbcsr_amd/csr.py: dbcsr_to_csr, dbcsr_from_csr, dbcsr_create_from_csr, dbcsr_csr_to_torch; the "Element CSR"
entries of include/dbcsr_amd_mm.h; kernels of dbcsr_amd/csrc/mm_csr.h) for float64, float32 and complex128.

Everything is a copy or a count, so everything is compared BIT FOR BIT with the numpy restatement of tests/csr_ref.py (checked without a GPU by
tests/test_csr_cpu.py).  No tolerance anywhere.

Matrices: the block-size mix of tests/test_gpu_dense.py -- 10 x 8 blocks of the sizes 1, 5, 13, 23, 32, 33, 40, 64, 96 with block rows 2 and 8 empty: the
smallest shapes that reach one tile, the tile loops in both directions and a block of one element -- at a partial pattern (csr_ref.eps_case: whole blocks
and single elements on either side of EPS, a row that loses everything, +-0.0, NaN, +-Inf) and at the full pattern; the same values in an unpacked data
area (the result of an in-place filter, its holes filled with NaN); a matrix without blocks; a 1 x 1 structure of a 1 x 1 block."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from dbcsr_amd import lib as L
from dbcsr_amd.csr import dbcsr_create_from_csr, dbcsr_csr_to_torch, dbcsr_from_csr, dbcsr_to_csr
from dbcsr_amd.matrix import DbcsrMatrix, StreamHandle
from dbcsr_amd.multiply import MultiplyEngine, dbcsr_multiply
from dbcsr_amd.operations import dbcsr_add, dbcsr_to_dense
from oracle import oracle as O
from tests import csr_ref as R
from tests import far_arena as FA
from tests import test_gpu_dense as GD
from tests.gpu_util import dev_to_bcsr, to_dev
from tests.test_gpu_matrix_norms import blocks_of, from_blocks, hole_positions, is_complex, same_bits, subset, with_holes

pytestmark = pytest.mark.gpu

DTYPES, IDS = R.DTYPES, R.IDS
EPS = R.EPS
EPSES = [None, 0.0, EPS]
EPS_IDS = ["all", "eps0", "eps"]


@pytest.fixture(scope="module")
def eng():
    return MultiplyEngine()


def host(t):
    return t.cpu().numpy()


def host_csr(csr):
    return tuple(host(t) for t in csr)


def dev_csr(csr):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in csr)


@functools.lru_cache(maxsize=None)
def reference(case, dtype_name, eps):
    """the reference CSR of a named packed case, computed once"""
    return R.to_csr(packed_case(case, dtype_name), eps)


def packed_case(case, dtype_name):
    if case == "partial":
        return R.eps_case(dtype_name)
    if case == "full":
        return R.full(dtype_name)
    if case == "empty":
        return subset(R.base(dtype_name), lambda r, c: False)
    one = np.asarray([1], np.int32)
    return from_blocks(one, one, {(0, 0): np.asarray([0.75], np.dtype(dtype_name))}, np.dtype(dtype_name))


def unpacked(eng, dtype):
    """(host, device): the values of csr_ref.eps_case in the data area an in-place filter left -- the blocks where they were, NaN in the holes between them"""
    name = np.dtype(dtype).name
    hB, dB = with_holes(eng, R.base(name), dtype)
    holes = hole_positions(hB)
    assert holes.size > 0 and not dB.packed
    values = blocks_of(R.eps_case(name))
    data = np.full(hB.data.size, np.nan, np.dtype(dtype))
    hU = O.Bcsr(hB.row_sizes, hB.col_sizes, hB.row_p, hB.col_i, hB.blk_p, data)
    for k, view in blocks_of(hU).items():
        view[:] = values[k]
    dB.data.copy_(torch.from_numpy(data).cuda())
    assert np.isnan(host(dB.data)[holes]).all()
    return hU, dB


def check_to_csr(eng, dM, ref, eps):
    stamp, area = dM.index_stamp(), host(dM.data).copy()
    crow, col, values = dbcsr_to_csr(dM, eps=eps, engine=eng)
    assert crow.dtype == torch.int64 and col.dtype == torch.int32 and values.dtype == dM.dtype and crow.is_cuda and col.is_cuda and values.is_cuda
    got = host_csr((crow, col, values))
    assert got[0][0] == 0 and got[0][-1] == got[1].size == got[2].size
    assert same_bits(got[0], ref[0]), "crow"
    assert same_bits(got[1], ref[1]), "col"
    assert same_bits(got[2], ref[2]), "values, by bits"
    assert R.same_csr(host_csr(dbcsr_to_csr(dM, eps=eps, engine=eng)), got), "the same bits on every call"
    assert dM.index_stamp() == stamp and same_bits(host(dM.data), area), "the matrix is only read"
    if eps is None:
        assert got[1].size == dM.nze


# ---- 1. to_csr ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", EPSES, ids=EPS_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_to_csr_of_packed_matrices(eng, dtype, eps):
    name = np.dtype(dtype).name
    for case in ("partial", "full", "empty", "one"):
        check_to_csr(eng, to_dev(packed_case(case, name)), reference(case, name, eps), eps)
    assert reference("empty", name, eps)[0].size == int(GD.ROWS.sum()) + 1 and not reference("empty", name, eps)[0].any()
    if eps == EPS:
        assert reference("partial", name, eps)[1].size < reference("partial", name, None)[1].size


@pytest.mark.parametrize("eps", EPSES, ids=EPS_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_to_csr_of_an_unpacked_matrix_never_reads_the_holes(eng, dtype, eps):
    hU, dU = unpacked(eng, dtype)
    ref = reference("partial", np.dtype(dtype).name, eps)
    assert R.same_csr(R.to_csr(hU, eps), ref), "the CSR does not depend on where the blocks lie"
    check_to_csr(eng, dU, ref, eps)


def test_to_csr_of_a_misaligned_data_area(eng):
    """the data area one element into its allocation: no 16-byte access fits, the walk goes element by element"""
    from tests.test_gpu_matrix_norms import misaligned
    for name in ("float64", "float32"):
        check_to_csr(eng, misaligned(to_dev(packed_case("partial", name))), reference("partial", name, EPS), EPS)


# ---- 2. stored triangles -------------------------------------------------------------------------------------------------------------------------------------
TRIANGLES = [("S", np.float64), ("A", np.float64), ("H", np.complex128), ("K", np.complex128)]


@pytest.mark.parametrize("symmetry,dtype", TRIANGLES, ids=["%s-%s" % (s, np.dtype(d).name) for s, d in TRIANGLES])
def test_to_csr_of_a_stored_triangle(eng, symmetry, dtype):
    M = GD.matrix(np.dtype(dtype).name, "triangle", zeros=True)
    dM = to_dev(M)
    dM.symmetry = symmetry
    expanded = dev_to_bcsr(eng.desymmetrized(dM))
    assert expanded.nblks > M.nblks
    for eps in (None, 0.0):
        got = host_csr(dbcsr_to_csr(dM, eps=eps, engine=eng))
        assert R.same_csr(got, R.to_csr(expanded, eps)), eps
    assert same_bits(host(dM.data), M.data)


# ---- 3. from_csr -------------------------------------------------------------------------------------------------------------------------------------------
def nan_of(dtype):
    return complex(np.nan, np.nan) if is_complex(dtype) else np.nan


def check_from_csr(eng, csr, hT, dT):
    """dT (host mirror hT) after dbcsr_from_csr of the device CSR: the reference's data area, whatever the area held before; no index array is written"""
    before = host(dT.data).copy()
    stamp, tensors = dT.index_stamp(), (dT.row_p, dT.col_i, dT.blk_p, dT.data)
    index = [host(t).copy() for t in tensors[:3]]
    assert dbcsr_from_csr(*csr, dT, engine=eng) is dT
    want = R.from_csr(*host_csr(csr), hT, area=before)
    got = host(dT.data)
    assert same_bits(got, want)
    assert dT.index_stamp() == stamp and all(a is b for a, b in zip(tensors, (dT.row_p, dT.col_i, dT.blk_p, dT.data)))
    assert all(same_bits(host(t), i) for t, i in zip(tensors[:3], index))
    return got


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_from_csr_onto_the_source_pattern(eng, dtype):
    name = np.dtype(dtype).name
    for case in ("partial", "full", "one"):
        M = packed_case(case, name)
        csr = dbcsr_to_csr(to_dev(M), engine=eng)
        dT = to_dev(M)
        dT.data.fill_(nan_of(dtype))
        assert same_bits(check_from_csr(eng, csr, M, dT), M.data), "the round trip gives the source bit for bit"
    hU, dU = unpacked(eng, dtype)
    csr = dbcsr_to_csr(dU, engine=eng)
    holes = hole_positions(hU)
    dU.data.fill_(nan_of(dtype))
    got = check_from_csr(eng, csr, hU, dU)
    assert np.isnan(got[holes]).all() and same_bits(np.delete(got, holes), np.delete(hU.data, holes)), "the holes keep their NaN"


def other_pattern(M):
    """every second block of the structure: about half of M's blocks, and as many that M does not store"""
    keys = [(r, c) for r in range(M.nbr) for c in range(M.nbc)][::2]
    assert 0 < len(set(keys) & set(blocks_of(M))) < min(len(keys), M.nblks)
    return from_blocks(M.row_sizes, M.col_sizes, {(r, c): np.zeros(int(M.row_sizes[r]) * int(M.col_sizes[c])) for r, c in keys}, M.data.dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_from_csr_onto_another_pattern_and_of_a_filtered_csr(eng, dtype):
    M = R.eps_case(np.dtype(dtype).name)
    dM = to_dev(M)
    T = other_pattern(M)
    dT = to_dev(T)
    dT.data.fill_(nan_of(dtype))
    got = check_from_csr(eng, dbcsr_to_csr(dM, engine=eng), T, dT)
    stored = set(blocks_of(M))
    missing = np.concatenate([np.arange(T.blk_p[b], T.blk_p[b] + int(T.row_sizes[r]) * int(T.col_sizes[c]))
                              for b, (r, c) in enumerate(zip(T.rows().tolist(), T.col_i.tolist())) if (r, c) not in stored])
    assert missing.size > 0 and same_bits(got[missing], np.zeros(missing.size, M.data.dtype)), "+0.0 by bits where the CSR has nothing"
    # a CSR that lost elements to eps: +0.0 where they were
    dS = to_dev(M)
    dS.data.fill_(nan_of(dtype))
    got = check_from_csr(eng, dbcsr_to_csr(dM, eps=EPS, engine=eng), M, dS)
    dropped = np.asarray([not R.kept(x, EPS) for x in M.data])
    assert dropped.sum() >= 10 and same_bits(got[dropped], np.zeros(int(dropped.sum()), M.data.dtype)) and same_bits(got[~dropped], M.data[~dropped])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_from_csr_skips_columns_outside_the_matrix(eng, dtype):
    M = R.eps_case(np.dtype(dtype).name)
    crow, col, values = (a.copy() for a in R.to_csr(M, None))
    n_cols = int(M.col_sizes.sum())
    moved = 0
    for i in range(0, len(crow) - 1, 3):   # (the first entry below 0, the last one at or above n_cols: the columns still ascend)
        if crow[i + 1] - crow[i] >= 3:
            col[crow[i]], col[crow[i + 1] - 1] = -1 - i, n_cols + i
            moved += 2
    assert moved >= 20
    dT = to_dev(M)
    dT.data.fill_(nan_of(dtype))
    got = check_from_csr(eng, dev_csr((crow, col, values)), M, dT)
    assert not same_bits(got, M.data) and (got == 0).sum() > (M.data == 0).sum(), "the entries moved outside left +0.0 behind"


def test_from_csr_between_multiplies_keeps_the_plan(monkeypatch):
    monkeypatch.delenv("DBCSR_AMD_MM_PLAN", raising=False)
    eng = MultiplyEngine()
    rng = np.random.default_rng(41)
    A = GD.matrix("float64", "triangle", zeros=False)   # (taken as a matrix without symmetry: an upper block triangle)
    B = from_blocks(GD.SQUARE, GD.SQUARE, {(r, c): GD.random_values(rng, int(GD.SQUARE[r]) * int(GD.SQUARE[c]), np.float64)
                                           for r in range(9) for c in range(9) if (r + 2 * c) % 3}, np.float64)
    dA, dB = to_dev(A), to_dev(B)
    dC = to_dev(subset(A, lambda r, c: False))
    dbcsr_multiply("N", "N", 1.0, dA, dB, 0.0, dC, engine=eng)
    assert eng.plan_stats() == (0, 1)
    torch.cuda.synchronize()
    first = dev_to_bcsr(dC)
    stamps = (dA.index_stamp(), dC.index_stamp())
    csr = dbcsr_to_csr(dA, engine=eng)
    dbcsr_to_csr(dC, eps=EPS, engine=eng)   # (of its result, too)
    dA.data.fill_(np.nan)
    dbcsr_from_csr(*csr, dA, engine=eng)
    assert (dA.index_stamp(), dC.index_stamp()) == stamps
    dbcsr_multiply("N", "N", 1.0, dA, dB, 0.0, dC, engine=eng)
    assert eng.plan_stats() == (1, 1), "a multiply after the CSR conversions must reuse its plan"
    torch.cuda.synchronize()
    assert same_bits(host(dA.data), A.data)
    again = dev_to_bcsr(dC)
    assert same_bits(again.col_i, first.col_i) and same_bits(again.blk_p, first.blk_p) and same_bits(again.data, first.data)


# ---- 4. create_from_csr --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_create_from_csr_reproduces_the_matrix(eng, dtype):
    """from the CSR of every element (explicit zeros count): M's index and its data, bit for bit"""
    M = R.eps_case(np.dtype(dtype).name)
    dM = to_dev(M)
    csr = dbcsr_to_csr(dM, engine=eng)
    rs, cs = dM.row_blk_size, dM.col_blk_size
    dC = dbcsr_create_from_csr(*csr, rs, cs, name="from csr", engine=eng)
    assert dC.row_blk_size is rs and dC.col_blk_size is cs and dC.name == "from csr" and dC.packed and dC.symmetry == "N"
    G = dev_to_bcsr(dC)
    assert same_bits(G.row_p, M.row_p) and same_bits(G.col_i, M.col_i) and same_bits(G.blk_p, M.blk_p) and same_bits(G.data, M.data)
    lists = dbcsr_create_from_csr(*csr, GD.ROWS.tolist(), GD.COLS.tolist(), engine=eng)
    assert same_bits(host(lists.data), M.data)
    none = dbcsr_create_from_csr(csr[0] * 0, csr[1][:0], csr[2][:0], rs, cs, engine=eng)
    assert none.nblks == 0 and none.data.numel() == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_create_from_csr_keeps_the_blocks_that_hold_an_entry(eng, dtype):
    M = R.eps_case(np.dtype(dtype).name)
    ref = R.to_csr(M, EPS)
    blocks = sorted(R.blocks_of_csr(ref[0], ref[1], M.row_sizes, M.col_sizes))
    assert 0 < len(blocks) < M.nblks, "some blocks lost every element"
    dC = dbcsr_create_from_csr(*dev_csr(ref), M.row_sizes, M.col_sizes, engine=eng)
    G = dev_to_bcsr(dC)
    assert dC.packed and sorted(blocks_of(G)) == blocks and np.all(np.diff(G.blk_p) > 0)
    assert same_bits(G.data, R.from_csr(*ref, G, area=np.full(G.data.size, np.nan, G.data.dtype)))
    crow, col, values = host_csr(dbcsr_to_csr(dC, engine=eng))
    at = {(i, int(col[t])): values[t].tobytes() for i in range(len(crow) - 1) for t in range(int(crow[i]), int(crow[i + 1]))}
    assert all(at[(i, int(ref[1][t]))] == ref[2][t].tobytes() for i in range(len(ref[0]) - 1) for t in range(int(ref[0][i]), int(ref[0][i + 1])))
    bad = ref[1].copy()
    bad[5] = int(M.col_sizes.sum())
    with pytest.raises(ValueError):
        dbcsr_create_from_csr(*dev_csr((ref[0], bad, ref[2])), M.row_sizes, M.col_sizes, engine=eng)


# ---- 5. the two-call protocol through the C entries ------------------------------------------------------------------------------------------------------------
def test_the_two_call_protocol(eng):
    M, N = R.eps_case("float64"), R.full("float64")
    dM, dN = to_dev(M), to_dev(N)
    lib, h, st, code = eng.L, eng.h, StreamHandle(), L.dbcsr_type_real_8
    d, other = dM.desc(), dN.desc()
    n_rows = int(M.row_sizes.sum())
    crow = torch.full((n_rows + 1,), -7, dtype=torch.int64, device="cuda")
    col = torch.full((N.data.size,), -7, dtype=torch.int32, device="cuda")
    values = torch.full((N.data.size,), -7.0, dtype=torch.float64, device="cuda")
    nnz = C.c_int64(-1)

    def count(handle=h, datatype=code, m=C.byref(d), use_eps=0, eps=0.0, cr=crow.data_ptr(), n=C.byref(nnz)):
        return lib.dbcsr_amd_bcsr_to_csr_count(handle, datatype, m, use_eps, eps, cr, n, st.ptr)

    def apply(handle=h, datatype=code, m=C.byref(d), c=col.data_ptr(), v=values.data_ptr()):
        return lib.dbcsr_amd_bcsr_to_csr_apply(handle, datatype, m, c, v, st.ptr)

    def untouched():
        torch.cuda.synchronize()
        return bool((col == -7).all()) and bool((values == -7.0).all())

    assert count(handle=None) == -1 and count(m=None) == -1 and count(cr=None) == -1 and count(n=None) == -1
    assert count(use_eps=1, eps=-1.0) == -1 and count(use_eps=1, eps=float("nan")) == -1 and count(datatype=99) == -10
    assert apply(handle=None) == -1 and apply(m=None) == -1 and apply(datatype=99) == -10
    assert apply() == -1 and untouched(), "an apply without a count is refused and writes nothing"
    assert count() == 0 and nnz.value == M.data.size
    assert apply(m=C.byref(other)) == -1 and untouched(), "an apply for another matrix is refused"
    assert apply() == -1 and untouched(), "... and the count it was given is over"
    assert count() == 0 and apply(datatype=L.dbcsr_type_real_4) == -1 and untouched(), "another type than the counted one"
    assert count() == 0 and apply(c=None) == -1 and untouched()

    # an add that builds a union pattern and a multiply between the two halves
    A = GD.matrix("float64", "triangle", zeros=False)
    rng = np.random.default_rng(43)
    B = from_blocks(GD.SQUARE, GD.SQUARE, {(r, c): GD.random_values(rng, int(GD.SQUARE[r]) * int(GD.SQUARE[c]), np.float64)
                                           for r in range(9) for c in range(9) if (r + 2 * c) % 3}, np.float64)
    for use_eps, eps in ((0, None), (1, EPS)):
        ref = R.to_csr(M, eps)
        assert count(use_eps=use_eps, eps=eps or 0.0) == 0 and nnz.value == ref[1].size
        dA, dB = to_dev(A), to_dev(B)
        dbcsr_add(dA, dB, 1.0, 2.0, engine=eng)
        dC = to_dev(subset(A, lambda r, c: False))
        dbcsr_multiply("N", "N", 1.0, dA, dB, 0.0, dC, engine=eng)
        assert dA.nblks > A.nblks and dC.nblks > 0
        col.fill_(-7)
        values.fill_(-7.0)
        assert apply() == 0
        torch.cuda.synchronize()
        k = nnz.value
        assert same_bits(host(crow), ref[0]) and same_bits(host(col[:k]), ref[1]) and same_bits(host(values[:k]), ref[2])
        assert bool((col[k:] == -7).all()) and bool((values[k:] == -7.0).all()), "nothing behind nnz is written"
        col.fill_(-7)
        values.fill_(-7.0)
        assert apply() == -1 and untouched(), "a second apply after one served is refused"


def test_c_abi_answers_of_from_csr_and_name_blocks(eng):
    M = R.eps_case("float64")
    dM = to_dev(M)
    lib, h, st, code = eng.L, eng.h, StreamHandle(), L.dbcsr_type_real_8
    d = dM.desc()
    n_rows, n_cols = int(M.row_sizes.sum()), int(M.col_sizes.sum())
    ref = R.to_csr(M, None)
    crow, col, values = dev_csr(ref)
    area = host(dM.data).copy()

    def from_csr(handle=h, datatype=code, rows=n_rows, cols=n_cols, n=col.numel(), cr=crow.data_ptr(), c=col.data_ptr(), v=values.data_ptr(), m=C.byref(d)):
        return lib.dbcsr_amd_bcsr_from_csr(handle, datatype, rows, cols, n, cr, c, v, m, st.ptr)

    assert from_csr(handle=None) == -1 and from_csr(m=None) == -1 and from_csr(cr=None) == -1 and from_csr(c=None) == -1 and from_csr(v=None) == -1
    assert from_csr(rows=n_rows - 1) == -1 and from_csr(cols=n_cols + 1) == -1 and from_csr(rows=-1) == -1 and from_csr(n=-1) == -1
    assert from_csr(cols=2 ** 31) == -1 and from_csr(datatype=99) == -10
    torch.cuda.synchronize()
    assert same_bits(host(dM.data), area), "a refused call writes nothing"
    # nnz below the true count: every position formed from crow is clamped -- the entries behind it are not read
    short = ref[1].size // 2
    dM.data.fill_(np.nan)
    assert from_csr(n=short) == 0
    clamped = np.minimum(ref[0], short)
    assert same_bits(host(dM.data), R.from_csr(clamped, ref[1], ref[2], M))
    none = np.zeros(0, np.int32)
    z = to_dev(from_blocks(none, none, {}, np.float64)).desc()
    assert from_csr(rows=0, cols=0, n=0, c=None, v=None, m=C.byref(z)) == 0

    rows = torch.full((col.numel(),), 7, dtype=torch.int32, device="cuda")
    cols = torch.full((col.numel(),), 7, dtype=torch.int32, device="cuda")

    def name(handle=h, n_r=n_rows, n=col.numel(), cr=crow.data_ptr(), c=col.data_ptr(), rs=dM.row_blk_size.data_ptr(), cs=dM.col_blk_size.data_ptr(),
             nbr=M.nbr, nbc=M.nbc, r=rows.data_ptr(), cc=cols.data_ptr()):
        return lib.dbcsr_amd_bcsr_csr_name_blocks(handle, n_r, n, cr, c, rs, cs, nbr, nbc, r, cc, st.ptr)

    assert name(handle=None) == -1 and name(cr=None) == -1 and name(c=None) == -1 and name(r=None) == -1 and name(rs=None) == -1
    assert name(n_r=-1) == -1 and name(n=-1) == -1 and name(nbr=-1) == -1
    torch.cuda.synchronize()
    assert bool((rows == 7).all()) and bool((cols == 7).all())
    bad = ref[1].copy()
    bad[3], bad[4] = -1, n_cols
    col.copy_(torch.from_numpy(bad).cuda())
    assert name() == 0
    got_r, got_c = host(rows), host(cols)
    ro, co = R.offsets(M.row_sizes), R.offsets(M.col_sizes)
    row_of = np.repeat(np.arange(n_rows), np.diff(ref[0]))
    want_r = (np.searchsorted(ro, row_of, side="right") - 1).astype(np.int32)
    want_c = (np.searchsorted(co, bad, side="right") - 1).astype(np.int32)
    want_r[3:5] = want_c[3:5] = -1
    assert same_bits(got_r, want_r) and same_bits(got_c, want_c), "an entry outside the structure is named (-1, -1)"


# ---- 6. positions above 2^31 ---------------------------------------------------------------------------------------------------------------------------------
def test_positions_above_2_to_the_31(eng):
    """the count half alone, without eps: the full pattern of 500 x 500 blocks of 96 x 96 names 2 304 000 000 elements.  The data pointer is a tensor of
    one element -- the entry reads no element; beyond the index only the slots (48 000 rows x 500 blocks) and crow are allocated."""
    nb, size = 500, 96
    sizes = torch.full((nb,), size, dtype=torch.int32, device="cuda")
    row_p = (torch.arange(nb + 1, dtype=torch.int64, device="cuda") * nb).to(torch.int32)
    col_i = torch.arange(nb, dtype=torch.int32, device="cuda").repeat(nb)
    blk_p = torch.arange(nb * nb, dtype=torch.int64, device="cuda") * (size * size)
    dM = DbcsrMatrix(sizes, sizes, row_p, col_i, blk_p, torch.zeros(1, dtype=torch.float64, device="cuda"), nze=nb * nb * size * size)
    d = dM.desc()
    crow = torch.full((nb * size + 1,), -7, dtype=torch.int64, device="cuda")
    nnz = C.c_int64(-1)
    for _ in range(2):   # (the second time the index is a known one)
        assert eng.L.dbcsr_amd_bcsr_to_csr_count(eng.h, L.dbcsr_type_real_8, C.byref(d), 0, 0.0, crow.data_ptr(), C.byref(nnz), StreamHandle().ptr) == 0
        torch.cuda.synchronize()
        assert nnz.value == 2304000000 > 2 ** 31
        assert same_bits(host(crow), np.cumsum(np.concatenate([[0], np.full(nb * size, nb * size, np.int64)])).astype(np.int64))
        crow.fill_(-7)


# ---- 7. far block offsets ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def arena():
    a = FA.arena()
    yield a
    if a is not None:
        a.release()
        del a
    torch.cuda.empty_cache()


def test_a_far_matrix(eng, arena):
    """float64: the blocks placed around 2^29, 2^31, 2^32, ... elements of one large allocation, one block straddling 2^32 (tests/far_arena.py)"""
    if arena is None:
        pytest.skip("the device has less than %d bytes free: no far arena" % (FA.ARENA_SMALL + FA.MARGIN))
    M = R.eps_case("float64")
    far = FA.Far(arena.view(np.float64))
    blk_p = FA.place(M, np.float64, "blocks", 0, arena.nbytes)
    dM = far.on_device(M, blk_p)
    far.seal()
    assert FA.straddlers(M, blk_p, 2 ** 32).size > 0 and far.max_high_byte() >= 1, "a block straddles 2^32 elements"
    for eps in (None, EPS):
        assert R.same_csr(host_csr(dbcsr_to_csr(dM, eps=eps, engine=eng)), reference("partial", "float64", eps)), eps
    ref = reference("partial", "float64", None)
    doubled = (ref[0], ref[1], np.where(np.isnan(ref[2]), 3.0, ref[2] * 2))
    dbcsr_from_csr(*dev_csr(doubled), dM, engine=eng)
    torch.cuda.synchronize()
    assert same_bits(FA.blocks_to_host(dM).data, R.from_csr(*doubled, M)) and far.guards_kept()


# ---- 8. interop ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_torch_tensor_of_the_csr(eng, dtype):
    M = R.nonzero(np.dtype(dtype).name)
    assert not np.any(M.data == 0) and not np.isnan(M.data).any()
    dM = to_dev(M)
    shape = GD.full_shape(M)
    T = dbcsr_csr_to_torch(*dbcsr_to_csr(dM, engine=eng), shape)
    assert T.layout == torch.sparse_csr and T.col_indices().dtype == torch.int64 and tuple(T.shape) == shape
    assert same_bits(T.cpu().to_dense().numpy(), host(dbcsr_to_dense(dM, engine=eng)))
