"""A matrix under another block structure on the device (dbcsr_amd/reblock.py: dbcsr_reblock, dbcsr_reblock_into; the "Re-blocking" entries of
include/dbcsr_amd_mm.h; kernels of dbcsr_amd/csrc/mm_reblock.h) for float64, float32 and complex128.

Everything is a copy, so everything is compared BIT FOR BIT with the numpy restatement tests/reblock_ref.py (checked without a GPU by
tests/test_reblock_cpu.py).  No tolerance anywhere but in the multiply in another blocking, whose bar is stated there.

The source is the block-size mix of tests/test_gpu_dense.py -- 10 x 8 blocks of 1, 5, 13, 23, 32, 33, 40, 64, 96, block rows 2 and 8 empty -- at the
partial pattern with -0.0, NaN and +-Inf and at the full pattern; the new structures (reblock_ref.STRUCTURES): the same sizes, all ones, one block for
everything, uniform 32 with a tail, boundaries shifted against the source (7, then 16s), consecutive pairs merged, every block halved, blocks of 96 and
100 for the tile loops."""
import ctypes as C

import numpy as np
import pytest
import torch

from dbcsr_amd import lib as L
from dbcsr_amd.matrix import DbcsrMatrix, StreamHandle
from dbcsr_amd.multiply import MultiplyEngine, dbcsr_multiply
from dbcsr_amd.operations import dbcsr_copy
from dbcsr_amd.reblock import dbcsr_merged_block_sizes, dbcsr_reblock, dbcsr_reblock_into
from oracle import oracle as O
from tests import csr_ref as CR
from tests import far_arena as FA
from tests import reblock_ref as R
from tests import test_gpu_dense as GD
from tests.gpu_util import dev_to_bcsr, to_dev
from tests.test_gpu_csr import unpacked
from tests.test_gpu_matrix_norms import blocks_of, dense, from_blocks, hole_positions, is_complex, pattern_mask, same_bits, subset

pytestmark = pytest.mark.gpu

DTYPES, IDS = R.DTYPES, R.IDS


@pytest.fixture(scope="module")
def eng():
    return MultiplyEngine()


def host(t):
    return t.cpu().numpy()


def nan_of(dtype):
    return complex(np.nan, np.nan) if is_complex(dtype) else np.nan


def check_reblock(eng, dM, ref, rs, cs):
    """dbcsr_reblock of the device matrix: the reference by bits, packed, the same on a second call, the source only read"""
    stamp, area = dM.index_stamp(), host(dM.data).copy()
    out = dbcsr_reblock(dM, rs, cs, engine=eng)
    got = dev_to_bcsr(out)
    assert R.same_matrix(got, ref), "index and data, by bits"
    assert out.packed and out.symmetry == "N" and out.dtype == dM.dtype and out.nze == ref.data.size
    assert out.row_p.dtype == torch.int32 and out.col_i.dtype == torch.int32 and out.blk_p.dtype == torch.int64
    assert R.same_matrix(dev_to_bcsr(dbcsr_reblock(dM, rs, cs, engine=eng)), got), "the same bits on every call"
    assert dM.index_stamp() == stamp and same_bits(host(dM.data), area), "the source is only read"
    return out


# ---- 1. dbcsr_reblock --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.NAMES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_reblock_of_packed_matrices(eng, dtype, name):
    dn = np.dtype(dtype).name
    rs, cs = R.STRUCTURES[name]
    for case in R.CASES:
        check_reblock(eng, to_dev(R.source(case, dn)), R.reference(case, dn, name), rs, cs)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_same_sizes_give_the_source_in_new_tensors(eng, dtype):
    M = R.source("partial", np.dtype(dtype).name)
    dM = to_dev(M)
    out = dbcsr_reblock(dM, dM.row_blk_size, dM.col_blk_size, engine=eng)   # (device tensors are taken as they are)
    assert out.row_blk_size is dM.row_blk_size and out.col_blk_size is dM.col_blk_size
    assert R.same_matrix(dev_to_bcsr(out), M)
    for a, b in zip((out.row_p, out.col_i, out.blk_p, out.data), (dM.row_p, dM.col_i, dM.blk_p, dM.data)):
        assert a is not b and a.data_ptr() != b.data_ptr()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_reblock_of_an_empty_matrix_and_of_one_element(eng, dtype):
    dn = np.dtype(dtype).name
    empty = subset(R.source("partial", dn), lambda r, c: False)
    for name in ("same", "u32", "one"):
        out = dbcsr_reblock(to_dev(empty), *R.STRUCTURES[name], engine=eng)
        assert out.nblks == 0 and out.data.numel() == 0 and out.nblkrows == len(R.STRUCTURES[name][0]) and not host(out.row_p).any()
    one = np.asarray([1], np.int32)
    M = from_blocks(one, one, {(0, 0): np.asarray([-0.0 if not is_complex(dtype) else 0.75], np.dtype(dtype))}, np.dtype(dtype))
    check_reblock(eng, to_dev(M), M, [1], [1])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_reblock_of_an_unpacked_matrix_never_reads_the_holes(eng, dtype):
    """the source is the result of an in-place filter, its holes full of NaN: no NaN of a hole arrives, the result is that of the packed twin"""
    dn = np.dtype(dtype).name
    hU, dU = unpacked(eng, dtype)
    assert not dU.packed and np.isnan(host(dU.data)[hole_positions(hU)]).all()
    for name in ("u32", "shifted", "one", "halves"):
        ref = R.reference("partial", dn, name)
        assert R.same_matrix(R.reblock(hU, *R.STRUCTURES[name]), ref), "the result does not depend on where the blocks lie"
        check_reblock(eng, dU, ref, *R.STRUCTURES[name])


def test_reblock_of_a_misaligned_data_area(eng):
    """the source's data area one element into its allocation; the new one is aligned: loads wherever they fall, 16-byte stores on the written side"""
    from tests.test_gpu_matrix_norms import misaligned
    for dn in ("float64", "float32"):
        for name in ("u32", "halves"):
            check_reblock(eng, misaligned(to_dev(R.source("partial", dn))), R.reference("partial", dn, name), *R.STRUCTURES[name])


# ---- 2. stored triangles -----------------------------------------------------------------------------------------------------------------------------------
TRIANGLES = [("S", np.float64), ("A", np.float64), ("S", np.float32), ("A", np.float32), ("H", np.complex128), ("K", np.complex128)]


@pytest.mark.parametrize("symmetry,dtype", TRIANGLES, ids=["%s-%s" % (s, np.dtype(d).name) for s, d in TRIANGLES])
def test_reblock_of_a_stored_triangle(eng, symmetry, dtype):
    M = GD.matrix(np.dtype(dtype).name, "triangle", zeros=True)
    dM = to_dev(M)
    dM.symmetry = symmetry
    expanded = dev_to_bcsr(eng.desymmetrized(dM))
    assert expanded.nblks > M.nblks
    n = int(GD.SQUARE.sum())
    for sizes in (R.uniform(n, 32), R.shifted(n)):
        out = dbcsr_reblock(dM, sizes, sizes, engine=eng)
        assert out.symmetry == "N" and R.same_matrix(dev_to_bcsr(out), R.reblock(expanded, sizes, sizes))
        T = R.half_pattern(M, sizes, sizes)
        dT = to_dev(T)
        dT.data.fill_(nan_of(dtype))
        dbcsr_reblock_into(dM, dT, engine=eng)
        assert same_bits(host(dT.data), R.reblock_into(expanded, T))
    assert same_bits(host(dM.data), M.data) and dM.symmetry == symmetry


# ---- 3. dbcsr_reblock_into -----------------------------------------------------------------------------------------------------------------------------------
UNMET = ("same", "ones", "shifted", "halves")   # the structures under which every second block holds one that the partial source does not meet


def check_into(eng, dA, hA, hT, dT):
    """dT (host mirror hT) after dbcsr_reblock_into(dA, dT): the reference's data area, whatever the area held before; no index array is written"""
    before = host(dT.data).copy()
    stamp, tensors = dT.index_stamp(), (dT.row_p, dT.col_i, dT.blk_p, dT.data)
    index = [host(t).copy() for t in tensors[:3]]
    a_stamp, a_area = dA.index_stamp(), host(dA.data).copy()
    assert dbcsr_reblock_into(dA, dT, engine=eng) is dT
    got = host(dT.data)
    assert same_bits(got, R.reblock_into(hA, hT, area=before))
    assert dT.index_stamp() == stamp and all(a is b for a, b in zip(tensors, (dT.row_p, dT.col_i, dT.blk_p, dT.data)))
    assert all(same_bits(host(t), i) for t, i in zip(tensors[:3], index))
    assert dA.index_stamp() == a_stamp and same_bits(host(dA.data), a_area)
    return got


@pytest.mark.parametrize("name", R.NAMES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_reblock_into_a_partial_pattern(eng, dtype, name):
    """the destination stores every second block of the new structure: blocks the source does not meet become +0.0, blocks it lacks are not made"""
    dn = np.dtype(dtype).name
    A = R.source("partial", dn)
    T = R.half_pattern(A, *R.STRUCTURES[name])
    met = R.pattern(A, *R.STRUCTURES[name])
    rs, cs = R.STRUCTURES[name]
    assert met - set(blocks_of(T)) or name == "one", "blocks the source meets and the destination lacks"
    assert set(blocks_of(T)) - met or name not in UNMET, "blocks the destination stores and the source does not meet"
    dT = to_dev(T)
    dT.data.fill_(nan_of(dtype))
    got = check_into(eng, to_dev(A), A, T, dT)
    assert not same_bits(got, T.data)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_reblock_into_an_unpacked_destination_keeps_the_holes(eng, dtype):
    """the destination is the result of an in-place filter with canaries in its holes; the source is the full pattern under other sizes"""
    dn = np.dtype(dtype).name
    hU, dU = unpacked(eng, dtype)
    holes = hole_positions(hU)
    canary = np.dtype(dtype).type(FA.CANARY)
    for name in ("u32", "shifted", "ones", "big"):
        A = R.reference("full", dn, name)
        area = host(dU.data).copy()
        area[:] = nan_of(dtype)
        area[holes] = canary
        dU.data.copy_(torch.from_numpy(area).cuda())
        got = check_into(eng, to_dev(A), A, hU, dU)
        assert same_bits(got[holes], np.full(holes.size, canary)), "the holes keep their bits"
        want = blocks_of(R.source("full", dn))
        mine = blocks_of(O.Bcsr(hU.row_sizes, hU.col_sizes, hU.row_p, hU.col_i, hU.blk_p, got))
        assert all(same_bits(v, want[k]) for k, v in mine.items()), "every stored block is the full matrix' block"


def test_reblock_into_between_multiplies_keeps_the_plan(monkeypatch):
    """as tests/test_gpu_csr.py checks it for dbcsr_from_csr: an operand rewritten by dbcsr_reblock_into, then the same multiply again"""
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
    n = int(GD.SQUARE.sum())
    merged = dbcsr_merged_block_sizes(GD.SQUARE, 32)
    dM = dbcsr_reblock(dA, merged, merged, engine=eng)   # (a reserve that creates blocks takes the work areas: the plan goes, as with the union add)
    dbcsr_multiply("N", "N", 1.0, dA, dB, 0.0, dC, engine=eng)
    hits, misses = eng.plan_stats()
    stamps = (dA.index_stamp(), dC.index_stamp())
    dA.data.fill_(np.nan)
    dbcsr_reblock_into(dM, dA, engine=eng)
    dbcsr_reblock_into(dC, to_dev(R.half_pattern(A, R.uniform(n, 32), R.uniform(n, 32))), engine=eng)   # (of its result, too)
    assert (dA.index_stamp(), dC.index_stamp()) == stamps
    dbcsr_multiply("N", "N", 1.0, dA, dB, 0.0, dC, engine=eng)
    assert eng.plan_stats() == (hits + 1, misses), "a multiply after dbcsr_reblock_into must reuse its plan"
    torch.cuda.synchronize()
    assert same_bits(host(dA.data), A.data)
    again = dev_to_bcsr(dC)
    assert same_bits(again.col_i, first.col_i) and same_bits(again.blk_p, first.blk_p) and same_bits(again.data, first.data)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_same_structure_gives_the_bits_of_copy_with_keep_sparsity(eng, dtype):
    dn = np.dtype(dtype).name
    A = R.source("partial", dn)
    T = CR.full(dn)
    T2 = R.half_pattern(A, R.ROWS.tolist(), R.COLS.tolist())
    for hT in (T, T2):
        dA, d1, d2 = to_dev(A), to_dev(hT), to_dev(hT)
        d1.data.fill_(nan_of(dtype)), d2.data.fill_(nan_of(dtype))
        dbcsr_copy(d1, dA, keep_sparsity=True, engine=eng)
        dbcsr_reblock_into(dA, d2, engine=eng)
        assert same_bits(host(d2.data), host(d1.data)) and same_bits(host(d2.data), R.reblock_into(A, hT))


# ---- 4. there and back -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.NAMES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_round_trip(eng, dtype, name):
    dn = np.dtype(dtype).name
    for case in R.CASES:
        A = R.source(case, dn)
        dA = to_dev(A)
        back = to_dev(A)   # (a copy of A's pattern)
        back.data.fill_(nan_of(dtype))
        dbcsr_reblock_into(dbcsr_reblock(dA, *R.STRUCTURES[name], engine=eng), back, engine=eng)
        assert R.same_matrix(dev_to_bcsr(back), A)


# ---- 5. a multiply in another blocking -----------------------------------------------------------------------------------------------------------------------
def test_multiply_in_merged_blocks(eng):
    """A (ROWS x COLS) and B (COLS x ROWS) of the mix, re-blocked to merged blocks of about 32, multiplied there, the product brought back.  The sums of a
    product element run over the same terms in another order (a merged block joins inner blocks), so bits may differ: the bar is the derived one of
    DESIGN 4c, |got - ref| <= gamma |alpha| (|A| |B|) with gamma = (n + 8) u / (1 - (n + 8) u), n = 243 inner elements, u = 2^-53."""
    rng = np.random.default_rng(77)
    A = CR.nonzero("float64")
    B = from_blocks(GD.COLS, GD.ROWS, {(r, c): GD.random_values(rng, int(GD.COLS[r]) * int(GD.ROWS[c]), np.float64)
                                       for r in range(len(GD.COLS)) for c in range(len(GD.ROWS)) if (r + 2 * c) % 3}, np.float64)
    alpha = -1.75
    dA, dB = to_dev(A), to_dev(B)
    dC = to_dev(from_blocks(GD.ROWS, GD.ROWS, {}, np.float64))
    dbcsr_multiply("N", "N", alpha, dA, dB, 0.0, dC, engine=eng)
    mr, mk = dbcsr_merged_block_sizes(GD.ROWS, 32), dbcsr_merged_block_sizes(GD.COLS, 32)
    assert len(mr) < len(GD.ROWS) and len(mk) < len(GD.COLS)
    mA, mB = dbcsr_reblock(dA, mr, mk, engine=eng), dbcsr_reblock(dB, mk, mr, engine=eng)
    mC = to_dev(from_blocks(np.asarray(mr, np.int32), np.asarray(mr, np.int32), {}, np.float64))
    dbcsr_multiply("N", "N", alpha, mA, mB, 0.0, mC, engine=eng)
    back = dev_to_bcsr(dbcsr_reblock(mC, GD.ROWS.tolist(), GD.ROWS.tolist(), engine=eng))
    ref = dev_to_bcsr(dC)
    n, u = int(GD.COLS.sum()), 2.0 ** -53
    gamma = (n + 8) * u / (1.0 - (n + 8) * u)
    bar = gamma * abs(alpha) * (np.abs(dense(A)) @ np.abs(dense(B)))
    err = np.abs(dense(back) - dense(ref))
    print("multiply in merged blocks: worst error / bar = %.3g" % float(np.max(err / np.maximum(bar, 1e-300))))
    assert ref.nblks > 0 and np.all(err <= bar)
    assert np.all(pattern_mask(back)[pattern_mask(ref)]), "the pattern contains the original product's pattern"


# ---- 6. far offsets ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def arena():
    a = FA.arena()
    yield a
    if a is not None:
        a.release()


def test_blocks_above_2_to_the_32_elements(eng, arena):
    """float32: the source's blocks and the destination's blocks above 2^32 elements of their data areas, the two halves of one large allocation that is
    never filled; canaries around the written window and where a lost high word would write instead (2^32 elements lower)"""
    if arena is None or arena.nbytes < FA.ARENA_LARGE:
        pytest.skip("the device has no room for the large arena")
    view = arena.view(np.float32)
    half = 2 ** 33
    assert view.numel() >= 2 * half
    src, dst = view[:half], view[half:2 * half]
    A = R.source("partial", "float32")
    T = R.half_pattern(A, *R.STRUCTURES["shifted"])
    base_s, base_d, guard = FA.TWO32 + 12345, FA.TWO32 + 2 ** 31 + 777, FA.GUARD
    src[base_s:base_s + A.data.size].copy_(torch.from_numpy(A.data))
    dst[base_d - guard:base_d + T.data.size + guard].fill_(FA.CANARY)
    low = dst[base_d - FA.TWO32 - guard:base_d - FA.TWO32 + T.data.size + guard]
    low.fill_(FA.CANARY)
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda()
    far = lambda M, area, base: DbcsrMatrix(t(M.row_sizes, torch.int32), t(M.col_sizes, torch.int32), t(M.row_p, torch.int32), t(M.col_i, torch.int32),
                                            t(M.blk_p.astype(np.int64) + base, torch.int64), area, nze=int(M.data.size))
    dbcsr_reblock_into(far(A, src, base_s), far(T, dst, base_d), engine=eng)
    torch.cuda.synchronize()
    got = host(dst[base_d - guard:base_d + T.data.size + guard])
    canary = np.full(guard, FA.CANARY, np.float32)
    assert same_bits(got[guard:-guard], R.reblock_into(A, T))
    assert same_bits(got[:guard], canary) and same_bits(got[-guard:], canary)
    assert same_bits(host(low), np.full(low.numel(), FA.CANARY, np.float32)), "nothing is written 2^32 elements lower"
    assert same_bits(host(src[base_s:base_s + A.data.size]), A.data)


# ---- 7. the C entries directly -------------------------------------------------------------------------------------------------------------------------------
def test_c_abi_answers(eng):
    st = StreamHandle()
    A = R.source("partial", "float64")
    dA = to_dev(A)
    rs, cs = R.STRUCTURES["u32"]
    t = lambda a: torch.as_tensor(np.asarray(a, np.int32)).cuda()
    drs, dcs = t(rs), t(cs)
    a = dA.desc()
    # the pieces: the total, then the list; every new block of the reference is named, nothing else
    total = C.c_int64(-5)
    assert eng.L.dbcsr_amd_bcsr_reblock_name_blocks(eng.h, C.byref(a), drs.data_ptr(), dcs.data_ptr(), len(rs), len(cs), C.byref(total), None, None, st.ptr) == 0
    n = total.value
    ref = R.reference("partial", "float64", "u32")
    assert ref.nblks <= n < 2 ** 31
    rows, cols = torch.full((n + 8,), -7, dtype=torch.int32, device="cuda"), torch.full((n + 8,), -7, dtype=torch.int32, device="cuda")
    assert eng.L.dbcsr_amd_bcsr_reblock_name_blocks(eng.h, C.byref(a), drs.data_ptr(), dcs.data_ptr(), len(rs), len(cs), C.byref(total), rows.data_ptr(),
                                                    cols.data_ptr(), st.ptr) == 0
    torch.cuda.synchronize()
    hr, hc = host(rows), host(cols)
    assert set(zip(hr[:n].tolist(), hc[:n].tolist())) == set(blocks_of(ref)) and (hr[n:] == -7).all() and (hc[n:] == -7).all()
    short = C.c_int64(n - 3)   # (a list shorter than the pieces: nothing is stored at or behind its length)
    rows.fill_(-7), cols.fill_(-7)
    assert eng.L.dbcsr_amd_bcsr_reblock_name_blocks(eng.h, C.byref(a), drs.data_ptr(), dcs.data_ptr(), len(rs), len(cs), C.byref(short), rows.data_ptr(),
                                                    cols.data_ptr(), st.ptr) == 0
    torch.cuda.synchronize()
    assert same_bits(host(rows)[:n - 3], hr[:n - 3]) and (host(rows)[n - 3:] == -7).all() and (host(cols)[n - 3:] == -7).all()
    assert eng.L.dbcsr_amd_bcsr_reblock_name_blocks(eng.h, C.byref(a), drs.data_ptr(), dcs.data_ptr(), len(rs), len(cs), C.byref(total), rows.data_ptr(), None,
                                                    st.ptr) == -1
    assert eng.L.dbcsr_amd_bcsr_reblock_name_blocks(eng.h, C.byref(a), drs.data_ptr(), dcs.data_ptr(), len(rs), len(cs), None, None, None, st.ptr) == -1
    assert eng.L.dbcsr_amd_bcsr_reblock_name_blocks(None, C.byref(a), drs.data_ptr(), dcs.data_ptr(), len(rs), len(cs), C.byref(total), None, None, st.ptr) == -1

    # _reserve_apply_index: without a pending count, twice, and for another matrix: -1 and nothing written
    empty = DbcsrMatrix.empty_like_pattern(drs, dcs, torch.float64)
    other = DbcsrMatrix.empty_like_pattern(drs, dcs, torch.float64)
    row_p = torch.empty(len(rs) + 1, dtype=torch.int32, device="cuda")
    col_i = torch.full((ref.nblks,), -7, dtype=torch.int32, device="cuda")
    blk_p = torch.full((ref.nblks,), -7, dtype=torch.int64, device="cuda")
    out = DbcsrMatrix(drs, dcs, row_p, col_i, blk_p, torch.full((ref.data.size,), np.nan, dtype=torch.float64, device="cuda"))
    untouched = lambda: (host(col_i) == -7).all() and (host(blk_p) == -7).all() and np.isnan(host(out.data)).all()
    m, o, d = empty.desc(), other.desc(), out.desc()
    assert eng.L.dbcsr_amd_bcsr_reserve_apply_index(eng.h, C.byref(m), C.byref(d), st.ptr) == -1 and untouched(), "no count is pending"

    def count(desc):
        nb, nz, new, bad = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        assert eng.L.dbcsr_amd_bcsr_reserve_count(eng.h, C.byref(desc), n + 8, rows.data_ptr(), cols.data_ptr(), 0, row_p.data_ptr(), C.byref(nb), C.byref(nz),
                                                  C.byref(new), C.byref(bad), st.ptr) == 0
        assert (nb.value, nz.value, new.value, bad.value) == (ref.nblks, ref.data.size, ref.nblks, 0)
    rows.copy_(torch.from_numpy(np.concatenate([hr[:n], hr[:8]])).cuda()), cols.copy_(torch.from_numpy(np.concatenate([hc[:n], hc[:8]])).cuda())
    count(m)
    assert eng.L.dbcsr_amd_bcsr_reserve_apply_index(eng.h, C.byref(o), C.byref(d), st.ptr) == -1 and untouched(), "another matrix than the counted one"
    assert eng.L.dbcsr_amd_bcsr_reserve_apply_index(eng.h, C.byref(m), C.byref(d), st.ptr) == -1 and untouched(), "the refusal ended the count"
    count(m)
    assert eng.L.dbcsr_amd_bcsr_reserve_apply_index(eng.h, C.byref(m), C.byref(d), st.ptr) == 0
    torch.cuda.synchronize()
    assert same_bits(host(col_i), ref.col_i.astype(np.int32)) and same_bits(host(blk_p), ref.blk_p.astype(np.int64)) and same_bits(host(row_p), ref.row_p.astype(np.int32))
    assert np.isnan(host(out.data)).all(), "the index alone: no element of the data area is written"
    kept = (host(col_i).copy(), host(blk_p).copy())
    col_i.fill_(-7), blk_p.fill_(-7)
    assert eng.L.dbcsr_amd_bcsr_reserve_apply_index(eng.h, C.byref(m), C.byref(d), st.ptr) == -1 and untouched(), "a second apply"
    col_i.copy_(torch.from_numpy(kept[0]).cuda()), blk_p.copy_(torch.from_numpy(kept[1]).cuda())

    # _reblock_gather: the move onto that index; its refusals
    d = out.desc()
    assert eng.L.dbcsr_amd_bcsr_reblock_gather(eng.h, L.dbcsr_type_real_8, C.byref(a), C.byref(d), st.ptr) == 0
    torch.cuda.synchronize()
    assert same_bits(host(out.data), ref.data)
    wrong = to_dev(subset(CR.full("float64"), lambda r, c: r < 9))
    wrong.row_blk_size = wrong.row_blk_size[:9].clone()   # (one block row less: the sums differ)
    wrong.row_p = wrong.row_p[:10].clone()
    before = host(out.data).copy()
    w = wrong.desc()
    assert eng.L.dbcsr_amd_bcsr_reblock_gather(eng.h, L.dbcsr_type_real_8, C.byref(w), C.byref(d), st.ptr) == -1
    assert eng.L.dbcsr_amd_bcsr_reblock_gather(eng.h, L.dbcsr_type_real_8, C.byref(a), C.byref(w), st.ptr) == -1
    assert eng.L.dbcsr_amd_bcsr_reblock_gather(eng.h, L.dbcsr_type_complex_4, C.byref(a), C.byref(d), st.ptr) == -10
    assert eng.L.dbcsr_amd_bcsr_reblock_gather(eng.h, L.dbcsr_type_real_8, C.byref(a), C.byref(a), st.ptr) == -1, "src->data == dst->data"
    assert eng.L.dbcsr_amd_bcsr_reblock_gather(eng.h, L.dbcsr_type_real_8, None, C.byref(d), st.ptr) == -1
    assert eng.L.dbcsr_amd_bcsr_reblock_gather(None, L.dbcsr_type_real_8, C.byref(a), C.byref(d), st.ptr) == -1
    e = empty.desc()
    assert eng.L.dbcsr_amd_bcsr_reblock_gather(eng.h, L.dbcsr_type_real_8, C.byref(a), C.byref(e), st.ptr) == 0, "a dst without blocks: nothing done"
    torch.cuda.synchronize()
    assert same_bits(host(out.data), before) and same_bits(host(dA.data), A.data)


# ---- 8. every refusal of the Python layer ----------------------------------------------------------------------------------------------------------------------
def test_refusals(eng, monkeypatch):
    from dbcsr_amd import reblock as RB

    def no_engine():
        raise AssertionError("a refusal must come before any call of the library")
    monkeypatch.setattr(RB, "default_engine", no_engine)
    A = R.source("partial", "float64")
    dA = to_dev(A)
    rs, cs = R.STRUCTURES["u32"]
    area = host(dA.data).copy()
    for bad_rs, bad_cs in ((rs[:-1], cs), (rs, cs + [1]), (rs[:-1] + [rs[-1] + 1], cs)):
        with pytest.raises(ValueError, match="sums to"):
            dbcsr_reblock(dA, bad_rs, bad_cs)
    with pytest.raises(ValueError, match="sums to"):
        dbcsr_reblock(dA, torch.as_tensor(np.asarray(rs[:-1], np.int32)).cuda(), cs)
    for bad in (rs[:-1] + [rs[-1] + 1, -1], [0] + rs, torch.as_tensor(np.asarray([0] + rs, np.int32)).cuda()):
        with pytest.raises(ValueError, match="below 1"):
            dbcsr_reblock(dA, bad, cs)
    with pytest.raises(TypeError):
        dbcsr_reblock(dA, [32.5] * 4, cs)
    hA = DbcsrMatrix(*(x.cpu() for x in (dA.row_blk_size, dA.col_blk_size, dA.row_p, dA.col_i, dA.blk_p, dA.data)))
    with pytest.raises(ValueError, match="on the host"):
        dbcsr_reblock(hA, rs, cs)
    X = to_dev(A)
    X.symmetry = "X"
    with pytest.raises(ValueError, match="symmetry"):
        dbcsr_reblock(X, rs, cs)
    # dbcsr_reblock_into
    T = R.half_pattern(A, rs, cs)
    dT = to_dev(T)
    for m_in, m_out in ((hA, dT), (dA, hA)):
        with pytest.raises(ValueError, match="on the host"):
            dbcsr_reblock_into(m_in, m_out)
    for m_in, m_out in ((X, dT), (dA, X)):
        with pytest.raises(ValueError, match="symmetry"):
            dbcsr_reblock_into(m_in, m_out)
    with pytest.raises(TypeError, match="data types"):
        dbcsr_reblock_into(dA, to_dev(R.half_pattern(R.source("partial", "float32"), rs, cs)))
    with pytest.raises(ValueError, match="sum to"):
        dbcsr_reblock_into(dA, to_dev(R.half_pattern(A, rs[:-1], cs)))
    with pytest.raises(ValueError, match="sum to"):
        dbcsr_reblock_into(dA, to_dev(R.half_pattern(A, rs, cs[:-1])))
    with pytest.raises(ValueError, match="share a data area"):
        dbcsr_reblock_into(dA, dA)
    shared = DbcsrMatrix(dT.row_blk_size, dT.col_blk_size, dT.row_p, dT.col_i, dT.blk_p, dA.data[:T.data.size]) if T.data.size <= A.data.size else None
    view = DbcsrMatrix(dA.row_blk_size, dA.col_blk_size, dA.row_p, dA.col_i, dA.blk_p, dA.data[:])
    for m_out in (view, shared):
        if m_out is not None:
            with pytest.raises(ValueError, match="share a data area"):
                dbcsr_reblock_into(dA, m_out)
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="different devices"):
            dbcsr_reblock_into(dA, DbcsrMatrix(*(x.to("cuda:1") for x in (dT.row_blk_size, dT.col_blk_size, dT.row_p, dT.col_i, dT.blk_p, dT.data))))
    torch.cuda.synchronize()
    assert same_bits(host(dA.data), area)
