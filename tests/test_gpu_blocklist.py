"""Block lists on the device: dbcsr_reserve_blocks, dbcsr_put_blocks, dbcsr_get_blocks and what is built on them, for float64, float32 and complex128.

The reference is the dict of numpy blocks of tests/test_blocklist_cpu.py, which goes through a list entry by entry in list order; that file also checks
that its matrices and lists are able to make these tests fail (reversing the order of the duplicates changes bits, the mixes hold present and absent
blocks).  With alpha == 1 everything is compared bit for bit -- index arrays, data, the sign of a zero.  With another alpha the bar per element is
u (k + 2) (|old| + sum |alpha| |x|), u the unit roundoff of the type and k the number of contributions (ref_put_wide there derives it); the reference
is formed in long double, and of a complex element the real and the imaginary part are each held to the bar.

Matrices: 31, 32, 33, 64 and 65 block columns of the sizes 13, 5, 7 (both sides of a bitmap word); blocks of 1 and 3 (float32 blocks shorter than a
16-byte pack) with 136 and 75 blocks in a block row; blocks of 23; blocks of 33 and 80; an empty block row in each; a matrix with no block; a matrix
left unpacked by an in-place filter.  Lists: none, one, a permutation of the pattern, present only, absent only, a mix, one block hit 3, 65 and 130
times; sources that start at element 1 (odd offsets) and sources with gaps."""
import ctypes as C

import numpy as np
import pytest
import torch

import dbcsr_amd
from dbcsr_amd import operations as OPS
from dbcsr_amd.matrix import DbcsrMatrix, StreamHandle
from dbcsr_amd.multiply import MultiplyEngine, _z, dbcsr_multiply
from dbcsr_amd.operations import (dbcsr_create_from_blocks, dbcsr_frobenius_norm, dbcsr_get_blocks, dbcsr_put_blocks, dbcsr_rank_update,
                                  dbcsr_reserve_all_blocks, dbcsr_reserve_blocks, dbcsr_reserve_diag_blocks)
from tests.gpu_util import dev_to_bcsr, to_dev
from tests.test_blocklist_cpu import (DTYPES, DUPLICATES, IDS, LISTS, MATRICES, NAMES, ODD, block_sizes, is_complex, lay_out, make_list, make_matrix,
                                      make_windows, ref_get, ref_put, ref_put_wide, ref_reserve, values)
from tests.test_gpu_matrix_norms import TORCH, blocks_of, dense, from_blocks, hole_positions, pattern_mask, product_bar, same_bits, with_holes
from tests.test_gpu_rank_update import reference as rank_reference
from tests.test_gpu_rank_update import stored_within, wide
from tests.test_gpu_multivec import random_vectors

pytestmark = pytest.mark.gpu

POISON = -7.25e33
STYLES = ("odd", "gaps")


@pytest.fixture(scope="module")
def eng():
    return MultiplyEngine()


def i32(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.int32)).cuda()


def i64(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.int64)).cuda()


def dev_matrix(rs, cs, blocks, dtype):
    if not blocks:
        return DbcsrMatrix.empty_like_pattern(i32(rs), i32(cs), TORCH[np.dtype(dtype)])
    return to_dev(from_blocks(rs, cs, blocks, dtype))


def index_of(dM):
    return (dM.row_p, dM.col_i, dM.blk_p, dM.data)


def snapshot(dM):
    return [t.clone() for t in index_of(dM)]


def untouched(dM, tensors, copies, stamp):
    """the same tensor objects, the same stamp, not a bit changed against the copies taken before"""
    torch.cuda.synchronize()
    assert all(t is u for t, u in zip(index_of(dM), tensors)) and dM.index_stamp() == stamp
    return all(same_bits(t.cpu().numpy(), c.cpu().numpy()) for t, c in zip(tensors, copies))


def equals_blocks(dM, rs, cs, blocks, dtype):
    """the device matrix is the packed matrix of these blocks: index arrays equal, data bit for bit"""
    torch.cuda.synchronize()
    got, want = dev_to_bcsr(dM), from_blocks(rs, cs, blocks, dtype)
    assert np.array_equal(got.row_p, want.row_p) and np.array_equal(got.col_i, want.col_i) and np.array_equal(got.blk_p, want.blk_p)
    assert dM.packed and same_bits(got.data, want.data.astype(dtype))


def source(rs, cs, rows, cols, dtype, style, seed=9):
    wins = make_windows(rs, cs, rows, cols, dtype, seed)
    flat, off = lay_out(wins, style, dtype, POISON)
    return wins, torch.as_tensor(flat).cuda(), i64(off)


def holes_matrix(eng, dtype):
    """(row sizes, column sizes, host matrix with the device's index, device matrix): unpacked, every element its index does not name poisoned"""
    rs, cs, blocks = make_matrix("w33", dtype)
    hM, dM = with_holes(eng, from_blocks(rs, cs, blocks, dtype), dtype)
    holes = hole_positions(hM)
    assert holes.size > 0 and not dM.packed, "the matrix really has holes"
    dM.data[torch.as_tensor(holes).cuda()] = POISON
    torch.cuda.synchronize()
    return rs, cs, dev_to_bcsr(dM), dM


def holes_kept(dM, hM):
    torch.cuda.synchronize()
    got = dM.data.cpu().numpy()
    return np.all(got[hole_positions(hM)] == np.asarray(POISON, got.dtype))


# ---- reserve ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", sorted(MATRICES))
def test_reserve(eng, name, dtype):
    rs, cs, blocks = make_matrix(name, dtype)
    for kind in LISTS:
        rows, cols = make_list(kind, rs, cs, blocks)
        dM = dev_matrix(rs, cs, blocks, dtype)
        tensors, copies, stamp = index_of(dM), snapshot(dM), dM.index_stamp()
        want, n_new = ref_reserve(rs, cs, blocks, rows, cols)
        assert dbcsr_reserve_blocks(dM, i32(rows), i32(cols), engine=eng) == n_new, kind
        if n_new == 0:
            assert untouched(dM, tensors, copies, stamp), kind
        else:
            assert dM.index_stamp() != stamp
            equals_blocks(dM, rs, cs, want, dtype)   # (old blocks bit for bit, new blocks +0.0: the bytes of the reference's zeros)
            assert all(same_bits(t.cpu().numpy(), c.cpu().numpy()) for t, c in zip(tensors, copies)), "the old arrays are not written"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_reserve_on_an_unpacked_matrix(eng, dtype):
    rs, cs, hM, dM = holes_matrix(eng, dtype)
    blocks = blocks_of(hM)
    rows, cols = make_list("perm", rs, cs, blocks)
    tensors, copies, stamp = index_of(dM), snapshot(dM), dM.index_stamp()
    assert dbcsr_reserve_blocks(dM, i32(rows), i32(cols), engine=eng) == 0
    assert untouched(dM, tensors, copies, stamp) and holes_kept(dM, hM)
    rows, cols = make_list("mix", rs, cs, blocks)
    want, n_new = ref_reserve(rs, cs, blocks, rows, cols)
    assert n_new > 0 and dbcsr_reserve_blocks(dM, i32(rows), i32(cols), engine=eng) == n_new
    equals_blocks(dM, rs, cs, want, dtype)   # (packed: the holes are gone, the blocks kept their bits)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_reserve_refuses_coordinates_outside_and_below_the_diagonal(eng, dtype):
    rs, cs, blocks = make_matrix("w33", dtype)
    for bad in ((len(rs), 0), (0, len(cs)), (-1, 3), (3, -1), (2 ** 31 - 1, 0)):
        dM = dev_matrix(rs, cs, blocks, dtype)
        tensors, copies, stamp = index_of(dM), snapshot(dM), dM.index_stamp()
        rows, cols = make_list("mix", rs, cs, blocks)
        rows, cols = np.concatenate([rows[:5], [bad[0]], rows[5:]]), np.concatenate([cols[:5], [bad[1]], cols[5:]])
        with pytest.raises(ValueError):
            dbcsr_reserve_blocks(dM, i32(rows), i32(cols), engine=eng)
        assert untouched(dM, tensors, copies, stamp)
    sizes = block_sizes(ODD, 7)
    rng = np.random.default_rng(17)
    upper = {(r, c): values(rng, int(sizes[r]) * int(sizes[c]), dtype) for r in range(7) for c in range(r, 7) if (r + c) % 3 != 1}
    for symmetry in (("H", "K") if is_complex(dtype) else ("S", "A")):
        dM = dev_matrix(sizes, sizes, upper, dtype)
        dM.symmetry = symmetry
        tensors, copies, stamp = index_of(dM), snapshot(dM), dM.index_stamp()
        with pytest.raises(ValueError):
            dbcsr_reserve_blocks(dM, i32([0, 4, 1]), i32([1, 2, 1]), engine=eng)   # (4, 2) lies below the diagonal
        assert untouched(dM, tensors, copies, stamp)
        want, n_new = ref_reserve(sizes, sizes, upper, [0, 1, 1, 0], [1, 3, 3, 0], upper_only=True)
        assert n_new == 2 and dbcsr_reserve_blocks(dM, i32([0, 1, 1, 0]), i32([1, 3, 3, 0]), engine=eng) == 2
        equals_blocks(dM, sizes, sizes, want, dtype)
        assert dM.symmetry == symmetry
        assert dbcsr_reserve_all_blocks(dM, engine=eng) == 28 - len(want) and dM.nblks == 28


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_reserve_diag_and_all(eng, dtype):
    rs, cs, blocks = make_matrix("w31", dtype)
    dM = dev_matrix(rs, cs, blocks, dtype)
    diag = [(i, i) for i in range(len(rs))]
    want, n_new = ref_reserve(rs, cs, blocks, [d[0] for d in diag], [d[1] for d in diag])
    assert n_new > 0 and dbcsr_reserve_diag_blocks(dM, engine=eng) == n_new
    equals_blocks(dM, rs, cs, want, dtype)
    everything = [(r, c) for r in range(len(rs)) for c in range(len(cs))]
    full, n_new = ref_reserve(rs, cs, want, [e[0] for e in everything], [e[1] for e in everything])
    assert dbcsr_reserve_all_blocks(dM, engine=eng) == n_new
    equals_blocks(dM, rs, cs, full, dtype)
    assert dbcsr_reserve_all_blocks(dM, engine=eng) == 0 and dbcsr_reserve_diag_blocks(dM, engine=eng) == 0


# ---- put ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", sorted(MATRICES))
def test_put_bit_for_bit(eng, name, dtype):
    """alpha == 1: overwrite and summation in list order, the pattern growing where the list names new blocks; the 3, 65 and 130 duplicates among them"""
    rs, cs, blocks = make_matrix(name, dtype)
    for n, kind in enumerate(LISTS):
        rows, cols = make_list(kind, rs, cs, blocks)
        wins, data, off = source(rs, cs, rows, cols, dtype, STYLES[n % 2])
        for summation in (False, True):
            dM = dev_matrix(rs, cs, blocks, dtype)
            assert dbcsr_put_blocks(dM, i32(rows), i32(cols), data, off, summation=summation, engine=eng) is None
            equals_blocks(dM, rs, cs, ref_put(rs, cs, blocks, rows, cols, wins, dtype, summation=summation), dtype)
        if kind in ("mix", "dup65"):   # offsets left to the call: the windows one after another
            packed = torch.as_tensor(np.concatenate(wins)).cuda()
            dM = dev_matrix(rs, cs, blocks, dtype)
            dbcsr_put_blocks(dM, i32(rows), i32(cols), packed, summation=True, engine=eng)
            equals_blocks(dM, rs, cs, ref_put(rs, cs, blocks, rows, cols, wins, dtype, summation=True), dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["w33", "tiny", "big"])
def test_put_keep_sparsity(eng, name, dtype):
    """entries whose block is absent (or outside the matrix) are skipped; no index tensor is touched"""
    rs, cs, blocks = make_matrix(name, dtype)
    for kind in ("absent", "mix", "dup3", "dup130"):
        rows, cols = make_list(kind, rs, cs, blocks)
        rows, cols = np.concatenate([rows, [len(rs), -1]]).astype(np.int32), np.concatenate([cols, [0, 0]]).astype(np.int32)   # + two entries outside
        flat_rows, flat_cols = np.clip(rows, 0, len(rs) - 1), cols
        wins, data, off = source(rs, cs, flat_rows, flat_cols, dtype, "gaps")
        for summation in (False, True):
            dM = dev_matrix(rs, cs, blocks, dtype)
            index, copies, stamp = index_of(dM)[:3], snapshot(dM)[:3], dM.index_stamp()
            dbcsr_put_blocks(dM, i32(rows), i32(cols), data, off, summation=summation, keep_sparsity=True, engine=eng)
            assert untouched(dM, index + (dM.data,), copies + [dM.data.clone()], stamp)
            equals_blocks(dM, rs, cs, ref_put(rs, cs, blocks, rows, cols, wins, dtype, summation=summation, keep_sparsity=True), dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["w33", "tiny", "big"])
def test_put_with_a_scale(eng, name, dtype):
    """alpha != 1, real and complex: within u (k + 2) (|old| + sum |alpha| |x|) per element of a reference in long double"""
    rs, cs, blocks = make_matrix(name, dtype)
    alphas = (-1.75, 0.75 - 1.25j) if is_complex(dtype) else (-1.75,)   # (exact in float32: what the bar allows alpha's own rounding is left unused)
    for kind in ("perm", "mix", "dup3", "dup65", "dup130"):
        rows, cols = make_list(kind, rs, cs, blocks)
        wins, data, off = source(rs, cs, rows, cols, dtype, "odd")
        for alpha in alphas:
            for summation in (False, True):
                dM = dev_matrix(rs, cs, blocks, dtype)
                dbcsr_put_blocks(dM, i32(rows), i32(cols), data, off, summation=summation, alpha=alpha, keep_sparsity=True, engine=eng)
                torch.cuda.synchronize()
                got = blocks_of(dev_to_bcsr(dM))
                ref, bar = ref_put_wide(rs, cs, blocks, rows, cols, wins, dtype, summation, alpha)
                assert sorted(got) == sorted(ref)
                worst = 0.0
                for k in ref:
                    err = got[k].astype(wide(dtype)) - ref[k]
                    parts = (np.abs(err.real), np.abs(err.imag)) if is_complex(dtype) else (np.abs(err),)
                    for e in parts:
                        e = e.astype(np.float64)
                        worst = max(worst, float(np.max(e / np.maximum(bar[k], 1e-300))))
                        assert np.all(e <= bar[k]), (kind, alpha, summation, k)
                print("%s alpha %r summation %d: worst error %.3f of its bar" % (kind, alpha, summation, worst))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_put_gives_the_same_bits_every_time(eng, dtype):
    rs, cs, blocks = make_matrix("w65", dtype)
    rows, cols = make_list("dup130", rs, cs, blocks)
    wins, data, off = source(rs, cs, rows, cols, dtype, "gaps")
    first = None
    for it in range(5):
        dM = dev_matrix(rs, cs, blocks, dtype)
        dbcsr_put_blocks(dM, i32(rows), i32(cols), data, off, summation=True, alpha=0.3, engine=eng)
        torch.cuda.synchronize()
        got = dM.data.cpu().numpy()
        first = got if first is None else first
        assert same_bits(got, first), it


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_put_onto_an_unpacked_matrix_keeps_the_holes(eng, dtype):
    rs, cs, hM, dM = holes_matrix(eng, dtype)
    blocks = blocks_of(hM)
    start = dM.data.clone()
    for kind in ("perm", "mix", "dup65"):
        rows, cols = make_list(kind, rs, cs, blocks)
        wins, data, off = source(rs, cs, rows, cols, dtype, "odd")
        for summation in (False, True):
            dM.data.copy_(start)
            index, copies, stamp = index_of(dM)[:3], snapshot(dM)[:3], dM.index_stamp()
            dbcsr_put_blocks(dM, i32(rows), i32(cols), data, off, summation=summation, keep_sparsity=True, engine=eng)
            assert untouched(dM, index + (dM.data,), copies + [dM.data.clone()], stamp) and holes_kept(dM, hM)
            got, want = blocks_of(dev_to_bcsr(dM)), ref_put(rs, cs, blocks, rows, cols, wins, dtype, summation=summation, keep_sparsity=True)
            assert sorted(got) == sorted(want) and all(same_bits(np.ascontiguousarray(got[k]), want[k]) for k in want)


def test_put_refuses_a_source_inside_the_matrix(eng):
    rs, cs, blocks = make_matrix("b23", np.float64)
    dM = dev_matrix(rs, cs, blocks, np.float64)
    tensors, copies, stamp = index_of(dM), snapshot(dM), dM.index_stamp()
    rows, cols = make_list("present", rs, cs, blocks)
    with pytest.raises(ValueError):
        dbcsr_put_blocks(dM, i32(rows), i32(cols), dM.data[7:], engine=eng)
    with pytest.raises(ValueError):
        dbcsr_get_blocks(dM, i32(rows), i32(cols), out=dM.data, engine=eng)
    assert untouched(dM, tensors, copies, stamp)


def test_a_window_that_leaves_the_source_is_skipped(eng):
    """nothing is read behind the end of data: the entry is skipped as one outside the matrix is"""
    rs, cs, blocks = make_matrix("b23", np.float64)
    rows, cols = make_list("present", rs, cs, blocks)
    wins, data, off = source(rs, cs, rows, cols, np.float64, "odd")
    short = data[:int(off[-1]) + 5].clone()   # (the last window is cut)
    dM = dev_matrix(rs, cs, blocks, np.float64)
    dbcsr_put_blocks(dM, i32(rows), i32(cols), short, off, engine=eng)
    equals_blocks(dM, rs, cs, ref_put(rs, cs, blocks, rows[:-1], cols[:-1], wins[:-1], np.float64), np.float64)


# ---- get ----------------------------------------------------------------------------------------------------------------------------------------------------
def check_get(eng, dM, rs, cs, blocks, rows, cols, dtype, style):
    wins, found = ref_get(rs, cs, blocks, rows, cols, dtype)
    data, got_found = dbcsr_get_blocks(dM, i32(rows), i32(cols), engine=eng)
    torch.cuda.synchronize()
    assert got_found.dtype == torch.int32 and np.array_equal(got_found.cpu().numpy(), found)
    assert same_bits(data.cpu().numpy(), np.concatenate(wins + [np.zeros(0, dtype)]))   # (stored blocks bit for bit, absent windows +0.0)
    want, off = lay_out(wins, style, dtype, POISON)
    out = torch.full((want.size,), POISON, dtype=TORCH[np.dtype(dtype)], device="cuda")
    data, got_found = dbcsr_get_blocks(dM, i32(rows), i32(cols), out=out, offsets=i64(off), engine=eng)
    torch.cuda.synchronize()
    assert data is out and np.array_equal(got_found.cpu().numpy(), found)
    assert same_bits(out.cpu().numpy(), want), "the windows, and the poison between and around them"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", sorted(MATRICES))
def test_get(eng, name, dtype):
    rs, cs, blocks = make_matrix(name, dtype)
    dM = dev_matrix(rs, cs, blocks, dtype)
    tensors, copies, stamp = index_of(dM), snapshot(dM), dM.index_stamp()
    for n, kind in enumerate(LISTS):
        rows, cols = make_list(kind, rs, cs, blocks)
        if kind == "mix":   # + coordinates outside the matrix: no window, found = 0
            rows, cols = np.concatenate([rows, [len(rs), 0, -1]]).astype(np.int32), np.concatenate([cols, [1, len(cs), 2]]).astype(np.int32)
        check_get(eng, dM, rs, cs, blocks, rows, cols, dtype, STYLES[n % 2])
    assert untouched(dM, tensors, copies, stamp)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_get_from_an_unpacked_matrix(eng, dtype):
    rs, cs, hM, dM = holes_matrix(eng, dtype)
    blocks = blocks_of(hM)
    for kind in ("perm", "mix"):
        rows, cols = make_list(kind, rs, cs, blocks)
        check_get(eng, dM, rs, cs, blocks, rows, cols, dtype, "gaps")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_get_of_put_round_trips(eng, dtype):
    rs, cs, blocks = make_matrix("w64", dtype)
    for kind in ("perm", "absent", "mix"):
        rows, cols = make_list(kind, rs, cs, blocks)
        rows, cols = (lambda u: (u[:, 0].astype(np.int32), u[:, 1].astype(np.int32)))(np.asarray(sorted(set(zip(rows.tolist(), cols.tolist())))[::-1]))
        wins, data, off = source(rs, cs, rows, cols, dtype, "gaps")
        dM = dev_matrix(rs, cs, blocks, dtype)
        dbcsr_put_blocks(dM, i32(rows), i32(cols), data, off, engine=eng)
        back = torch.full_like(data, POISON)
        _, found = dbcsr_get_blocks(dM, i32(rows), i32(cols), out=back, offsets=off, engine=eng)
        torch.cuda.synchronize()
        assert bool(found.all()) and same_bits(back.cpu().numpy(), data.cpu().numpy())


# ---- create_from_blocks ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["w32", "tiny", "big"])
def test_create_from_blocks_equals_from_host_of_the_numpy_assembly(eng, name, dtype):
    rs, cs, blocks = make_matrix(name, dtype)
    for kind in ("perm", "mix", "dup65"):
        rows, cols = make_list(kind, rs, cs, blocks)
        wins, data, off = source(rs, cs, rows, cols, dtype, "odd")
        for summation in (True, False):
            M = dbcsr_create_from_blocks(rs, cs, i32(rows), i32(cols), data, off, summation=summation, name="made", engine=eng)
            assert M.name == "made" and M.symmetry == "N" and M.row_blk_size.dtype == torch.int32
            equals_blocks(M, rs, cs, ref_put(rs, cs, {}, rows, cols, wins, dtype, summation=summation), dtype)
    M = dbcsr_create_from_blocks(i32(rs), i32(cs), i32([]), i32([]), torch.zeros(0, dtype=TORCH[np.dtype(dtype)], device="cuda"), engine=eng)
    assert M.nblks == 0 and M.nblkrows == len(rs)


# ---- a multiply before and after ----------------------------------------------------------------------------------------------------------------------------
def test_put_and_reserve_between_multiplies_keep_the_plan(monkeypatch):
    monkeypatch.delenv("DBCSR_AMD_MM_PLAN", raising=False)
    eng = MultiplyEngine()
    dtype = np.float64
    sizes = block_sizes(ODD, 24)
    rng = np.random.default_rng(23)
    pattern = lambda p: {(r, c): values(rng, int(sizes[r]) * int(sizes[c]), dtype) for r in range(24) for c in range(24) if rng.random() < p}
    a_blocks, b_blocks = pattern(0.4), pattern(0.5)
    dA, dB = dev_matrix(sizes, sizes, a_blocks, dtype), dev_matrix(sizes, sizes, b_blocks, dtype)
    empty = lambda: DbcsrMatrix.empty_like_pattern(dA.row_blk_size, dA.col_blk_size, torch.float64)
    dC = empty()
    dbcsr_multiply("N", "N", 1.0, dA, dB, 0.0, dC, engine=eng)
    assert eng.plan_stats() == (0, 1)

    def fresh_product():
        other, out = MultiplyEngine(), empty()
        for _ in range(2):   # (as here: the second product onto the pattern of the first)
            dbcsr_multiply("N", "N", 1.0, dA, dB, 0.0, out, engine=other)
        torch.cuda.synchronize()
        return dev_to_bcsr(out)

    def same_as_fresh():
        torch.cuda.synchronize()
        got, want = dev_to_bcsr(dC), fresh_product()
        return np.array_equal(got.row_p, want.row_p) and np.array_equal(got.col_i, want.col_i) and same_bits(got.data, want.data)

    # 1. a put onto stored blocks of an operand (through the reserve that finds nothing to do)
    rows, cols = make_list("present", sizes, sizes, a_blocks)
    wins, data, off = source(sizes, sizes, rows, cols, dtype, "odd")
    stamp = dA.index_stamp()
    dbcsr_put_blocks(dA, i32(rows), i32(cols), data, off, summation=True, engine=eng)
    a_blocks = ref_put(sizes, sizes, a_blocks, rows, cols, wins, dtype, summation=True)
    assert dA.index_stamp() == stamp
    dbcsr_multiply("N", "N", 1.0, dA, dB, 0.0, dC, engine=eng)
    assert eng.plan_stats() == (1, 1), "a multiply after a put onto stored blocks must reuse its plan"
    assert same_as_fresh()
    # 2. a reserve of stored blocks
    rows, cols = make_list("perm", sizes, sizes, a_blocks)
    assert dbcsr_reserve_blocks(dA, i32(rows), i32(cols), engine=eng) == 0 and dA.index_stamp() == stamp
    dbcsr_multiply("N", "N", 1.0, dA, dB, 0.0, dC, engine=eng)
    assert eng.plan_stats() == (2, 1), "a multiply after a reserve of stored blocks must reuse its plan"
    assert same_as_fresh()
    equals_blocks(dA, sizes, sizes, a_blocks, dtype)
    # 3. a reserve that creates blocks, filled by a put: the multiply runs its symbolic phase and matches the dense product
    rows, cols = make_list("mix", sizes, sizes, a_blocks)
    wins, data, off = source(sizes, sizes, rows, cols, dtype, "gaps")
    assert dbcsr_reserve_blocks(dA, i32(rows), i32(cols), engine=eng) > 0 and dA.index_stamp() != stamp
    dbcsr_put_blocks(dA, i32(rows), i32(cols), data, off, keep_sparsity=True, engine=eng)
    a_blocks = ref_put(sizes, sizes, a_blocks, rows, cols, wins, dtype)
    equals_blocks(dA, sizes, sizes, a_blocks, dtype)
    dbcsr_multiply("N", "N", 1.0, dA, dB, 0.0, dC, engine=eng)
    assert eng.plan_stats() == (2, 2), "a grown pattern: the symbolic phase runs"
    torch.cuda.synchronize()
    product_bar(dev_to_bcsr(dC), 1.0, dense(from_blocks(sizes, sizes, a_blocks, dtype)), dense(from_blocks(sizes, sizes, b_blocks, dtype)))


# ---- the two halves of the reserve in C ---------------------------------------------------------------------------------------------------------------------
def c_count(eng, dM, rows, cols, upper_only=0):
    a, st = dM.desc(), StreamHandle()
    row_p = torch.full((dM.nblkrows + 1,), -77, dtype=torch.int32, device="cuda")
    nb, nz, new, bad = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
    rc = eng.L.dbcsr_amd_bcsr_reserve_count(eng.h, C.byref(a), int(rows.numel()), rows.data_ptr(), cols.data_ptr(), upper_only, row_p.data_ptr(),
                                            C.byref(nb), C.byref(nz), C.byref(new), C.byref(bad), st.ptr)
    return rc, row_p, nb.value, nz.value, new.value, bad.value


def poisoned_result(dM, row_p, nblks, nze):
    return DbcsrMatrix(dM.row_blk_size, dM.col_blk_size, row_p, torch.full((nblks,), -77, dtype=torch.int32, device="cuda"),
                       torch.full((nblks,), -77, dtype=torch.int64, device="cuda"), torch.full((nze,), POISON, dtype=dM.dtype, device="cuda"))


def c_apply(eng, dM, out):
    a, dst, st = dM.desc(), out.desc(out=True), StreamHandle()
    rc = eng.L.dbcsr_amd_bcsr_reserve_apply(eng.h, dM.dtype_code, C.byref(a), C.byref(dst), st.ptr)
    torch.cuda.synchronize()
    return rc


def still_poisoned(out):
    return bool((out.col_i == -77).all()) and bool((out.blk_p == -77).all()) and bool((out.data == POISON).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_two_halves_of_the_reserve(dtype):
    eng = MultiplyEngine()   # (a fresh handle: nothing was ever counted on it)
    rs, cs, blocks = make_matrix("w33", dtype)
    rows, cols = make_list("mix", rs, cs, blocks)
    want, n_new = ref_reserve(rs, cs, blocks, rows, cols)
    shape = from_blocks(rs, cs, want, dtype)
    dM, dOther = dev_matrix(rs, cs, blocks, dtype), dev_matrix(rs, cs, blocks, dtype)   # (another matrix with the same sizes and block count)
    r, c = i32(rows), i32(cols)
    # an apply without a count
    out = poisoned_result(dM, torch.full((len(rs) + 1,), -77, dtype=torch.int32, device="cuda"), shape.nblks, shape.data.size)
    assert c_apply(eng, dM, out) == -1 and still_poisoned(out)
    # a count that finds nothing new leaves nothing to apply
    pr, pc = make_list("perm", rs, cs, blocks)
    rc, row_p, nb, nz, new, bad = c_count(eng, dM, i32(pr), i32(pc))
    assert (rc, new, bad) == (0, 0, 0) and bool((row_p == -77).all())
    assert c_apply(eng, dM, out) == -1 and still_poisoned(out)
    # a count with coordinates outside reports them and leaves nothing to apply
    rc, row_p, nb, nz, new, bad = c_count(eng, dM, i32([0, len(rs), 1]), i32([0, 0, len(cs)]))
    assert (rc, bad) == (0, 2) and c_apply(eng, dM, out) == -1 and still_poisoned(out)
    # an apply after a count for another matrix; the count is then used up
    rc, row_p, nb, nz, new, bad = c_count(eng, dM, r, c)
    assert (rc, nb, nz, new, bad) == (0, shape.nblks, shape.data.size, n_new, 0)
    out = poisoned_result(dM, row_p, nb, nz)
    assert c_apply(eng, dOther, out) == -1 and still_poisoned(out)
    assert c_apply(eng, dM, out) == -1 and still_poisoned(out)
    # a put, a get and a norm between the two halves
    rc, row_p, nb, nz, new, bad = c_count(eng, dM, r, c)
    assert (rc, nb, nz, new) == (0, shape.nblks, shape.data.size, n_new)
    pr, pc = make_list("dup65", rs, cs, blocks)
    wins, data, off = source(rs, cs, pr, pc, dtype, "odd")
    dbcsr_put_blocks(dM, i32(pr), i32(pc), data, off, summation=True, keep_sparsity=True, engine=eng)
    changed = ref_put(rs, cs, blocks, pr, pc, wins, dtype, summation=True, keep_sparsity=True)
    dbcsr_get_blocks(dM, r, c, engine=eng)
    dbcsr_frobenius_norm(dM, engine=eng)
    out = poisoned_result(dM, row_p, nb, nz)
    assert c_apply(eng, dM, out) == 0
    equals_blocks(out, rs, cs, ref_reserve(rs, cs, changed, rows, cols)[0], dtype)
    assert c_apply(eng, dM, poisoned_result(dM, row_p, nb, nz)) == -1, "one apply per count"


# ---- composition -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_rank_update_onto_a_reserved_pattern(eng, dtype):
    """the missing half of dbcsr_rank_update: the pattern is made on the device, then A <- alpha X Y^T on it, against the rank update's own bar"""
    rs, cs, blocks = make_matrix("w33", dtype)
    rows, cols = make_list("perm", rs, cs, blocks)
    dM = DbcsrMatrix.empty_like_pattern(i32(rs), i32(cs), TORCH[np.dtype(dtype)])
    assert dbcsr_reserve_blocks(dM, i32(rows), i32(cols), engine=eng) == len(blocks)
    hM = dev_to_bcsr(dM)
    assert not np.any(hM.data)
    nrhs, alpha = 5, (0.7 - 0.4j if is_complex(dtype) else -1.3)
    x, y = random_vectors(int(rs.sum()), nrhs, dtype, 61), random_vectors(int(cs.sum()), nrhs, dtype, 62)
    dbcsr_rank_update(dM, torch.as_tensor(x).cuda(), torch.as_tensor(y).cuda(), alpha, 1.0, "T", engine=eng)
    torch.cuda.synchronize()
    F = dense(hM).astype(wide(dtype))
    ref, bar = rank_reference(F, np.abs(F).astype(np.float64), alpha, 1.0, x, y, "T")
    stored_within(dM.data.cpu().numpy(), hM, ref, bar, pattern_mask(hM), "a rank update onto a reserved pattern")


def test_the_package_exports_the_operations():
    for name in NAMES:
        assert getattr(dbcsr_amd, name) is getattr(OPS, name) and name in dbcsr_amd.__all__
