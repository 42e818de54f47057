"""Block-sparse tensors on the device (dbcsr_amd/tensor.py, dbcsr_amd_tensor_permute_blocks of include/dbcsr_amd_mm.h, kernel of
dbcsr_amd/csrc/mm_tensor.h) against tests/tensor_ref.py, for float64, float32 and complex128.  The inputs are those of tests/tensor_cases.py; the
conditions they meet are checked without a GPU in tests/test_tensor_cpu.py.

1. the kernel through the C entry: every permutation of ranks 2, 3 and 4, bit for bit, canaries, skipped windows, return codes, offsets above 2^32;
2. put / get round trips and dbcsr_t_block_indices on every listed mapping;
3. dbcsr_t_copy between mappings, with and without order and summation;
4. dbcsr_t_contract against the block-wise reference: index and flop exact, every element within the bar gamma (|alpha| sum |T1| |T2| + |beta| |T3|)
   of tests/option_sweep.py -- the remaps move bits and add no rounding;
5. the matrix interface on a tensor's matrix, and matrices with symmetry into tensors and back."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import dbcsr_amd.tensor as T
from dbcsr_amd import (dbcsr_frobenius_norm, dbcsr_scale, dbcsr_t_block_indices, dbcsr_t_contract, dbcsr_t_copy,
                       dbcsr_t_copy_matrix_to_tensor, dbcsr_t_copy_tensor_to_matrix, dbcsr_t_create, dbcsr_t_create_from_blocks, dbcsr_t_filter,
                       dbcsr_t_get_blocks, dbcsr_t_put_blocks, dbcsr_to_dense)
from dbcsr_amd.matrix import DbcsrMatrix, StreamHandle, _dtype_code
from dbcsr_amd.multiply import dbcsr_multiply, default_engine
from tests import far_arena
from tests import tensor_cases as TC
from tests import tensor_ref as TR
from tests.option_sweep import LONG_DOUBLE_OK, gamma_of

pytestmark = pytest.mark.gpu

TORCH = {TC.F64: torch.float64, TC.F32: torch.float32, TC.Z64: torch.complex128}
CANARY_BYTE = 0xA5


def gpu(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def host(t):
    return t.detach().cpu().numpy()


# ---- 1. the kernel through the C entry ----------------------------------------------------------------------------------------------------------------------------
def permute(dtype, perm, ext, src_off, dst_off, src, src_len, dst, dst_len, nblk=None, rank=None, code=None, handle=True):
    E = default_engine()
    st = StreamHandle()
    rank = len(perm) if rank is None else rank
    p = (C.c_int * max(len(perm), 1))(*perm)
    ptr = lambda t: None if t is None else t.data_ptr()
    return E.L.dbcsr_amd_tensor_permute_blocks(E.h if handle else None, _dtype_code(TORCH[dtype]) if code is None else code,
                                               (int(ext.shape[0]) if ext is not None else 1) if nblk is None else nblk, rank, p, ptr(ext), ptr(src_off), ptr(dst_off), ptr(src), src_len,
                                               ptr(dst), dst_len, st.ptr)


def random_bits(rng, n, dtype):
    """n elements of random bit patterns (NaN payloads, denormals, infinities among them): the move must not look at them"""
    return np.frombuffer(rng.bytes(n * np.dtype(dtype).itemsize), dtype=dtype).copy()


def padded(exts):
    out = np.ones((len(exts), 4), np.int32)
    for b, e in enumerate(exts):
        out[b, :len(e)] = e
    return out


def expected_windows(dst0, src, exts, perm, src_off, dst_off):
    want = dst0.copy()
    for e, so, do in zip(exts, src_off, dst_off):
        n = int(np.prod(e))
        want[do:do + n] = np.transpose(src[so:so + n].reshape(e, order="F"), perm).reshape(-1, order="F")
    return want


KERNEL_CASES = [(dt, rank, perm) for dt in TC.DTYPES for rank in (2, 3, 4) for perm in TC.permutations(rank)]


@pytest.mark.parametrize("dtype,rank,perm", KERNEL_CASES, ids=lambda v: "".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_permute_moves_every_window_bit_for_bit_and_nothing_else(dtype, rank, perm):
    k = TC.permutations(rank).index(perm)
    exts = TC.kernel_extents(rank, perm, 1000 * rank + k)
    item = np.dtype(dtype).itemsize
    src_off, dst_off, src_len, dst_len = TC.kernel_layout(exts, item, 0)
    rng = np.random.default_rng(77 + k)
    src = random_bits(rng, src_len, dtype)
    dst0 = np.frombuffer(bytes([CANARY_BYTE]) * (dst_len * item), dtype=dtype).copy()
    d_src, d_dst = gpu(src), gpu(dst0)
    assert d_dst.data_ptr() % 16 == 0
    rc = permute(dtype, perm, gpu(padded(exts)), gpu(src_off), gpu(dst_off), d_src, src_len, d_dst, dst_len)
    torch.cuda.synchronize()
    assert rc == 0
    want = expected_windows(dst0, src, exts, perm, src_off, dst_off)
    assert host(d_dst).tobytes() == want.tobytes()       # the windows equal numpy.transpose, the canaries between and around them are untouched
    assert host(d_src).tobytes() == src.tobytes()        # the source is unchanged


@pytest.mark.parametrize("dtype", TC.DTYPES)
def test_permute_on_a_written_side_that_is_not_16_byte_aligned(dtype):
    """a destination area that starts at an odd element: the 16-byte path must not be taken (no aligned pack store at an unaligned address)"""
    perm, exts = (1, 0, 2), [(23, 23, 23), (33, 2, 5), (3, 65, 2)]
    item = np.dtype(dtype).itemsize
    src_off, dst_off, src_len, dst_len = TC.kernel_layout(exts, item, 0)
    rng = np.random.default_rng(5)
    src = random_bits(rng, src_len, dtype)
    dst0 = np.frombuffer(bytes([CANARY_BYTE]) * ((dst_len + 1) * item), dtype=dtype).copy()
    d_src, d_all = gpu(src), gpu(dst0)
    d_dst = d_all[1:]
    rc = permute(dtype, perm, gpu(padded(exts)), gpu(src_off), gpu(dst_off), d_src, src_len, d_dst, dst_len)
    torch.cuda.synchronize()
    assert rc == 0
    want = expected_windows(dst0[1:], src, exts, perm, src_off, dst_off)
    assert host(d_all)[1:].tobytes() == want.tobytes() and host(d_all)[:1].tobytes() == dst0[:1].tobytes()


def test_permute_skips_windows_that_leave_their_area_and_bad_extents():
    dtype, perm = TC.F64, (2, 0, 1)
    exts = [(3, 5, 2), (4, 4, 4), (2, 3, 7), (5, 1, 3), (2, 2, 2), (3, 3, 3)]
    n = [int(np.prod(e)) for e in exts]
    src_len, dst_len = 400, 300
    #            fine   written window past dst_len   read window past src_len   fine   negative offset   fine
    src_off = np.array([1, 40, src_len - n[2] + 1, 150, 200, 230], np.int64)
    dst_off = np.array([2, dst_len - n[1] + 1, 60, 120, -1, 200], np.int64)
    ext = padded(exts)
    ext = np.concatenate([ext, [[3, 0, 2, 1]]]).astype(np.int32)   # an extent below 1: skipped as well
    src_off, dst_off = np.append(src_off, 300), np.append(dst_off, 250)
    rng = np.random.default_rng(9)
    src = random_bits(rng, src_len, dtype)
    dst0 = np.frombuffer(bytes([CANARY_BYTE]) * (dst_len * 8), dtype=dtype).copy()
    d_src, d_dst = gpu(src), gpu(dst0)
    rc = permute(dtype, perm, gpu(ext), gpu(src_off), gpu(dst_off), d_src, src_len, d_dst, dst_len)
    torch.cuda.synchronize()
    assert rc == 0
    keep = [0, 3, 5]
    want = expected_windows(dst0, src, [exts[b] for b in keep], perm, src_off[keep], dst_off[keep])
    assert host(d_dst).tobytes() == want.tobytes() and host(d_src).tobytes() == src.tobytes()


def test_permute_return_codes():
    dtype = TC.F64
    ext, off = gpu(padded([(2, 3)])), gpu(np.array([0], np.int64))
    src, dst = gpu(np.arange(6.0)), gpu(np.full(6, -1.0))
    ok = lambda **kw: permute(dtype, kw.pop("perm", (1, 0)), kw.pop("ext", ext), kw.pop("so", off), kw.pop("do", off), kw.pop("src", src), kw.pop("sl", 6),
                              kw.pop("dst", dst), kw.pop("dl", 6), **kw)
    assert ok(nblk=0) == 0
    torch.cuda.synchronize()
    assert host(dst).tolist() == [-1.0] * 6                     # nblk == 0: nothing moves
    assert ok(handle=False) == -1
    assert ok(ext=None) == -1 and ok(so=None) == -1 and ok(do=None) == -1 and ok(src=None) == -1 and ok(dst=None) == -1
    assert ok(perm=(0,), rank=1) == -1 and ok(perm=(0, 1, 2, 3, 4), rank=5) == -1
    assert ok(perm=(0, 0)) == -1 and ok(perm=(1, 2)) == -1 and ok(perm=(0, -1)) == -1 and ok(perm=(0, 1, 1), rank=3) == -1
    assert ok(nblk=-1) == -1 and ok(sl=-1) == -1
    both = gpu(np.arange(12.0))
    assert ok(src=both, sl=8, dst=both[6:], dl=6) == -1          # [src, src + len) overlaps [dst, dst + len)
    assert ok(src=both, sl=6, dst=both[6:], dl=6) == 0           # adjacent areas do not
    assert ok(code=5) == -10 and ok(code=9) == -10 and ok(code=0) == -10   # complex_4 and unknown type codes
    torch.cuda.synchronize()
    assert host(dst).tolist() == [-1.0] * 6
    assert ok() == 0
    torch.cuda.synchronize()
    assert host(dst).tolist() == np.arange(6.0).reshape((2, 3), order="F").T.reshape(-1, order="F").tolist()


@pytest.fixture(scope="module")
def arena():
    a = far_arena.arena()
    yield a
    if a is not None:
        a.release()


def test_permute_with_offsets_above_2_to_the_32_elements(arena):
    """float32: source and written offsets above 2^32 elements, in the two halves of one large allocation that is never filled"""
    if arena is None or arena.nbytes < far_arena.ARENA_LARGE:
        pytest.skip("the device has no room for the large arena")
    view = arena.view(np.float32)
    half = 2 ** 33
    assert view.numel() >= 2 * half
    src, dst = view[:half], view[half:2 * half]
    perm, exts = (2, 1, 0), [(23, 23, 23), (33, 2, 65), (1, 7, 3), (32, 32, 3)]
    n = [int(np.prod(e)) for e in exts]
    base_s, base_d = far_arena.TWO32 + 12345, far_arena.TWO32 + 2 ** 31 + 777
    src_off = np.array([base_s + 1, base_s + 20001, base_s + 40001, base_s + 60001], np.int64)
    dst_off = np.array([base_d, base_d + 20001, base_d + 40002, base_d + 60003], np.int64)
    rng = np.random.default_rng(3)
    guard = 64
    blocks = [random_bits(rng, k, np.float32) for k in n]
    for b, so in zip(blocks, src_off):
        src[int(so):int(so) + b.size].copy_(torch.from_numpy(b))
    for do, k in zip(dst_off, n):
        dst[int(do) - guard:int(do) + k + guard].fill_(far_arena.CANARY)
    # where a lost high word would write instead: the same places 2^32 elements lower
    low = [dst[int(do) - far_arena.TWO32:int(do) - far_arena.TWO32 + k] for do, k in zip(dst_off, n)]
    for w in low:
        w.fill_(far_arena.CANARY)
    rc = permute(TC.F32, perm, gpu(padded(exts)), gpu(src_off), gpu(dst_off), src, half, dst, half)
    torch.cuda.synchronize()
    assert rc == 0
    canary = np.float32(far_arena.CANARY)
    for b, e, so, do, k, w in zip(blocks, exts, src_off, dst_off, n, low):
        got = host(dst[int(do) - guard:int(do) + k + guard])
        want = np.transpose(b.reshape(e, order="F"), perm).reshape(-1, order="F")
        assert got[guard:guard + k].tobytes() == want.tobytes()
        assert np.all(got[:guard] == canary) and np.all(got[guard + k:] == canary)
        assert host(src[int(so):int(so) + k]).tobytes() == b.tobytes()
        assert np.all(host(w) == canary)


# ---- device tensors from host blocks ----------------------------------------------------------------------------------------------------------------------------------
def size_tensors(sizes):
    return [torch.as_tensor(np.asarray(s), dtype=torch.int32) for s in sizes]


def device_tensor(sizes, blocks, mapping, dtype):
    """a DbcsrTensor that stores the blocks, its matrix uploaded as the reference folds it"""
    rs, cs, row_p, col_i, blk_p, data, _ = TR.matrix_of(blocks, sizes, mapping[0], mapping[1], dtype)
    t = dbcsr_t_create(size_tensors(sizes), mapping[0], mapping[1], TORCH[dtype])
    assert np.array_equal(host(t.matrix.row_blk_size), rs) and np.array_equal(host(t.matrix.col_blk_size), cs)
    t.matrix.adopt(DbcsrMatrix.from_host(rs.astype(np.int32), cs.astype(np.int32), row_p, col_i, blk_p, data))
    return t


def matrix_equals(t, blocks, sizes, mapping, dtype, packed=True):
    rs, cs, row_p, col_i, blk_p, data, _ = TR.matrix_of(blocks, sizes, mapping[0], mapping[1], dtype)
    _, _, g_row_p, g_col_i, g_blk_p, g_data = t.matrix.to_host()
    assert np.array_equal(g_row_p, row_p) and np.array_equal(g_col_i, col_i)
    if packed:
        assert t.matrix.packed and np.array_equal(g_blk_p, blk_p) and g_data.tobytes() == data.tobytes()
    return True


def blocks_on_host(t, sizes):
    _, _, row_p, col_i, blk_p, data = t.matrix.to_host()
    return TR.blocks_of_matrix(row_p, col_i, blk_p, data, sizes, t.map1, t.map2)


@functools.lru_cache(maxsize=None)
def putget_case(rank, dtype):
    return TC.putget_tensor(rank, dtype)


def block_list(blocks, order):
    """(idx, flat data, offsets): the listed blocks one after another in canonical order"""
    flats = [TR.flat_canonical(blocks[ix]) for ix in order]
    sizes = np.array([f.size for f in flats], np.int64)
    return np.array(order, np.int32).reshape(len(order), -1), np.concatenate(flats) if flats else None, np.cumsum(sizes) - sizes


# ---- 2. put / get and the block indices -----------------------------------------------------------------------------------------------------------------------------------
PUTGET_CASES = [(rank, m, TC.F64) for rank in (2, 3, 4) for m in TC.MAPPINGS[rank]] + \
    [(rank, TC.MAPPINGS[rank][-1], dt) for rank in (2, 3, 4) for dt in (TC.F32, TC.Z64)]


@pytest.mark.parametrize("rank,mapping,dtype", PUTGET_CASES, ids=str)
def test_put_get_round_trip(rank, mapping, dtype):
    sizes, blocks = putget_case(rank, dtype)
    canonical = mapping[0] + mapping[1] == tuple(range(rank))
    rng = np.random.default_rng(31)
    order = [list(blocks)[k] for k in rng.permutation(len(blocks))]
    idx, data, _ = block_list(blocks, order)
    t = dbcsr_t_create(size_tensors(sizes), mapping[0], mapping[1], TORCH[dtype])
    T.reset_stats()
    dbcsr_t_put_blocks(t, gpu(idx), gpu(data))
    assert T.stats()["permute_launches"] == (0 if canonical else 1)
    assert T.stats()["permuted_elements"] == (0 if canonical else data.size)
    assert matrix_equals(t, blocks, sizes, mapping, dtype)
    want_order = TR.matrix_of(blocks, sizes, mapping[0], mapping[1], dtype)[6]
    got_idx = dbcsr_t_block_indices(t)
    assert got_idx.dtype == torch.int32 and got_idx.is_cuda and [tuple(r) for r in host(got_idx).tolist()] == want_order
    assert t.nblks == len(blocks) and t.rank == rank and t.dtype == TORCH[dtype] and t.nblks_per_dim == tuple(len(s) for s in sizes)
    # get: every stored block in another order, absent blocks among them, an index outside the tensor
    nb = [len(s) for s in sizes]
    absent = [ix for ix in np.ndindex(*nb) if ix not in blocks][:5]
    asked = [order[k] for k in rng.permutation(len(order))][:40] + absent
    asked = [asked[k] for k in rng.permutation(len(asked))]
    outside = tuple(nb[d] if d == rank - 1 else 0 for d in range(rank))
    T.reset_stats()
    got, found = dbcsr_t_get_blocks(t, gpu(np.array(asked + [outside], np.int32)))
    assert T.stats()["permute_launches"] == (0 if canonical else 1)
    got, found = host(got), host(found)
    at = 0
    for k, ix in enumerate(asked):
        n = int(np.prod(TR.extents(ix, sizes)))
        if ix in blocks:
            assert found[k] == 1 and got[at:at + n].tobytes() == TR.flat_canonical(blocks[ix]).tobytes()
        else:
            assert found[k] == 0 and got[at:at + n].tobytes() == np.zeros(n, dtype).tobytes()   # (+0.0)
        at += n
    assert found[-1] == 0 and at == got.size
    # summation: the same list once more doubles every block, exactly
    dbcsr_t_put_blocks(t, gpu(idx), gpu(data), summation=True)
    assert matrix_equals(t, {ix: b + b for ix, b in blocks.items()}, sizes, mapping, dtype)


def test_put_with_offsets_duplicates_and_windows_outside_data():
    sizes, blocks = putget_case(3, TC.F64)
    mapping = ((2, 0), (1,))
    some = list(blocks)[:6]
    idx, data, off = block_list(blocks, some)
    # the list backwards through offsets, the first block twice (the last of the list wins without summation), and one window that leaves data
    twice = TC.values(np.random.default_rng(1), blocks[some[0]].shape, TC.F64)
    flat = np.concatenate([data, TR.flat_canonical(twice)])
    idx2 = np.concatenate([idx[::-1], idx[:1], idx[1:2]])
    off2 = np.concatenate([off[::-1], [data.size], [flat.size - 3]])
    t = dbcsr_t_create(size_tensors(sizes), mapping[0], mapping[1], torch.float64)
    dbcsr_t_put_blocks(t, gpu(idx2), gpu(flat), offsets=gpu(off2))
    want = {ix: blocks[ix] for ix in some}
    want[some[0]] = twice
    assert matrix_equals(t, want, sizes, mapping, TC.F64)
    with pytest.raises(ValueError):
        dbcsr_t_put_blocks(t, gpu(np.array([[0, 0, len(sizes[2])]], np.int32)), gpu(np.zeros(4)))
    assert matrix_equals(t, want, sizes, mapping, TC.F64)
    t2 = dbcsr_t_create_from_blocks(size_tensors(sizes), mapping[0], mapping[1], gpu(idx2[:6]), gpu(flat), offsets=gpu(off2[:6]))
    assert matrix_equals(t2, {ix: blocks[ix] for ix in some}, sizes, mapping, TC.F64)
    # get into a given tensor at given offsets: a window that does not fit is treated as out of range
    out = gpu(np.full(flat.size, -3.0))
    got, found = dbcsr_t_get_blocks(t, gpu(idx2[:7]), out=out, offsets=gpu(np.append(off2[:6], flat.size - 3)))
    assert got is out and host(found).tolist() == [1] * 6 + [0]
    res = host(out)
    for ix, o in zip(some[::-1], off2[:6]):
        n = want[ix].size
        assert res[o:o + n].tobytes() == TR.flat_canonical(want[ix]).tobytes()
    assert np.all(res[data.size:] == -3.0)


def test_an_empty_tensor_and_a_dimension_with_one_block():
    sizes = [np.array([2, 3]), np.array([5]), np.array([1, 2, 3])]
    mapping = ((2, 0), (1,))
    t = dbcsr_t_create(size_tensors(sizes), mapping[0], mapping[1], torch.float64)
    assert t.nblks == 0 and dbcsr_t_block_indices(t).shape == (0, 3)
    dbcsr_t_put_blocks(t, gpu(np.zeros((0, 3), np.int32)), gpu(np.zeros(0)))
    got, found = dbcsr_t_get_blocks(t, gpu(np.array([[1, 0, 2], [0, 0, 0]], np.int32)))
    assert host(found).tolist() == [0, 0] and host(got).tobytes() == np.zeros(45 + 10).tobytes()
    empty2 = dbcsr_t_create(size_tensors(sizes), (0,), (1, 2), torch.float64)
    T.reset_stats()
    dbcsr_t_copy(t, empty2)
    assert empty2.nblks == 0 and T.stats()["permute_launches"] == 0
    rng = np.random.default_rng(2)
    blocks = {ix: TC.values(rng, TR.extents(ix, sizes), TC.F64) for ix in [(1, 0, 2), (0, 0, 1), (1, 0, 0)]}
    idx, data, _ = block_list(blocks, list(blocks))
    dbcsr_t_put_blocks(t, gpu(idx), gpu(data))
    assert matrix_equals(t, blocks, sizes, mapping, TC.F64)
    dbcsr_t_copy(t, empty2)
    assert matrix_equals(empty2, blocks, sizes, ((0,), (1, 2)), TC.F64)


# ---- 3. dbcsr_t_copy -----------------------------------------------------------------------------------------------------------------------------------------------------
def copy_cases():
    for rank in (2, 3, 4):
        for a, b in TC.COPY_PAIRS[rank]:
            for order in (None, TC.ORDERS[rank]):
                for summation in (False, True):
                    yield rank, a, b, order, summation, TC.F64
    for dt in (TC.F32, TC.Z64):
        yield 3, 0, 3, TC.ORDERS[3], False, dt
        yield 3, 4, 2, None, True, dt
        yield 4, 1, 2, TC.ORDERS[4], False, dt


@functools.lru_cache(maxsize=None)
def copy_source(rank, a, dtype):
    sizes, blocks = putget_case(rank, dtype)
    return device_tensor(sizes, blocks, TC.MAPPINGS[rank][a], dtype)


@functools.lru_cache(maxsize=None)
def copy_target_blocks(rank, order, dtype):
    """what tensor_out stores before a copy with summation: another pattern on the permuted sizes"""
    sizes, _ = putget_case(rank, dtype)
    out_sizes = [sizes[d] for d in order]
    rng = np.random.default_rng(500 + rank)
    blocks = {}
    for ix in np.ndindex(*[len(s) for s in out_sizes]):
        if rng.random() < 0.4:
            blocks[ix] = TC.values(rng, TR.extents(ix, out_sizes), dtype)
    return blocks


@pytest.mark.parametrize("rank,a,b,order,summation,dtype", list(copy_cases()), ids=str)
def test_copy_between_mappings(rank, a, b, order, summation, dtype):
    sizes, blocks = putget_case(rank, dtype)
    m_in, m_out = TC.MAPPINGS[rank][a], TC.MAPPINGS[rank][b]
    o = order or tuple(range(rank))
    out_sizes = [sizes[d] for d in o]
    t_in = copy_source(rank, a, dtype)
    before = [x.clone() for x in (t_in.matrix.row_p, t_in.matrix.col_i, t_in.matrix.blk_p, t_in.matrix.data)]
    moved = TR.permuted(blocks, o)
    if summation:
        old = copy_target_blocks(rank, o, dtype)
        t_out = device_tensor(out_sizes, old, m_out, dtype)
        want = dict(old)
        for ix, blk in moved.items():
            want[ix] = old[ix] + blk if ix in old else blk
    else:
        t_out = dbcsr_t_create(size_tensors(out_sizes), m_out[0], m_out[1], TORCH[dtype])
        want = moved
    same = tuple(o[j] for j in m_out[0]) == m_in[0] and tuple(o[j] for j in m_out[1]) == m_in[1]
    T.reset_stats()
    dbcsr_t_copy(t_in, t_out, order=order, summation=summation)
    assert T.stats()["permute_launches"] == (0 if same else 1)
    assert matrix_equals(t_out, want, out_sizes, m_out, dtype)    # blocks bit for bit, row_p / col_i the reference's, packed
    assert all(torch.equal(x, y) for x, y in zip(before, (t_in.matrix.row_p, t_in.matrix.col_i, t_in.matrix.blk_p, t_in.matrix.data)))
    assert t_out.matrix.data.data_ptr() != t_in.matrix.data.data_ptr()


# ---- 4. dbcsr_t_contract -----------------------------------------------------------------------------------------------------------------------------------------------------
def contract_cases():
    for name in sorted(TC.CONTRACTIONS):
        c = TC.CONTRACTIONS[name]
        dtypes = TC.DTYPES if name in TC.TYPED_CASES else (TC.F64,)
        for dtype in dtypes:
            for variant in ("compatible", "reversed", "foreign"):
                if c.operands[variant] is None:
                    continue
                for with_beta in (False, True):
                    yield name, dtype, variant, "foreign", with_beta, None, False
            for variant in ("compatible", "reversed"):
                yield name, dtype, variant, "compatible", True, None, False
        for name2 in ([name] if name in TC.FILTER_CASES else []):
            for dtype in dtypes:
                yield name2, dtype, "foreign", "foreign", False, TC.FILTER_EPS, False
                yield name2, dtype, "compatible", "compatible", False, TC.FILTER_EPS, False
        if name == "a":
            yield name, TC.F64, "foreign", "foreign", True, None, True
            yield name, TC.F64, "compatible", "compatible", True, None, True


@functools.lru_cache(maxsize=None)
def contract_reference(name, dtype, with_beta, eps, retain):
    alpha, beta = TC.SCALARS[dtype]
    return TC.reference(TC.CONTRACTIONS[name], dtype, alpha, beta if with_beta else 0.0, filter_eps=eps, retain_sparsity=retain)


def check_contraction(t3, s3, ref, dtype, flop):
    order = sorted(ref.blocks, key=lambda ix: TR.block_row_col(ix, [len(s) for s in s3], t3.map1, t3.map2))
    assert [tuple(r) for r in host(dbcsr_t_block_indices(t3)).tolist()] == order     # the index, exact
    assert flop == ref.flop
    gamma = gamma_of({"M": 1, "N": 1, "K": ref.n_inner_total, "limits": None, "dtype": dtype})
    got = blocks_on_host(t3, s3)
    worst = 0.0
    for ix in order:
        err, bar = np.abs(got[ix].astype(TR.wide(dtype)) - ref.blocks[ix]), gamma * ref.bound[ix]
        assert np.all(err <= bar), (ix, float(np.max(err - bar)))
        worst = max(worst, float(np.max(err / np.maximum(bar, np.finfo(np.float64).tiny))))
    print("worst error / bar = %.3g (gamma %.3g)" % (worst, gamma))


@pytest.mark.skipif(not LONG_DOUBLE_OK, reason="the reference needs an extended long double")
@pytest.mark.parametrize("name,dtype,variant,t3_kind,with_beta,eps,retain", list(contract_cases()), ids=str)
def test_contract_against_the_reference(name, dtype, variant, t3_kind, with_beta, eps, retain):
    c = TC.CONTRACTIONS[name]
    alpha, beta = TC.SCALARS[dtype]
    beta = beta if with_beta else 0.0
    (s1, B1), (s2, B2), (s3, B3) = c.tensors(dtype, small_free_2=eps is not None)
    map_1, map_2 = c.operands[variant]
    map_3 = c.t3_foreign if t3_kind == "foreign" else c.t3_compatible
    t1, t2, t3 = device_tensor(s1, B1, map_1, dtype), device_tensor(s2, B2, map_2, dtype), device_tensor(s3, B3, map_3, dtype)
    ref = contract_reference(name, dtype, with_beta, eps, retain)
    launches = TC.OPERAND_LAUNCHES.get((name, variant), 0) + (0 if t3_kind == "compatible" else (2 if (with_beta or retain) else 1))
    T.reset_stats()
    flop = dbcsr_t_contract(alpha, t1, t2, beta, t3, filter_eps=eps, retain_sparsity=retain, **TC.contract_args(c))
    assert T.stats()["permute_launches"] == launches
    assert (t3.map1, t3.map2) == map_3
    check_contraction(t3, s3, ref, dtype, flop)
    assert matrix_equals(t1, B1, s1, map_1, dtype) and matrix_equals(t2, B2, s2, map_2, dtype)   # the operands are as they were


def test_rank_2_contraction_is_dbcsr_multiply_bit_for_bit():
    c = TC.CONTRACTIONS["e"]
    alpha, beta = TC.SCALARS[TC.F64]
    (s1, B1), (s2, B2), (s3, B3) = c.tensors(TC.F64)
    straight = ((0,), (1,))
    t1, t2, t3 = (device_tensor(s, B, straight, TC.F64) for s, B in ((s1, B1), (s2, B2), (s3, B3)))
    m1, m2, m3 = (device_tensor(s, B, straight, TC.F64).matrix for s, B in ((s1, B1), (s2, B2), (s3, B3)))
    T.reset_stats()
    flop = dbcsr_t_contract(alpha, t1, t2, beta, t3, **TC.contract_args(c))
    assert T.stats()["permute_launches"] == 0
    counts = dbcsr_multiply("N", "N", alpha, m1, m2, beta, m3)
    assert flop == counts.flop
    for x, y in zip(t3.matrix.to_host()[2:], m3.to_host()[2:]):
        assert x.tobytes() == y.tobytes()
    # the reversed operands take "T" / "T": the same as dbcsr_multiply("T", "T") on the transposed matrices' stored forms
    r1, r2 = device_tensor(s1, B1, ((1,), (0,)), TC.F64), device_tensor(s2, B2, ((1,), (0,)), TC.F64)
    t3b, m3b = device_tensor(s3, B3, straight, TC.F64), device_tensor(s3, B3, straight, TC.F64).matrix
    flop = dbcsr_t_contract(alpha, r1, r2, beta, t3b, **TC.contract_args(c))
    assert T.stats()["permute_launches"] == 0
    counts = dbcsr_multiply("T", "T", alpha, r1.matrix, r2.matrix, beta, m3b)
    assert flop == counts.flop
    for x, y in zip(t3b.matrix.to_host()[2:], m3b.to_host()[2:]):
        assert x.tobytes() == y.tobytes()


@pytest.mark.skipif(not LONG_DOUBLE_OK, reason="the reference needs an extended long double")
def test_contract_on_a_side_stream_gives_the_same_bits():
    c = TC.CONTRACTIONS["a"]
    alpha, beta = TC.SCALARS[TC.F64]
    (s1, B1), (s2, B2), (s3, B3) = c.tensors(TC.F64)
    f1, f2 = c.operands["foreign"]
    make = lambda: (device_tensor(s1, B1, f1, TC.F64), device_tensor(s2, B2, f2, TC.F64), device_tensor(s3, B3, c.t3_foreign, TC.F64))
    t1, t2, t3 = make()
    flop = dbcsr_t_contract(alpha, t1, t2, beta, t3, **TC.contract_args(c))
    u1, u2, u3 = make()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    assert dbcsr_t_contract(alpha, u1, u2, beta, u3, stream=side, **TC.contract_args(c)) == flop
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    for x, y in zip(t3.matrix.to_host()[2:], u3.matrix.to_host()[2:]):
        assert x.tobytes() == y.tobytes()
    check_contraction(u3, s3, contract_reference("a", TC.F64, True, None, False), TC.F64, flop)


# ---- 5. interplay ----------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not LONG_DOUBLE_OK, reason="the reference needs an extended long double")
def test_the_matrix_interface_on_a_contracted_tensor():
    c = TC.CONTRACTIONS["a"]
    alpha, beta = TC.SCALARS[TC.F64]
    (s1, B1), (s2, B2), (s3, B3) = c.tensors(TC.F64)
    t1, t2 = device_tensor(s1, B1, c.operands["foreign"][0], TC.F64), device_tensor(s2, B2, c.operands["foreign"][1], TC.F64)
    t3 = device_tensor(s3, B3, c.t3_foreign, TC.F64)
    dbcsr_t_contract(alpha, t1, t2, beta, t3, **TC.contract_args(c))
    ref = contract_reference("a", TC.F64, True, None, False)
    R = np.concatenate([b.reshape(-1) for b in ref.blocks.values()])
    bound = np.concatenate([b.reshape(-1) for b in ref.bound.values()])
    gamma = gamma_of({"M": 1, "N": 1, "K": ref.n_inner_total, "limits": None, "dtype": TC.F64})
    want = float(np.sqrt((np.abs(R) ** 2).sum()))
    # the elements are within gamma bound of R (the bar above), so the norm is within gamma ||bound||; the norm's own sum of N squares and its root
    # add (N + 2) u of it (Higham, section 3.1, as in tests/option_sweep.py)
    tol = gamma * float(np.sqrt((bound ** 2).sum())) + (R.size + 2) * 2.0 ** -53 * want
    assert abs(dbcsr_frobenius_norm(t3.matrix) - want) <= tol
    data = host(t3.matrix.data).copy()
    dbcsr_scale(t3.matrix, 2.0)
    assert host(t3.matrix.data).tobytes() == (2.0 * data).tobytes()
    nb = t3.nblks
    dbcsr_t_filter(t3, 1e-100)
    assert t3.nblks == nb
    dbcsr_t_filter(t3, 1e100)
    assert t3.nblks == 0


def test_a_symmetric_matrix_into_a_tensor_and_back():
    rng = np.random.default_rng(8)
    bs = np.array([3, 1, 23, 5, 2], np.int32)
    nb = len(bs)
    row_p, col_i, flats = [0], [], []
    for r in range(nb):
        for cc in range(r, nb):
            if cc == r or rng.random() < 0.5:
                blk = TC.values(rng, (bs[r], bs[cc]), TC.F64)
                if cc == r:
                    blk = blk + blk.T
                col_i.append(cc)
                flats.append(blk.reshape(-1, order="F"))
        row_p.append(len(col_i))
    sizes = np.array([f.size for f in flats], np.int64)
    S = DbcsrMatrix.from_host(bs, bs, np.array(row_p, np.int32), np.array(col_i, np.int32), np.cumsum(sizes) - sizes, np.concatenate(flats))
    S.symmetry = "S"
    dense = host(dbcsr_to_dense(S))
    assert np.array_equal(dense, dense.T) and np.count_nonzero(dense) > np.count_nonzero(np.triu(dense))
    for mapping in (((0,), (1,)), ((1,), (0,))):
        t = dbcsr_t_create(size_tensors([bs, bs]), mapping[0], mapping[1], torch.float64)
        T.reset_stats()
        dbcsr_t_copy_matrix_to_tensor(S, t)
        assert T.stats()["permute_launches"] == (0 if mapping == ((0,), (1,)) else 1)
        assert S.symmetry == "S"
        full = blocks_on_host(t, [bs, bs])
        assert TR.dense_of(full, [bs, bs], np.float64).tobytes() == dense.tobytes()
        back = DbcsrMatrix.empty_like_pattern(gpu(bs), gpu(bs), torch.float64)
        back.symmetry = "S"
        dbcsr_t_copy_tensor_to_matrix(t, back)
        assert back.symmetry == "N" and back.nblks == t.nblks
        assert host(dbcsr_to_dense(back)).tobytes() == dense.tobytes()
