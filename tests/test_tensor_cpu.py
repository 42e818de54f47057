"""The block-sparse tensor interface without a GPU: the index work of dbcsr_amd/tensor.py on host tensors against tests/tensor_ref.py, its ValueErrors,
the glue of dbcsr_t_copy with a numpy stand-in for the permute launch (the C entry's convention, include/dbcsr_amd_mm.h "Tensors"), the foldings
dbcsr_t_contract chooses, and the conditions the inputs of tests/test_gpu_tensor.py must meet (tests/tensor_cases.py)."""
import itertools

import numpy as np
import pytest
import torch

import dbcsr_amd.tensor as T
from tests import tensor_cases as TC
from tests import tensor_ref as TR
from tests.option_sweep import LONG_DOUBLE_OK

ALL_MAPPINGS = [(r, m) for r in (2, 3, 4) for m in TC.MAPPINGS[r]]
TORCH_DTYPE = {TC.F64: torch.float64, TC.F32: torch.float32, TC.Z64: torch.complex128}


def small_tensor(rank, seed, dtype=TC.F64):
    return TC.random_tensor(seed, rank, dtype, pool=(1, 2, 3, 5), nb_range=(2, 4))


def host_tensor(sizes, blocks, mapping, dtype=TC.F64):
    """a DbcsrTensor of host tensors that stores the blocks, built from the reference's matrix"""
    rs, cs, row_p, col_i, blk_p, data, _ = TR.matrix_of(blocks, sizes, mapping[0], mapping[1], dtype)
    t = T.dbcsr_t_create([torch.as_tensor(s, dtype=torch.int32) for s in sizes], mapping[0], mapping[1], TORCH_DTYPE[dtype], device="cpu")
    assert np.array_equal(t.matrix.row_blk_size.numpy(), rs) and np.array_equal(t.matrix.col_blk_size.numpy(), cs)
    t.matrix.row_p, t.matrix.col_i, t.matrix.blk_p = torch.as_tensor(row_p), torch.as_tensor(col_i), torch.as_tensor(blk_p)
    t.matrix.data = torch.as_tensor(data)
    return t


def numpy_permute(E, stream, dtype, perm, ext, src_off, dst_off, src, dst, elements):
    """dbcsr_amd_tensor_permute_blocks as the header states it: dimension j of the written array is dimension perm[j] of the read one"""
    s, d = src.numpy(), dst.numpy()
    rank = len(perm)
    for b in range(ext.shape[0]):
        e = [int(x) for x in ext[b][:rank]]
        assert all(int(x) == 1 for x in ext[b][rank:])
        n, so, do = int(np.prod(e)), int(src_off[b]), int(dst_off[b])
        assert 0 <= so and so + n <= s.size and 0 <= do and do + n <= d.size
        d[do:do + n] = np.transpose(s[so:so + n].reshape(e, order="F"), perm).reshape(-1, order="F")
    T._STATS["permute_launches"] += 1


# ---- the index functions ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rank,mapping", ALL_MAPPINGS)
def test_combined_indices_are_a_bijection_and_sizes_are_products(rank, mapping):
    sizes, _ = small_tensor(rank, 7 + rank)
    nb = [len(s) for s in sizes]
    every = torch.as_tensor(list(itertools.product(*[range(n) for n in nb])), dtype=torch.int32)
    rows, cols = T.combine_index(every, nb, mapping[0]), T.combine_index(every, nb, mapping[1])
    nbr, nbc = int(np.prod([nb[d] for d in mapping[0]])), int(np.prod([nb[d] for d in mapping[1]]))
    assert sorted((rows * nbc + cols).tolist()) == list(range(nbr * nbc))
    for k, ix in enumerate(every.tolist()):
        assert (int(rows[k]), int(cols[k])) == TR.block_row_col(ix, nb, mapping[0], mapping[1])
    back = T.split_index(rows, nb, mapping[0])
    back.update(T.split_index(cols, nb, mapping[1]))
    assert all(torch.equal(back[d], every[:, d].long()) for d in range(rank))
    tsizes = [torch.as_tensor(s, dtype=torch.int32) for s in sizes]
    assert np.array_equal(T.fold_sizes(tsizes, mapping[0]).numpy(), TR.folded_sizes(sizes, mapping[0]))
    assert np.array_equal(T.fold_sizes(tsizes, mapping[1]).numpy(), TR.folded_sizes(sizes, mapping[1]))
    R, Cc = int(rows[-1]), int(cols[-1])
    assert int(T.fold_sizes(tsizes, mapping[0])[R]) * int(T.fold_sizes(tsizes, mapping[1])[Cc]) == int(np.prod(TR.extents(every[-1].tolist(), sizes)))


@pytest.mark.parametrize("rank,mapping", ALL_MAPPINGS)
def test_fold_and_unfold_equal_the_reference(rank, mapping):
    sizes, blocks = small_tensor(rank, 11 + rank)
    rs, cs, row_p, col_i, blk_p, data, order = TR.matrix_of(blocks, sizes, mapping[0], mapping[1], TC.F64)
    rng = np.random.default_rng(3)
    listed = [list(blocks)[k] for k in rng.permutation(len(blocks))]
    idx = torch.as_tensor(listed, dtype=torch.int32)
    tsizes = [torch.as_tensor(s, dtype=torch.int32) for s in sizes]
    by, t_row_p, t_col_i, t_blk_p, nze = T.fold_index(idx, tsizes, mapping[0], mapping[1])
    assert t_row_p.dtype == torch.int32 and t_col_i.dtype == torch.int32 and t_blk_p.dtype == torch.int64
    assert np.array_equal(t_row_p.numpy(), row_p) and np.array_equal(t_col_i.numpy(), col_i) and np.array_equal(t_blk_p.numpy(), blk_p)
    assert int(nze) == data.size
    assert [tuple(listed[k]) for k in by.tolist()] == order
    got = T.unfold_index(t_row_p, t_col_i, [len(s) for s in sizes], mapping[0], mapping[1])
    assert [tuple(r) for r in got.tolist()] == order
    assert TR.blocks_of_matrix(row_p, col_i, blk_p, data, sizes, mapping[0], mapping[1]).keys() == blocks.keys()


def test_an_empty_tensor_and_a_dimension_with_one_block():
    t = T.dbcsr_t_create([[2, 3], [5], [1, 2, 3]], (2, 0), (1,), torch.float64, device="cpu")
    assert t.nblks == 0 and t.rank == 3 and t.nblks_per_dim == (2, 1, 3) and t.dtype == torch.float64
    assert T.dbcsr_t_block_indices(t).shape == (0, 3)
    assert t.matrix.nblkrows == 6 and t.matrix.nblkcols == 1
    by, row_p, col_i, blk_p, nze = T.fold_index(torch.zeros((0, 3), dtype=torch.int32), t.blk_sizes, t.map1, t.map2)
    assert row_p.tolist() == [0] * 7 and col_i.numel() == 0 and int(nze) == 0


# ---- dbcsr_t_copy's glue, with numpy in the kernel's place ----------------------------------------------------------------------------------------------------------
def copy_cases():
    for rank in (2, 3, 4):
        for a, b in TC.COPY_PAIRS[rank]:
            for order in (None, TC.ORDERS[rank]):
                yield rank, a, b, order


@pytest.mark.parametrize("rank,a,b,order", list(copy_cases()))
def test_copy_remaps_index_and_blocks_exactly(monkeypatch, rank, a, b, order):
    monkeypatch.setattr(T, "_permute", numpy_permute)
    sizes, blocks = small_tensor(rank, 20 + rank)
    m_in, m_out = TC.MAPPINGS[rank][a], TC.MAPPINGS[rank][b]
    o = order or tuple(range(rank))
    t_in = host_tensor(sizes, blocks, m_in)
    before = [x.clone() for x in (t_in.matrix.row_p, t_in.matrix.col_i, t_in.matrix.blk_p, t_in.matrix.data)]
    out_sizes = [sizes[d] for d in o]
    t_out = T.dbcsr_t_create(out_sizes, m_out[0], m_out[1], torch.float64, device="cpu")
    T.reset_stats()
    same = tuple(o[j] for j in m_out[0]) == m_in[0] and tuple(o[j] for j in m_out[1]) == m_in[1]
    T.dbcsr_t_copy(t_in, t_out, order=order, engine=object())
    assert T.stats()["permute_launches"] == (0 if same else 1)
    rs, cs, row_p, col_i, blk_p, data, _ = TR.matrix_of(TR.permuted(blocks, o), out_sizes, m_out[0], m_out[1], TC.F64)
    M = t_out.matrix
    assert np.array_equal(M.row_p.numpy(), row_p) and np.array_equal(M.col_i.numpy(), col_i) and np.array_equal(M.blk_p.numpy(), blk_p)
    assert M.data.numpy().tobytes() == data.tobytes() and M.packed
    assert all(torch.equal(x, y) for x, y in zip(before, (t_in.matrix.row_p, t_in.matrix.col_i, t_in.matrix.blk_p, t_in.matrix.data)))


# ---- errors, all without a device -------------------------------------------------------------------------------------------------------------------------------------
def test_create_refuses_what_is_no_tensor_of_this_library():
    s = [2, 3]
    for sizes, m1, m2 in (([s], (0,), ()), ([s] * 5, (0, 1), (2, 3, 4)), ([s] * 3, (0,), (1,)), ([s] * 3, (0, 1), (1, 2)), ([s] * 3, (), (0, 1, 2)),
                          ([s] * 2, (0,), (2,)), ([s, [0, 1]], (0,), (1,))):
        with pytest.raises(ValueError):
            T.dbcsr_t_create(sizes, m1, m2, torch.float64, device="cpu")
    with pytest.raises(TypeError):
        T.dbcsr_t_create([s, s], (0,), (1,), torch.complex64, device="cpu")
    with pytest.raises(TypeError):
        T.dbcsr_t_create([s, s], (0,), (1,), torch.float16, device="cpu")


def test_create_refuses_folded_sizes_beyond_int32_before_it_allocates():
    many = np.ones(50000, np.int64)
    with pytest.raises(ValueError, match="block rows"):
        T.dbcsr_t_create([many, many, [1]], (0, 1), (2,), torch.float64, device="cpu")
    with pytest.raises(ValueError, match="block columns"):
        T.dbcsr_t_create([[1], many, many], (0,), (2, 1), torch.float64, device="cpu")
    with pytest.raises(ValueError, match="block size"):
        T.dbcsr_t_create([[70000], [70000], [1]], (1, 0), (2,), torch.float64, device="cpu")
    with pytest.raises(ValueError, match="block size"):
        T.dbcsr_t_create([[1], [70000, 2], [3, 70000]], (0,), (1, 2), torch.float64, device="cpu")
    ok = T.dbcsr_t_create([[46340], [46340], [1]], (1, 0), (2,), torch.float64, device="cpu")   # 46340^2 < 2^31
    assert int(ok.matrix.row_blk_size[0]) == 46340 ** 2


def test_copy_refuses_before_any_device_work():
    a = T.dbcsr_t_create([[2, 3], [5, 1], [4]], (0,), (1, 2), torch.float64, device="cpu")
    with pytest.raises(ValueError):   # sizes do not agree under the identity
        T.dbcsr_t_copy(a, T.dbcsr_t_create([[5, 1], [2, 3], [4]], (0,), (1, 2), torch.float64, device="cpu"))
    with pytest.raises(ValueError):   # nor under this order
        T.dbcsr_t_copy(a, T.dbcsr_t_create([[5, 1], [2, 3], [4]], (0,), (1, 2), torch.float64, device="cpu"), order=(2, 0, 1))
    with pytest.raises(ValueError):
        T.dbcsr_t_copy(a, T.dbcsr_t_create([[2, 3], [5, 1], [4]], (0,), (1, 2), torch.float64, device="cpu"), order=(0, 0, 1))
    with pytest.raises(ValueError):
        T.dbcsr_t_copy(a, T.dbcsr_t_create([[2, 3], [5, 1]], (0,), (1,), torch.float64, device="cpu"))
    with pytest.raises(TypeError):
        T.dbcsr_t_copy(a, T.dbcsr_t_create([[2, 3], [5, 1], [4]], (0,), (1, 2), torch.float32, device="cpu"))
    with pytest.raises(ValueError):
        T.dbcsr_t_copy(a, a)


def test_contract_refuses_inconsistent_tuples_and_sizes_before_any_device_work():
    mk = lambda sizes, m1, m2, dt=torch.float64: T.dbcsr_t_create(sizes, m1, m2, dt, device="cpu")
    i, j, k, l = [2, 3], [5, 1, 2], [4, 4], [3]
    t1, t2, t3 = mk([i, j, k], (0, 1), (2,)), mk([k, l], (0,), (1,)), mk([i, j, l], (0, 1), (2,))
    good = dict(contract_1=(2,), notcontract_1=(0, 1), contract_2=(0,), notcontract_2=(1,), map_1=(0, 1), map_2=(2,))
    for change in (dict(contract_1=(1,)), dict(notcontract_1=(0,)), dict(contract_2=(0, 1)), dict(notcontract_2=(0,)), dict(map_1=(0,)), dict(map_2=(1,)),
                   dict(contract_1=(), notcontract_1=(0, 1, 2)), dict(map_1=(0, 1, 2), map_2=()), dict(contract_1=(3,))):
        with pytest.raises(ValueError):
            T.dbcsr_t_contract(1.0, t1, t2, 0.0, t3, **dict(good, **change))
    with pytest.raises(ValueError):   # contracted sizes differ
        T.dbcsr_t_contract(1.0, t1, mk([[4, 3], l], (0,), (1,)), 0.0, t3, **good)
    with pytest.raises(ValueError):   # free sizes differ
        T.dbcsr_t_contract(1.0, t1, t2, 0.0, mk([i, [5, 1, 3], l], (0, 1), (2,)), **good)
    with pytest.raises(ValueError):   # paired the wrong way round
        T.dbcsr_t_contract(1.0, t1, t2, 0.0, t3, **dict(good, map_1=(1, 0)))
    with pytest.raises(TypeError):
        T.dbcsr_t_contract(1.0, t1, t2, 0.0, mk([i, j, l], (0, 1), (2,), torch.float32), **good)


# ---- the foldings a contraction chooses ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(TC.CONTRACTIONS))
def test_plan_contract_uses_what_fits_as_it_is(name):
    c = TC.CONTRACTIONS[name]
    args = (c.ranks[0], c.ranks[1], c.ranks[2])
    tup = (c.c1, c.n1, c.c2, c.n2, c.m1, c.m2)
    m1c, m2c = c.operands["compatible"]
    need = T.plan_contract(*args, m1c, m2c, c.t3_compatible, *tup)
    assert need == (m1c, m2c, c.t3_compatible), need          # all three used as they are
    m1r, m2r = c.operands["reversed"]
    need = T.plan_contract(*args, m1r, m2r, c.t3_compatible, *tup)
    assert need == ((m1r[1], m1r[0]), (m2r[1], m2r[0]), c.t3_compatible), need   # exactly the reversed pairs: "T", no remap
    for maps_1, maps_2, maps_3 in ((m1c, m2c, c.t3_foreign), (m1r, m2r, c.t3_foreign)) + (((c.operands["foreign"]) + (c.t3_foreign,),) if c.operands["foreign"] else ()):
        (n1, c1), (c2, n2), (m1, m2) = T.plan_contract(*args, maps_1, maps_2, maps_3, *tup)
        assert sorted(n1) == sorted(c.n1) and sorted(c1) == sorted(c.c1) and sorted(c2) == sorted(c.c2) and sorted(n2) == sorted(c.n2)
        pair_c, pair_1, pair_2 = dict(zip(c.c1, c.c2)), dict(zip(c.n1, c.m1)), dict(zip(c.n2, c.m2))
        assert tuple(pair_c[d] for d in c1) == c2 and tuple(pair_1[d] for d in n1) == m1 and tuple(pair_2[d] for d in n2) == m2
    if c.operands["foreign"]:
        f1, f2 = c.operands["foreign"]
        (n1, c1), (c2, n2), _ = T.plan_contract(*args, f1, f2, c.t3_foreign, *tup)
        remaps = sum(1 for have, need in ((f1, (n1, c1)), (f2, (c2, n2))) if have != need and have != (need[1], need[0]))
        assert remaps == TC.OPERAND_LAUNCHES[(name, "foreign")]
    # tensor_1 (x | contract) with the contracted dimensions in another order: tensor_2 follows it
    if len(c.c1) == 2:
        (n1, c1), (c2, n2), _ = T.plan_contract(*args, (c.n1, c.c1[::-1]), (c.c2, c.n2), c.t3_compatible, *tup)
        assert c1 == c.c1[::-1] and c2 == c.c2[::-1]


# ---- the conditions on the inputs of the GPU tests ----------------------------------------------------------------------------------------------------------------------
def test_every_permutation_and_every_listed_mapping_is_reached():
    assert [len(TC.permutations(r)) for r in (2, 3, 4)] == [2, 6, 24]
    assert TC.MAPPINGS[2] == [((0,), (1,)), ((1,), (0,))]
    assert TC.MAPPINGS[3] == [((0,), (1, 2)), ((0, 1), (2,)), ((1,), (2, 0)), ((2, 0), (1,)), ((2, 1), (0,))]
    assert TC.MAPPINGS[4] == [((0, 1), (2, 3)), ((3, 1), (0, 2)), ((2,), (3, 0, 1))]
    assert len(TC.COPY_PAIRS[3]) == 25 and len(TC.COPY_PAIRS[4]) == 4 and len(TC.COPY_PAIRS[2]) == 4
    for rank in (2, 3, 4):
        T.check_order("test", rank, TC.ORDERS[rank])
        assert TC.ORDERS[rank] != tuple(range(rank))
        reached = {m for pair in TC.COPY_PAIRS[rank] for m in pair}
        assert reached == set(range(len(TC.MAPPINGS[rank])))


@pytest.mark.parametrize("rank", (2, 3, 4))
def test_kernel_launches_hold_every_extent_class_on_both_fast_sides(rank):
    for k, perm in enumerate(TC.permutations(rank)):
        exts = TC.kernel_extents(rank, perm, 1000 * rank + k)
        assert all(len(e) == rank and set(e) <= set(TC.EXTENT_POOL) | {5} and int(np.prod(e)) <= TC.KERNEL_MAX_BLOCK for e in exts)
        assert tuple([23] * min(rank, 3) + [1] * (rank - min(rank, 3))) in exts
        for pos in range(rank):
            assert any(e[pos] == 1 and all(x > 1 for j, x in enumerate(e) if j != pos) for e in exts)
        assert {e[0] for e in exts} >= set(TC.EXTENT_CLASSES), "source-fastest"
        assert {e[perm[0]] for e in exts} >= set(TC.EXTENT_CLASSES), "written-fastest"
        assert len({e for e in exts}) > 3
        for itemsize in (4, 8, 16):
            so, do, sl, dl = TC.kernel_layout(exts, itemsize, 0)
            assert np.all(so % 2 == 1)
            V = 16 // itemsize
            assert {int(x) % V for x in do} == set(range(V))
            n = np.array([int(np.prod(e)) for e in exts])
            assert np.all(so[1:] >= so[:-1] + n[:-1] + 2) and np.all(do[1:] >= do[:-1] + n[:-1] + 2) and so[0] >= 8 and do[0] >= 8
            assert so[-1] + n[-1] + 8 <= sl and do[-1] + n[-1] + 8 <= dl


@pytest.mark.parametrize("rank", (2, 3, 4))
def test_putget_tensors_are_as_the_issue_sets_them(rank):
    sizes, blocks = TC.putget_tensor(rank, TC.F64)
    assert all(3 <= len(s) <= 5 and set(s.tolist()) <= set(TC.SIZE_POOL) for s in sizes)
    total = int(np.prod([len(s) for s in sizes]))
    assert 0.3 * total <= len(blocks) <= 0.7 * total
    assert 0 < TC.elements(blocks) <= TC.MAX_ELEMENTS
    assert len(blocks) < total   # (absent blocks exist for the get test)


@pytest.mark.skipif(not LONG_DOUBLE_OK, reason="the reference needs an extended long double")
@pytest.mark.parametrize("name", sorted(TC.CONTRACTIONS))
def test_contraction_inputs_and_the_two_references_agree(name):
    c = TC.CONTRACTIONS[name]
    alpha, beta = TC.SCALARS[TC.F64]
    (s1, B1), (s2, B2), (s3, B3) = c.tensors(TC.F64)
    P = TR.contract_pattern(TR.pattern_of(B1, s1), TR.pattern_of(B2, s2), c.c1, c.n1, c.c2, c.n2, c.m1, c.m2)
    assert P.any() and not P.all()
    assert any(not P[ix] for ix in B3), "tensor_3 must store blocks outside the product's pattern"
    assert any(P[ix] for ix in B3) and any(tuple(ix) not in B3 for ix in np.argwhere(P))
    ref0 = TC.reference(c, TC.F64, alpha, 0.0)
    assert set(ref0.blocks) == {tuple(ix) for ix in np.argwhere(P)}
    ref = TC.reference(c, TC.F64, alpha, beta)
    assert set(ref.blocks) == {tuple(ix) for ix in np.argwhere(P)} | set(B3)
    assert ref.flop == ref0.flop > 0
    R, bound = TR.contract_dense(alpha, TR.dense_of(B1, s1, TC.F64), TR.dense_of(B2, s2, TC.F64), beta, TR.dense_of(B3, s3, TC.F64), c.c1, c.n1, c.c2,
                                 c.n2, c.m1, c.m2)
    D = TR.dense_of(ref.blocks, s3, TR.LD)
    Bd = TR.dense_of(ref.bound, s3, TR.LD)
    assert np.all(np.abs(D - R) <= 2.0 ** -58 * bound) and np.all(np.abs(Bd - bound) <= 2.0 ** -58 * bound)
    kept = TC.reference(c, TC.F64, alpha, beta, retain_sparsity=True)
    assert set(kept.blocks) == set(B3) and 0 < kept.flop < ref.flop


@pytest.mark.parametrize("dtype", TC.DTYPES)
@pytest.mark.parametrize("name", TC.FILTER_CASES)
def test_filtered_cases_stay_clear_of_their_thresholds(name, dtype):
    c = TC.CONTRACTIONS[name]
    alpha, _ = TC.SCALARS[dtype]
    ref = TC.reference(c, dtype, alpha, 0.0, filter_eps=TC.FILTER_EPS)
    assert ref.product_margins and all(m < 1.0 / 16 or m > 16 for m in ref.product_margins), sorted(ref.product_margins)[:5]   # (squares: a factor 4)
    assert ref.block_margins and all(m < 0.25 or m > 4 for m in ref.block_margins)
    dropped = ref.unfiltered - set(ref.blocks)
    assert dropped and ref.blocks, "at least one block dropped and one kept"
    assert any(m < 1 for m in ref.product_margins) and any(m > 1 for m in ref.product_margins)
