"""The submatrix method on the device (dbcsr_amd/submatrix.py: dbcsr_submatrix_plan, dbcsr_submatrix_gather, dbcsr_submatrix_scatter, dbcsr_submatrix_apply; the
"Submatrix method" entries of include/dbcsr_amd_mm.h; kernels of dbcsr_amd/csrc/mm_submatrix.h) for float64, float32 and complex128.

Everything is a copy, so everything is compared BIT FOR BIT with the numpy restatement of tests/submatrix_ref.py (checked without a GPU by
tests/test_submatrix_cpu.py).  No tolerance anywhere but in the inverse workflow, whose bar is stated in submatrix_ref.inverse_bar.

Matrices: 9 x 9 blocks with the sizes 5 13 1 23 32 33 40 64 1 (see tests/submatrix_ref.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

from dbcsr_amd import lib as L
from dbcsr_amd.matrix import DbcsrMatrix, StreamHandle
from dbcsr_amd.multiply import MultiplyEngine, dbcsr_multiply
from dbcsr_amd.operations import dbcsr_to_dense
from dbcsr_amd.submatrix import dbcsr_submatrix_apply, dbcsr_submatrix_gather, dbcsr_submatrix_plan, dbcsr_submatrix_scatter
from tests import submatrix_ref as R
from tests import test_gpu_dense as GD
from tests.gpu_util import dev_to_bcsr, to_dev
from tests.test_gpu_matrix_norms import TORCH, blocks_of, dense, from_blocks, from_dense, is_complex, misaligned, same_bits, subset, with_holes

pytestmark = pytest.mark.gpu

DTYPES, IDS = GD.DTYPES, GD.IDS
host, nan_of = GD.host, GD.nan_of


@pytest.fixture(scope="module")
def eng():
    return MultiplyEngine()


def dev(M, symmetry="N"):
    dM = to_dev(M)
    dM.symmetry = symmetry
    return dM


def plan_matches(plan, M, groups, symmetry):
    """the device's plan is the brute-force one; returns (sets, owner)"""
    sets, owner = R.brute_sets(M, groups, symmetry)
    for name, want in zip(("set_ptr", "set_idx", "set_off", "sub_dim"), R.plan_arrays(sets, M.row_sizes)):
        got = getattr(plan, name)
        assert got.is_cuda and same_bits(host(got), want), name
    assert same_bits(host(plan.owner), np.asarray(owner, np.int32))
    assert (plan.nsub, plan.max_members, plan.max_dim) == (len(sets), max(map(len, sets), default=0), int(max(plan.sub_dim_host, default=0)))
    return sets, owner


def random_batch(rng, shape, dtype):
    return GD.random_values(rng, int(np.prod(shape)), dtype).reshape(shape)


# ---- 1. the full set is dbcsr_to_dense ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_full_set_is_to_dense(eng, dtype):
    name = np.dtype(dtype).name
    cases = [("N", R.general(name))] + [(s, T) for s in R.SYMMETRIES[name] for T in (R.triangle(name), R.triangle(name, below=True))]
    for symmetry, M in cases:
        dM = dev(M, symmetry)
        plan = dbcsr_submatrix_plan(dM, [0] * R.NB)
        assert (plan.nsub, plan.max_members, plan.max_dim) == (1, R.NB, int(R.SQUARE.sum()))
        got = host(dbcsr_submatrix_gather(dM, plan, engine=eng))
        ref = R.full_dense(M, symmetry)
        assert got.shape == (1,) + ref.shape and same_bits(got[0], host(dbcsr_to_dense(dM, engine=eng))), symmetry
        assert same_bits(got[0], ref), symmetry
        if symmetry == "A":
            assert np.any((ref == 0) & np.signbit(ref)) and np.any((ref == 0) & ~np.signbit(ref)), "the -0.0 twin of +0.0 is there"
        assert same_bits(host(dM.data), M.data)
    assert any(r > c for r, c in blocks_of(cases[-1][1])) and any(r < c for r, c in blocks_of(cases[-1][1]))


# ---- 2. every window of the default and of a grouped plan ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_every_window_against_numpy(eng, dtype):
    name = np.dtype(dtype).name
    for symmetry, M in [("N", R.general(name)), (R.SYMMETRIES[name][1], R.triangle(name, below=True))]:
        dM = dev(M, symmetry)
        stamp = dM.index_stamp()
        for groups in (None, R.GROUPED):
            plan = dbcsr_submatrix_plan(dM, groups)
            sets, owner = plan_matches(plan, M, groups, symmetry)
            got = dbcsr_submatrix_gather(dM, plan, engine=eng)
            assert tuple(got.shape) == (plan.nsub, plan.max_dim, plan.max_dim) and got.is_contiguous() and got.dtype == TORCH[np.dtype(dtype)]
            assert same_bits(host(got), R.gathered(M, symmetry, sets, None, plan.max_dim, 0.0)), (symmetry, groups)
            if symmetry == "N":
                stored = set(blocks_of(M))
                assert any((a, b) not in stored for S in sets for a in S for b in S), "sets that are not closed: absent tiles become zeros"
                if groups is None:
                    assert sets[R.EMPTY] == [R.EMPTY] and min(map(len, sets)) == 1, "the empty column's set {j}: a one-member set"
        assert dM.index_stamp() == stamp and same_bits(host(dM.data), M.data)


# ---- 3. the window and nothing else -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad_diag", [0.0, 1.0])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gather_writes_the_windows_and_nothing_else(eng, dtype, pad_diag):
    M = R.general(np.dtype(dtype).name)
    dM = dev(M)
    plan = dbcsr_submatrix_plan(dM, R.GROUPED)
    sets, _ = R.brute_sets(M, R.GROUPED)
    n = plan.max_dim + 3
    ld, stride = n + 5, n * (n + 5) + 7
    buf = torch.full((1 + plan.nsub * stride + 3,), nan_of(dtype), dtype=TORCH[np.dtype(dtype)], device="cuda")
    before = host(buf).copy()
    out = torch.as_strided(buf, (plan.nsub, n, n), (stride, ld, 1), 1)
    assert dbcsr_submatrix_gather(dM, plan, n=n, pad_diag=pad_diag, out=out, engine=eng) is out
    ref = R.gathered(M, "N", sets, None, n, pad_diag)
    assert same_bits(host(out), ref), "every element inside is written: no NaN is left"
    for g, S in enumerate(sets):
        ng = int(plan.sub_dim_host[g])
        pad = ref[g].copy()
        pad[:ng, :ng] = 0
        want = np.zeros((n, n), dtype)
        want[np.arange(ng, n), np.arange(ng, n)] = pad_diag
        assert ng < n and same_bits(pad, want), "the padding is +0.0 with pad_diag on the diagonal"
    after = host(buf).copy()
    inside = np.zeros(after.size, bool)
    for g in range(plan.nsub):
        inside[1 + g * stride:1 + g * stride + n * ld].reshape(n, ld)[:, :n] = True
    assert inside.sum() == plan.nsub * n * n
    assert same_bits(after[~inside], before[~inside]), "the columns n ... ld - 1 and what lies between two windows keep their NaN bits"


# ---- 4. some submatrices into the slots -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_subs_choose_the_slots(eng, dtype):
    M = R.general(np.dtype(dtype).name)
    dM = dev(M)
    plan = dbcsr_submatrix_plan(dM, R.GROUPED)
    sets, owner = R.brute_sets(M, R.GROUPED)
    subs = [3, 1]
    got = dbcsr_submatrix_gather(dM, plan, subs=subs, pad_diag=1.0, engine=eng)
    assert tuple(got.shape) == (2, plan.max_dim, plan.max_dim), "with subs given and n omitted: plan.max_dim"
    assert same_bits(host(got), R.gathered(M, "N", sets, subs, plan.max_dim, 1.0))
    n = int(max(plan.sub_dim_host[subs]))
    small = dbcsr_submatrix_gather(dM, plan, subs=torch.tensor(subs), n=n, engine=eng)
    assert same_bits(host(small), R.gathered(M, "N", sets, subs, n, 0.0))
    batch = random_batch(np.random.default_rng(71), (2, n, n), dtype)
    dB = dev(M)
    dB.data.fill_(nan_of(dtype))
    area = host(dB.data).copy()
    assert dbcsr_submatrix_scatter(torch.from_numpy(batch).cuda(), dB, plan, subs=subs, engine=eng) is dB
    want, written = R.scattered_area(M, area, sets, owner, batch, subs)
    assert same_bits(host(dB.data), want) and written == {(r, c) for r, c in blocks_of(M) if owner[c] in subs} and 0 < len(written) < M.nblks
    assert np.isnan(host(dB.data)).any(), "the blocks of the other block columns keep their NaN bits"


# ---- 5. scatter ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_scatter_writes_the_owned_blocks_and_nothing_else(eng, dtype):
    M = R.general(np.dtype(dtype).name)
    rng = np.random.default_rng(72)
    plan = dbcsr_submatrix_plan(dev(M), R.GROUPED)
    sets, owner = R.brute_sets(M, R.GROUPED)
    n = plan.max_dim + 2
    batch = random_batch(rng, (plan.nsub, n, n), dtype)
    dbatch = torch.from_numpy(batch).cuda()
    hB, dB = with_holes(eng, M, dtype)
    full = from_dense(random_batch(rng, (int(R.SQUARE.sum()),) * 2, dtype), R.SQUARE, R.SQUARE, np.dtype(dtype))   # another pattern: rows that are no members
    for hX, dX in ((M, dev(M)), (hB, dB), (M, misaligned(dev(M))), (full, dev(full))):
        # the data area one element into a tensor of NaN: guard elements in front of and behind it
        size = dX.data.numel()
        big = torch.full((size + 3,), nan_of(dtype), dtype=dX.data.dtype, device="cuda")
        big[1:1 + size].copy_(dX.data)
        dG = DbcsrMatrix(dX.row_blk_size, dX.col_blk_size, dX.row_p, dX.col_i, dX.blk_p, big[1:1 + size], nze=dX.nze)
        before = host(big).copy()
        stamp, tensors = dG.index_stamp(), (dG.row_p, dG.col_i, dG.blk_p, dG.data)
        assert dbcsr_submatrix_scatter(dbatch, dG, plan, engine=eng) is dG
        want = before.copy()
        want[1:1 + size], written = R.scattered_area(hX, before[1:1 + size], sets, owner, batch)
        assert same_bits(host(big), want), "owned blocks = the windows' elements; unowned blocks, holes and guard elements keep their bits"
        assert dG.index_stamp() == stamp and all(a is b for a, b in zip(tensors, (dG.row_p, dG.col_i, dG.blk_p, dG.data)))
        assert same_bits(host(dG.row_p), hX.row_p) and same_bits(host(dG.col_i), hX.col_i) and same_bits(host(dG.blk_p), hX.blk_p)
        assert 0 < len(written) < hX.nblks
        if hX is full:
            assert any(owner[c] >= 0 and (r, c) not in written for r, c in blocks_of(full)), "blocks whose row is not in the set keep their bits"
    assert hB.nblks == M.nblks and hB.data.size > M.data.size


def test_submatrix_between_multiplies_keeps_the_plan(monkeypatch):
    monkeypatch.delenv("DBCSR_AMD_MM_PLAN", raising=False)
    eng = MultiplyEngine()
    rng = np.random.default_rng(73)
    A = R.general("float64")
    B = from_blocks(R.SQUARE, R.SQUARE, {(r, c): GD.random_values(rng, int(R.SQUARE[r]) * int(R.SQUARE[c]), np.float64)
                                         for r in range(9) for c in range(9) if (r + 2 * c) % 3}, np.float64)
    dA, dB = to_dev(A), to_dev(B)
    dC = to_dev(subset(A, lambda r, c: False))
    dbcsr_multiply("N", "N", 1.0, dA, dB, 0.0, dC, engine=eng)
    assert eng.plan_stats() == (0, 1)
    torch.cuda.synchronize()
    first = dev_to_bcsr(dC)
    tensors = [(m.row_p, m.col_i, m.blk_p, m.data) for m in (dA, dC)]
    stamps = (dA.index_stamp(), dC.index_stamp())
    plan = dbcsr_submatrix_plan(dA)
    W = dbcsr_submatrix_gather(dA, plan, engine=eng)
    dA.data.fill_(np.nan)
    dbcsr_submatrix_scatter(W, dA, plan, engine=eng)
    dbcsr_submatrix_gather(dC, dbcsr_submatrix_plan(dC), engine=eng)   # (of its result, too)
    assert (dA.index_stamp(), dC.index_stamp()) == stamps
    assert all(a is b for m, t in zip((dA, dC), tensors) for a, b in zip((m.row_p, m.col_i, m.blk_p, m.data), t))
    dbcsr_multiply("N", "N", 1.0, dA, dB, 0.0, dC, engine=eng)
    assert eng.plan_stats() == (1, 1), "a multiply after a gather and a scatter must reuse its plan"
    torch.cuda.synchronize()
    assert same_bits(host(dA.data), A.data)
    again = dev_to_bcsr(dC)
    assert same_bits(again.col_i, first.col_i) and same_bits(again.blk_p, first.blk_p) and same_bits(again.data, first.data)


# ---- 6. round trip ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_round_trip(eng, dtype):
    name = np.dtype(dtype).name
    M = R.general(name)
    dM = dev(M)
    plan = dbcsr_submatrix_plan(dM)
    W = dbcsr_submatrix_gather(dM, plan, engine=eng)
    dZ = dev(M)
    dZ.data.zero_()
    dbcsr_submatrix_scatter(W, dZ, plan, engine=eng)
    assert same_bits(host(dZ.data), M.data), "the default plan on 'N': every stored block comes back"
    # a stored triangle: exactly the blocks whose row is in their column's set -- all of them, since (r, c) stored puts r into S_c
    symmetry = R.SYMMETRIES[name][0]
    T = R.triangle(name, below=True)
    dT = dev(T, symmetry)
    plan = dbcsr_submatrix_plan(dT, R.GROUPED)
    sets, owner = R.brute_sets(T, R.GROUPED, symmetry)
    W = dbcsr_submatrix_gather(dT, plan, engine=eng)
    dZ = dev(T, symmetry)
    dZ.data.zero_()
    dbcsr_submatrix_scatter(W, dZ, plan, engine=eng)
    want, written = R.scattered_area(T, np.zeros_like(T.data), sets, owner, host(W))
    keep = subset(T, lambda r, c: owner[c] >= 0 and r in sets[owner[c]])
    assert written == set(blocks_of(keep)) and 0 < len(written) < T.nblks
    assert same_bits(host(dZ.data), want)
    assert all(same_bits(v, blocks_of(T)[k]) for k, v in blocks_of(dev_to_bcsr(dZ)).items() if k in written)
    assert all(not v.any() for k, v in blocks_of(dev_to_bcsr(dZ)).items() if k not in written)


# ---- 7. offsets beyond 2^31 -------------------------------------------------------------------------------------------------------------------------------------
def test_batch_offsets_beyond_2_to_the_31(eng):
    """float32, two slots, batch_stride = 2^31 + 5 elements in one arena of about 8.6 GB of which only the windows and a few guard elements are touched"""
    M = R.general("float32")
    dM = dev(M)
    plan = dbcsr_submatrix_plan(dM, R.GROUPED)
    sets, owner = R.brute_sets(M, R.GROUPED)
    subs = [0, 2]
    n = int(max(plan.sub_dim_host[subs]))
    stride = 2 ** 31 + 5
    try:
        arena = torch.empty(stride + n * n + 64, dtype=torch.float32, device="cuda")
    except (RuntimeError, MemoryError) as e:
        pytest.skip("no room for the 8.6 GB arena: %s" % str(e).splitlines()[0])
    guards = [slice(n * n, n * n + 64), slice(stride - 64, stride), slice(stride + n * n, stride + n * n + 64)]
    for s in guards:
        arena[s] = np.nan
    out = torch.as_strided(arena, (2, n, n), (stride, n, 1))
    out[0].fill_(np.nan)
    out[1].fill_(np.nan)
    dbcsr_submatrix_gather(dM, plan, subs=subs, n=n, pad_diag=1.0, out=out, engine=eng)
    ref = R.gathered(M, "N", sets, subs, n, 1.0)
    assert same_bits(host(out[1]), ref[1]), "the second window, beyond 2^31 elements"
    assert same_bits(host(out[0]), ref[0]), "the first window is unharmed"
    assert all(np.isnan(host(arena[s])).all() for s in guards), "the arena around the windows is not touched"
    batch = random_batch(np.random.default_rng(74), (2, n, n), np.float32)
    out.copy_(torch.from_numpy(batch).cuda())
    dbcsr_submatrix_scatter(out, dM, plan, subs=subs, engine=eng)
    assert same_bits(host(dM.data), R.scattered_area(M, M.data, sets, owner, batch, subs)[0])
    del out, arena
    torch.cuda.empty_cache()


# ---- 8. the same bits on every call ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_same_bits_on_a_second_call_and_on_a_side_stream(eng, dtype):
    M = R.general(np.dtype(dtype).name)
    dM = dev(M)
    plan = dbcsr_submatrix_plan(dM, R.GROUPED)
    first = host(dbcsr_submatrix_gather(dM, plan, pad_diag=1.0, engine=eng))
    assert same_bits(host(dbcsr_submatrix_gather(dM, plan, pad_diag=1.0, engine=eng)), first)
    batch = torch.from_numpy(random_batch(np.random.default_rng(75), first.shape, dtype)).cuda()
    dX, dY = dev(M), dev(M)
    dbcsr_submatrix_scatter(batch, dX, plan, engine=eng)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    W = dbcsr_submatrix_gather(dM, plan, pad_diag=1.0, engine=eng, stream=side)
    dbcsr_submatrix_scatter(batch, dY, plan, engine=eng, stream=side)
    side.synchronize()
    assert same_bits(host(W), first) and same_bits(host(dY.data), host(dX.data))


# ---- 9. the workflow ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_apply_with_an_exact_function(eng, dtype):
    M = R.general(np.dtype(dtype).name)
    dM = dev(M)
    out = dbcsr_submatrix_apply(dM, lambda X: X.transpose(-1, -2).contiguous(), engine=eng)
    assert out is not dM and out.data.data_ptr() != dM.data.data_ptr() and same_bits(host(dM.data), M.data)
    sets, owner = R.brute_sets(M)
    n = max(int(R.SQUARE[S].sum()) for S in sets)
    batch = R.gathered(M, "N", sets, None, n, 1.0).transpose(0, 2, 1)
    assert same_bits(host(out.data), R.scattered_area(M, M.data, sets, owner, batch)[0])
    plan = dbcsr_submatrix_plan(dM, R.GROUPED)
    sets, owner = R.brute_sets(M, R.GROUPED)
    assert len(plan.buckets(0.1)) > 1, "several buckets of different sides"
    target = dev(M)
    target.data.fill_(nan_of(dtype))
    area = host(target.data).copy()
    assert dbcsr_submatrix_apply(dM, lambda X: X.transpose(-1, -2), plan=plan, out=target, max_waste=0.1, engine=eng) is target
    batch = R.gathered(M, "N", sets, None, plan.max_dim, 1.0).transpose(0, 2, 1)
    assert same_bits(host(target.data), R.scattered_area(M, area, sets, owner, batch)[0])


def test_apply_inverts_a_matrix_with_closed_groups(eng):
    M, A = R.spd_closed()
    dA = dev(M)
    plan = dbcsr_submatrix_plan(dA, R.CLOSED)
    out = dbcsr_submatrix_apply(dA, torch.linalg.inv, plan=plan, engine=eng)
    D = host(dbcsr_to_dense(dA, engine=eng))
    assert same_bits(D, A)
    mask = dense(from_blocks(M.row_sizes, M.col_sizes, {k: np.ones(v.size) for k, v in blocks_of(M).items()}, np.float64)) != 0
    ref = np.where(mask, np.linalg.inv(D), 0.0)
    got = dense(dev_to_bcsr(out))
    bar = R.inverse_bar(A, plan.max_dim)
    diff = float(np.max(np.abs(got - ref)))
    print("inverse by the submatrix method on the device against numpy on the whole matrix: %.3g, bar %.3g" % (diff, bar))
    assert diff <= bar


# ---- 10. C-ABI answers, empty matrices -----------------------------------------------------------------------------------------------------------------------------
def test_c_abi_answers(eng):
    M = R.general("float64")
    dM = dev(M)
    plan = dbcsr_submatrix_plan(dM, R.GROUPED)
    n = plan.max_dim
    out = torch.full((plan.nsub, n, n), np.nan, dtype=torch.float64, device="cuda")
    untouched = host(out).copy()
    lib, h, st, code = eng.L, eng.h, StreamHandle(), L.dbcsr_type_real_8
    d = dM.desc()
    dW = to_dev(GD.matrix("float64"))   # 10 x 8 blocks
    wide = dW.desc()
    area = host(dM.data).copy()
    slots = plan.all_slots()
    p = lambda t: t.data_ptr()

    def gather(handle=h, datatype=code, m=C.byref(d), kind=-1, nsub=plan.nsub, set_ptr=p(plan.set_ptr), set_idx=p(plan.set_idx), set_off=p(plan.set_off),
               sub_dim=p(plan.sub_dim), nslot=plan.nsub, slot_sub=None, max_members=plan.max_members, ptr=out.data_ptr(), n=n, ld=n, stride=n * n, pad=0.0):
        return lib.dbcsr_amd_bcsr_submatrix_gather(handle, datatype, m, kind, nsub, set_ptr, set_idx, set_off, sub_dim, nslot, slot_sub, max_members, ptr, n, ld,
                                                   stride, pad, st.ptr)

    def scatter(handle=h, datatype=code, m=C.byref(d), nsub=plan.nsub, set_ptr=p(plan.set_ptr), set_idx=p(plan.set_idx), set_off=p(plan.set_off),
                owner=p(plan.owner), sub_slot=p(slots), ptr=out.data_ptr(), n=n, ld=n, stride=n * n):
        return lib.dbcsr_amd_bcsr_submatrix_scatter(handle, datatype, ptr, n, ld, stride, nsub, set_ptr, set_idx, set_off, owner, sub_slot, m, st.ptr)

    for f in (gather, scatter):
        assert f(handle=None) == -1 and f(m=None) == -1 and f(m=C.byref(wide)) == -1, "a null handle or matrix; nblkrows != nblkcols"
        assert f(nsub=-1) == -1 and f(n=-1) == -1 and f(ld=n - 1) == -1, "a negative count; ld < n"
        assert f(ptr=None) == -1 and f(set_ptr=None) == -1 and f(set_idx=None) == -1 and f(set_off=None) == -1, "a null tensor with a non-empty batch"
        assert f(datatype=99) == -10
        assert f(n=0, ld=0, stride=0) == 0, "n == 0: nothing written"
    assert gather(nslot=-1) == -1 and gather(max_members=-1) == -1 and gather(sub_dim=None) == -1
    assert gather(kind=4) == -1 and gather(kind=-2) == -1
    assert gather(stride=n * n - 1) == -1, "batch_stride < n ld with more than one slot"
    assert gather(nslot=0) == 0 and gather(nslot=0, ptr=None) == 0 and gather(nslot=0, datatype=99) == -10
    assert scatter(owner=None) == -1 and scatter(sub_slot=None) == -1 and scatter(stride=-1) == -1
    assert scatter(nsub=0) == 0 and scatter(nsub=0, set_ptr=None, set_idx=None, set_off=None, owner=None, sub_slot=None, ptr=None) == 0
    torch.cuda.synchronize()
    assert same_bits(host(out), untouched) and same_bits(host(dM.data), area), "a refused call, and a call without work, writes nothing"
    assert gather(kind=0) == 0 and gather() == 0
    torch.cuda.synchronize()
    assert same_bits(host(out), R.gathered(M, "N", R.brute_sets(M, R.GROUPED)[0], None, n, 0.0))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_empty_matrices_and_no_submatrix(eng, dtype):
    td = TORCH[np.dtype(dtype)]
    E = subset(R.general(np.dtype(dtype).name), lambda r, c: False)
    dE = dev(E)
    plan = dbcsr_submatrix_plan(dE)
    assert (plan.nsub, plan.nmem, plan.max_members, plan.max_dim) == (R.NB, R.NB, 1, int(R.SQUARE.max()))
    got = host(dbcsr_submatrix_gather(dE, plan, pad_diag=1.0, engine=eng))
    assert same_bits(got, R.gathered(E, "N", [[j] for j in range(R.NB)], None, plan.max_dim, 1.0)) and not np.any(np.signbit(got.real))
    dbcsr_submatrix_scatter(torch.from_numpy(got).cuda(), dE, plan, engine=eng)
    assert dbcsr_submatrix_apply(dE, lambda X: X, plan=plan, engine=eng).nblks == 0
    none = np.zeros(0, np.int32)
    dZ = dev(from_blocks(none, none, {}, dtype))
    zplan = dbcsr_submatrix_plan(dZ)
    assert zplan.nsub == 0 and tuple(dbcsr_submatrix_gather(dZ, zplan, engine=eng).shape) == (0, 0, 0)
    dbcsr_submatrix_scatter(torch.zeros((0, 0, 0), dtype=td, device="cuda"), dZ, zplan, engine=eng)
    assert dbcsr_submatrix_apply(dZ, torch.linalg.inv, engine=eng).nblks == 0
    # nsub = 0: no block column has a submatrix
    M = R.general(np.dtype(dtype).name)
    dM = dev(M)
    nplan = dbcsr_submatrix_plan(dM, [-1] * R.NB)
    assert (nplan.nsub, nplan.nmem, nplan.max_dim) == (0, 0, 0)
    assert tuple(dbcsr_submatrix_gather(dM, nplan, engine=eng).shape) == (0, 0, 0)
    dbcsr_submatrix_scatter(torch.zeros((0, 5, 5), dtype=td, device="cuda"), dM, nplan, engine=eng)
    assert dbcsr_submatrix_apply(dM, torch.linalg.inv, plan=nplan, engine=eng) is not dM
    assert same_bits(host(dM.data), M.data)


# ---- 11. refusals ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_call(monkeypatch):
    class Refuses:
        def __getattr__(self, name):
            raise AssertionError("the library was called (%s)" % name)

    eng = MultiplyEngine()
    monkeypatch.setattr(eng, "L", Refuses())
    M = R.general("float64")
    dM = dev(M)
    plan = dbcsr_submatrix_plan(dM, R.GROUPED)
    n, ns = plan.max_dim, plan.nsub
    good = torch.zeros((ns, n, n), dtype=torch.float64, device="cuda")
    wide = torch.zeros((ns, 2 * n, 2 * n), dtype=torch.float64, device="cuda")
    size = dM.data.numel()
    big = torch.zeros(size + ns * n * n, dtype=torch.float64, device="cuda")
    inside = DbcsrMatrix(dM.row_blk_size, dM.col_blk_size, dM.row_p, dM.col_i, dM.blk_p, big[:size])
    over = torch.as_strided(big, (ns, n, n), (n * n, n, 1), size - 1)
    bad = [
        (TypeError, np.zeros((ns, n, n))),                                                          # not a tensor
        (TypeError, good.to(torch.float32)),                                                        # wrong data type
        (ValueError, good.cpu()),                                                                   # wrong device
        (ValueError, good[:-1]),                                                                    # wrong shape
        (ValueError, good[:, :, :-1]),
        (ValueError, good.reshape(ns, -1)),
        (ValueError, wide[:, ::2, ::2]),                                                            # stride(2) is not 1
        (ValueError, good.transpose(1, 2)),
        (ValueError, torch.zeros(n, dtype=torch.float64, device="cuda").expand(ns, n, n)),          # rows that overlap: ld too small
        (ValueError, torch.zeros((n, n), dtype=torch.float64, device="cuda").expand(ns, n, n)),     # windows that overlap: batch_stride too small
    ]
    stamp, area = dM.index_stamp(), dM.data.clone()
    for error, t in bad:
        with pytest.raises(error):
            dbcsr_submatrix_gather(dM, plan, out=t, engine=eng)
        with pytest.raises(error):
            dbcsr_submatrix_scatter(t, dM, plan, engine=eng)
    for f in (lambda: dbcsr_submatrix_gather(inside, plan, out=over, engine=eng), lambda: dbcsr_submatrix_scatter(over, inside, plan, engine=eng),
              lambda: dbcsr_submatrix_apply(dM, torch.linalg.inv, plan=plan, out=dM, engine=eng)):
        with pytest.raises(ValueError, match="overlap"):
            f()
    for subs in ([0, ns], [-1], [1, 1]):
        with pytest.raises(ValueError):
            dbcsr_submatrix_gather(dM, plan, subs=subs, engine=eng)
        with pytest.raises(ValueError):
            dbcsr_submatrix_scatter(good[:len(subs)], dM, plan, subs=subs, engine=eng)
    for pad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError):
            dbcsr_submatrix_gather(dM, plan, pad_diag=pad, engine=eng)
        with pytest.raises(ValueError):
            dbcsr_submatrix_apply(dM, torch.linalg.inv, plan=plan, pad_diag=pad, engine=eng)
    with pytest.raises(ValueError):
        dbcsr_submatrix_gather(dM, plan, n=n - 1, engine=eng)
    sizes2 = np.ascontiguousarray(R.SQUARE[::-1])
    other = dev(from_blocks(sizes2, sizes2, {(0, 0): np.ones(1)}, np.float64))
    fewer = dev(from_blocks(sizes2[:4], sizes2[:4], {}, np.float64))
    for wrong in (other, fewer):   # a plan made for another block structure
        with pytest.raises(ValueError):
            dbcsr_submatrix_gather(wrong, plan, engine=eng)
        with pytest.raises(ValueError):
            dbcsr_submatrix_scatter(good, wrong, plan, engine=eng)
        with pytest.raises(ValueError):
            dbcsr_submatrix_apply(dM, torch.linalg.inv, plan=plan, out=wrong, engine=eng)
    with pytest.raises(TypeError):
        dbcsr_submatrix_apply(dM, torch.linalg.inv, plan=plan, out=dev(R.general("float32")), engine=eng)
    ints = DbcsrMatrix(dM.row_blk_size, dM.col_blk_size, dM.row_p, dM.col_i, dM.blk_p, torch.zeros(size, dtype=torch.int32, device="cuda"))
    with pytest.raises(TypeError):
        dbcsr_submatrix_gather(ints, plan, engine=eng)
    for sym in ("X", "H"):   # an unknown symmetry; a symmetry that real data does not have
        dM.symmetry = sym
        with pytest.raises(ValueError):
            dbcsr_submatrix_gather(dM, plan, engine=eng)
        with pytest.raises(ValueError):
            dbcsr_submatrix_scatter(good, dM, plan, engine=eng)
    dM.symmetry = "N"
    with pytest.raises(ValueError):
        dbcsr_submatrix_plan(dM, [0, 2] + [0] * 7)
    with pytest.raises(ValueError):
        dbcsr_submatrix_plan(to_dev(GD.matrix("float64")))
    assert dM.index_stamp() == stamp and torch.equal(dM.data, area)
