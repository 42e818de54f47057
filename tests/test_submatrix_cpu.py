"""The submatrix method without a GPU (dbcsr_amd/submatrix.py): the plan builder on host tensors against a brute-force restatement for all five symmetries,
with group arrays that hold -1, an empty block column and zero-size blocks; buckets() keeps its waste cap and puts every submatrix into exactly one
bucket; the numpy helpers of tests/submatrix_ref.py agree with dense / twin_dense on the full set; the bar of the inverse workflow is met by numpy against
torch on the host, with the measured figure printed; the two C entries are declared in the header with their argument lists and listed in lib.MM_SYMBOLS
(tests/test_cabi_symbols.py then checks the export); the Python names are exported; and the refusals that need no device come before any call of the
library."""
import os
import re

import numpy as np
import pytest
import torch

import dbcsr_amd
from dbcsr_amd import lib as L
from dbcsr_amd import submatrix as SM
from dbcsr_amd.matrix import DbcsrMatrix
from tests import submatrix_ref as R
from tests import test_gpu_dense as GD
from tests.test_gpu_matrix_norms import blocks_of, dense, from_blocks, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_matrix(M, symmetry="N", dtype=None):
    """a matrix whose tensors stay on the host: enough for the plan builder and for every check that comes before the library"""
    t = torch.from_numpy
    data = t(M.data) if dtype is None else t(M.data).to(dtype)
    rs = t(np.ascontiguousarray(M.row_sizes, np.int32))
    return DbcsrMatrix(rs, rs, t(M.row_p), t(M.col_i), t(M.blk_p), data, symmetry=symmetry)


def check_plan(plan, M, groups, symmetry):
    sets, owner = R.brute_sets(M, groups, symmetry)
    set_ptr, set_idx, set_off, sub_dim = R.plan_arrays(sets, M.row_sizes)
    for name, want in (("set_ptr", set_ptr), ("set_idx", set_idx), ("set_off", set_off), ("sub_dim", sub_dim), ("owner", np.asarray(owner, np.int32))):
        got = getattr(plan, name)
        assert got.dtype == torch.int32 and got.is_contiguous() and same_bits(got.numpy(), want), name
    assert (plan.nsub, plan.nmem) == (len(sets), len(set_idx))
    assert plan.max_members == max((len(S) for S in sets), default=0) and plan.max_dim == max(sub_dim.tolist(), default=0)
    assert plan.sub_dim_host.tolist() == sub_dim.tolist() and plan.members_host.tolist() == [len(S) for S in sets]
    for g, S in enumerate(sets):
        assert all(j in S for j in range(len(owner)) if owner[j] == g) and S == sorted(S)
    return sets


CASES = [("N", "float64"), ("N", "complex128"), ("S", "float64"), ("A", "float32"), ("H", "complex128"), ("K", "complex128")]


@pytest.mark.parametrize("symmetry,dtype_name", CASES, ids=["%s-%s" % c for c in CASES])
def test_plan_against_brute_force(symmetry, dtype_name):
    mats = [R.general(dtype_name)] if symmetry == "N" else [R.triangle(dtype_name), R.triangle(dtype_name, below=True)]
    for M in mats:
        dM = host_matrix(M, symmetry)
        stamp = dM.index_stamp()
        for groups in (None, R.GROUPED, torch.tensor(R.GROUPED), np.asarray([-1] * R.NB), [0] * R.NB, [2, 2, 1, 1, 0, 0, -1, -1, 0]):
            plan = SM.dbcsr_submatrix_plan(dM, groups)
            sets = check_plan(plan, M, groups if groups is None else [int(g) for g in groups], symmetry)
            assert plan.stamp == stamp == dM.index_stamp() and plan.row_blk_size is dM.row_blk_size
            if groups is None and symmetry == "N":
                assert sets[R.EMPTY] == [R.EMPTY], "the empty block column's set is the column itself"
                assert all(j in sets[j] for j in R.NO_DIAG), "j is a member without a stored diagonal block"
    if symmetry != "N":   # both placements of the triangle stand for one full pattern: the same sets
        a, b = (R.brute_sets(M, R.GROUPED, symmetry)[0] for M in mats)
        assert a == b


def test_plan_with_zero_size_blocks_and_without_blocks():
    sizes = np.asarray([3, 0, 2, 0, 4], np.int32)
    rng = np.random.default_rng(3)
    blocks = {(r, c): rng.uniform(-1, 1, int(sizes[r]) * int(sizes[c])) for r, c in ((0, 0), (0, 1), (1, 3), (2, 0), (3, 3), (4, 2), (1, 4), (4, 4))}
    M = from_blocks(sizes, sizes, blocks, np.float64)
    for groups in (None, [0, 1, 1, -1, 0], [0, 0, 0, 0, 0]):
        plan = SM.dbcsr_submatrix_plan(host_matrix(M), groups)
        check_plan(plan, M, groups, "N")
    E = from_blocks(sizes, sizes, {}, np.float64)
    plan = SM.dbcsr_submatrix_plan(host_matrix(E))
    check_plan(plan, E, None, "N")
    assert plan.nmem == 5 and plan.max_members == 1
    none = np.zeros(0, np.int32)
    Z = SM.dbcsr_submatrix_plan(host_matrix(from_blocks(none, none, {}, np.float64)))
    assert (Z.nsub, Z.nmem, Z.max_members, Z.max_dim) == (0, 0, 0, 0) and Z.set_ptr.tolist() == [0] and Z.buckets() == []
    unowned = SM.dbcsr_submatrix_plan(host_matrix(M), [-1] * 5)
    assert unowned.nsub == 0 and unowned.set_ptr.tolist() == [0] and unowned.owner.tolist() == [-1] * 5


def test_plan_refusals():
    M = R.general("float64")
    dM = host_matrix(M)
    for error, groups in [(ValueError, [0, 1, 2]), (ValueError, [0, 2, 2, 2, 2, 2, 2, 2, 2]), (ValueError, [-2] + [0] * 8), (ValueError, [9] + [0] * 8),
                          (TypeError, [0.0] * 9), (TypeError, np.zeros((3, 3), np.int64)), (ValueError, [1] * 9)]:
        with pytest.raises(error):
            SM.dbcsr_submatrix_plan(dM, groups)
    G = GD.matrix("float64")   # 10 x 8 blocks
    t = torch.from_numpy
    with pytest.raises(ValueError):
        SM.dbcsr_submatrix_plan(DbcsrMatrix(t(G.row_sizes), t(G.col_sizes), t(G.row_p), t(G.col_i), t(G.blk_p), t(G.data)))
    other = t(np.ascontiguousarray(M.row_sizes[::-1]))
    with pytest.raises(ValueError):   # square in blocks, but the row block sizes are not the column block sizes
        SM.dbcsr_submatrix_plan(DbcsrMatrix(dM.row_blk_size, other, dM.row_p, dM.col_i, dM.blk_p, dM.data))
    for sym in ("X", "H"):
        dM.symmetry = sym
        with pytest.raises(ValueError):
            SM.dbcsr_submatrix_plan(dM)


def test_buckets_keep_their_waste_cap():
    M = R.general("float64")
    for groups in (None, R.GROUPED):
        plan = SM.dbcsr_submatrix_plan(host_matrix(M), groups)
        dims = plan.sub_dim_host
        for cap in (0.0, 0.1, 0.5, 0.9, 1.0):
            buckets = plan.buckets(cap)
            assert sorted(g for b in buckets for g in b) == list(range(plan.nsub)), "every submatrix in exactly one bucket"
            for b in buckets:
                n = int(dims[b].max())
                used, total = int((dims[b] ** 2).sum()), len(b) * n * n
                assert total - used <= cap * total, (cap, b)
                assert b == sorted(b)
            if cap == 0.0:
                assert all(len(set(dims[b].tolist())) == 1 for b in buckets)
            if cap == 1.0:
                assert len(buckets) == 1
    with pytest.raises(ValueError):
        plan.buckets(-0.1)
    with pytest.raises(ValueError):
        plan.buckets(float("nan"))


@pytest.mark.parametrize("dtype", GD.DTYPES, ids=GD.IDS)
def test_the_helpers_agree_with_dense_on_the_full_set(dtype):
    name = np.dtype(dtype).name
    M = R.general(name)
    everything = [list(range(R.NB))]
    n = int(R.SQUARE.sum())
    assert same_bits(R.gathered(M, "N", everything, None, n, 0.0)[0], dense(M))
    for symmetry in R.SYMMETRIES[name]:
        for T in (R.triangle(name), R.triangle(name, below=True)):
            assert same_bits(R.gathered(T, symmetry, everything, None, n, 1.0)[0], GD.twin_dense(T, symmetry))
    W = R.gathered(M, "N", everything, None, n + 3, 1.0)[0]
    assert same_bits(W[:n, :n], dense(M)) and not W[:n, n:].any() and not W[n:, :n].any() and same_bits(W[n:, n:], np.eye(3, dtype=dtype))
    # gather then scatter on the default plan gives back every stored block
    sets, owner = R.brute_sets(M, None, "N")
    batch = R.gathered(M, "N", sets, None, int(max(R.plan_arrays(sets, R.SQUARE)[3])), 0.0)
    area, written = R.scattered_area(M, np.zeros_like(M.data), sets, owner, batch)
    assert same_bits(area, M.data) and written == set(blocks_of(M))
    sets, owner = R.brute_sets(M, R.GROUPED, "N")
    batch = R.gathered(M, "N", sets, [3, 1], 200, 0.0)
    area, written = R.scattered_area(M, np.zeros_like(M.data), sets, owner, batch, [3, 1])
    assert written == {(r, c) for r, c in blocks_of(M) if owner[c] in (3, 1)} and 0 < len(written) < M.nblks


def test_the_inverse_bar_is_met_on_the_host():
    M, A = R.spd_closed()
    sets, owner = R.brute_sets(M, R.CLOSED, "N")
    assert owner == R.CLOSED and all(S == [j for j in range(R.NB) if R.CLOSED[j] == g] for g, S in enumerate(sets)), "the groups' sets are closed"
    assert np.linalg.eigvalsh(A).min() >= 1.0
    n_window = int(max(R.plan_arrays(sets, R.SQUARE)[3]))
    bar = R.inverse_bar(A, n_window)
    ref = np.linalg.inv(A)
    # the submatrix method on the host: torch inverts the windows, numpy the whole matrix
    got = np.zeros_like(A)
    for S in sets:
        e = R.elements_of(S, R.SQUARE)
        got[np.ix_(e, e)] = torch.linalg.inv(torch.from_numpy(A[np.ix_(e, e)])).numpy()
    diff = float(np.max(np.abs(got - ref)))
    print("inverse by windows (torch on the host) against numpy on the whole matrix: %.3g, bar n u kappa ||A^-1|| = %.3g (n = %d, kappa = %.3g)"
          % (diff, bar, n_window, np.linalg.cond(A, 2)))
    assert diff <= bar / 4 <= 1e-12, "met with room to spare"


def test_the_entries_are_declared_and_listed():
    header = " ".join(open(os.path.join(ROOT, "include", "dbcsr_amd_mm.h")).read().split())
    want = {
        "dbcsr_amd_bcsr_submatrix_gather": "void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* m, int kind, int nsub, const int32_t* set_ptr, "
                                           "const int32_t* set_idx, const int32_t* set_off, const int32_t* sub_dim, int nslot, const int32_t* slot_sub, "
                                           "int max_members, void* dense, int64_t n, int64_t ld, int64_t batch_stride, double pad_diag, void* stream",
        "dbcsr_amd_bcsr_submatrix_scatter": "void* handle, libsmm_acc_data_t datatype, const void* dense, int64_t n, int64_t ld, int64_t batch_stride, int nsub, "
                                            "const int32_t* set_ptr, const int32_t* set_idx, const int32_t* set_off, const int32_t* owner, "
                                            "const int32_t* sub_slot, dbcsr_amd_bcsr* m, void* stream",
    }
    assert "Submatrix method" in header
    for name, args in want.items():
        m = re.search(r"int %s\(([^;]*)\);" % name, header)
        assert m and m.group(1) == args, name
        assert name in L.MM_SYMBOLS


def test_the_names_are_exported():
    for name in ("SubmatrixPlan", "dbcsr_submatrix_plan", "dbcsr_submatrix_gather", "dbcsr_submatrix_scatter", "dbcsr_submatrix_apply"):
        assert name in dbcsr_amd.__all__ and getattr(dbcsr_amd, name) is getattr(SM, name)
        if name != "SubmatrixPlan":
            assert name + "(" in SM.__doc__


class Refuses:
    L = property(lambda self: (_ for _ in ()).throw(AssertionError("the library was called")))
    h = None


def test_refusals_that_need_no_device():
    eng = Refuses()
    M = R.general("float64")
    dM = host_matrix(M)
    plan = SM.dbcsr_submatrix_plan(dM, R.GROUPED)
    n, ns = plan.max_dim, plan.nsub
    good = torch.zeros((ns, n, n), dtype=torch.float64)
    wide = torch.zeros((ns, 2 * n, 2 * n), dtype=torch.float64)
    bad = [(TypeError, good.numpy()), (TypeError, good.to(torch.float32)), (ValueError, good[:-1]), (ValueError, good[:, :-1]), (ValueError, good.reshape(ns, -1)),
           (ValueError, wide[:, ::2, ::2]), (ValueError, good.transpose(1, 2)),
           (ValueError, torch.zeros(n, dtype=torch.float64).expand(ns, n, n)),            # rows that overlap: ld too small
           (ValueError, torch.zeros((n, n), dtype=torch.float64).expand(ns, n, n))]       # windows that overlap: batch_stride too small
    for error, t in bad:
        with pytest.raises(error):
            SM.dbcsr_submatrix_gather(dM, plan, out=t, engine=eng)
        with pytest.raises(error):
            SM.dbcsr_submatrix_scatter(t, dM, plan, engine=eng)
    for subs in ([0, 4], [-1], [1, 1], [0.5]):
        with pytest.raises((ValueError, TypeError)):
            SM.dbcsr_submatrix_gather(dM, plan, subs=subs, engine=eng)
        with pytest.raises((ValueError, TypeError)):
            SM.dbcsr_submatrix_scatter(good[:1], dM, plan, subs=subs, engine=eng)
    for pad in (float("nan"), float("inf")):
        with pytest.raises(ValueError):
            SM.dbcsr_submatrix_gather(dM, plan, pad_diag=pad, engine=eng)
        with pytest.raises(ValueError):
            SM.dbcsr_submatrix_apply(dM, torch.linalg.inv, plan=plan, pad_diag=pad, engine=eng)
    with pytest.raises(ValueError):   # n below a side
        SM.dbcsr_submatrix_gather(dM, plan, n=n - 1, engine=eng)
    with pytest.raises(ValueError):
        SM.dbcsr_submatrix_scatter(good[:, :n - 1, :n - 1], dM, plan, engine=eng)
    # overlap with the matrix' data area
    size = dM.data.numel()
    big = torch.zeros(size + ns * n * n, dtype=torch.float64)
    inside = DbcsrMatrix(dM.row_blk_size, dM.col_blk_size, dM.row_p, dM.col_i, dM.blk_p, big[:size])
    over = torch.as_strided(big, (ns, n, n), (n * n, n, 1), size - 1)
    with pytest.raises(ValueError, match="overlap"):
        SM.dbcsr_submatrix_gather(inside, plan, out=over, engine=eng)
    with pytest.raises(ValueError, match="overlap"):
        SM.dbcsr_submatrix_scatter(over, inside, plan, engine=eng)
    with pytest.raises(ValueError, match="overlap"):
        SM.dbcsr_submatrix_apply(dM, torch.linalg.inv, plan=plan, out=dM, engine=eng)
    # a plan made for another block structure
    sizes2 = np.ascontiguousarray(R.SQUARE[::-1])
    other = host_matrix(from_blocks(sizes2, sizes2, {(0, 0): np.ones(1)}, np.float64))
    small = host_matrix(from_blocks(sizes2[:4], sizes2[:4], {}, np.float64))
    for wrong in (other, small):
        with pytest.raises(ValueError):
            SM.dbcsr_submatrix_gather(wrong, plan, engine=eng)
        with pytest.raises(ValueError):
            SM.dbcsr_submatrix_scatter(good, wrong, plan, engine=eng)
        with pytest.raises(ValueError):
            SM.dbcsr_submatrix_apply(dM, torch.linalg.inv, plan=plan, out=wrong, engine=eng)
    with pytest.raises(TypeError):
        SM.dbcsr_submatrix_gather(dM, "plan", engine=eng)
    with pytest.raises(TypeError):
        SM.dbcsr_submatrix_gather(host_matrix(M, dtype=torch.int32), plan, engine=eng)
    with pytest.raises(TypeError):
        SM.dbcsr_submatrix_apply(dM, None, plan=plan, engine=eng)
    dM.symmetry = "H"
    with pytest.raises(ValueError):
        SM.dbcsr_submatrix_gather(dM, plan, engine=eng)
