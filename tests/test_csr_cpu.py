"""What tests/test_gpu_csr.py compares with, checked without a GPU: the inputs of the eps cases keep every non-zero, non-NaN magnitude outside
[EPS / 2, 2 EPS] (so no rounding of hypot decides an element) with kept and dropped elements, a row and a block that lose everything, a block that keeps
everything, +-0.0, NaN and +-Inf all there; the numpy reference (tests/csr_ref.py) round-trips and agrees with torch's to_sparse_csr() on the host; the four C
entries are declared in the header and listed once in lib.MM_SYMBOLS (tests/test_cabi_symbols.py then checks the export); the four Python names are
exported; and the refusals that need no device come before any call of the library."""
import os
import re

import numpy as np
import pytest
import torch

import dbcsr_amd
from dbcsr_amd import csr as CSR
from dbcsr_amd import lib as L
from dbcsr_amd.matrix import DbcsrMatrix
from tests import csr_ref as R
from tests import test_gpu_dense as GD
from tests.test_gpu_matrix_norms import blocks_of, dense, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the eps cases ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.IDS)
def test_eps_inputs_keep_every_magnitude_away_from_eps(dtype):
    M = R.eps_case(np.dtype(dtype).name)
    mag = R.magnitudes(M)
    known = ~np.isnan(mag) & (mag != 0)
    assert not np.any((mag[known] >= R.EPS / 2) & (mag[known] <= 2 * R.EPS))
    keep = np.asarray([R.kept(x, R.EPS) for x in M.data])
    assert np.array_equal(keep[known], mag[known] > 2 * R.EPS) and keep[np.isnan(mag)].all() and not keep[mag == 0].any()
    assert keep.sum() >= 10 and (~keep).sum() >= 10
    per_block = {k: np.asarray([R.kept(x, R.EPS) for x in v]) for k, v in blocks_of(M).items()}
    assert any(not k.any() for k in per_block.values()), "a block that loses every element"
    assert any(k.all() for k in per_block.values()), "a block that keeps every element"
    special = blocks_of(M)[(4, 7)][:5]
    assert special[0] == 0 and special[1] == 0 and not np.signbit(special[0].real) and np.signbit(special[1].real)
    assert np.isnan(special[2]) and np.isinf(special[3]) and np.isinf(special[4]) and special[3].real > 0 > special[4].real
    crow = R.to_csr(M, R.EPS)[0]
    i = int(R.offsets(M.row_sizes)[R.LOSING_ROW[0]]) + R.LOSING_ROW[1]
    assert M.row_p[R.LOSING_ROW[0]] < M.row_p[R.LOSING_ROW[0] + 1] and crow[i] == crow[i + 1], "an empty CSR row inside a stored block row"
    assert crow[i - 1] < crow[i] < crow[-1]
    zero_crow, _, zero_values = R.to_csr(M, 0.0)
    assert zero_values.size == M.data.size - 2 and zero_crow[-1] == zero_values.size, "eps = 0 drops exactly the two zeros"
    assert np.isnan(R.to_csr(M, R.EPS)[2]).sum() == 1, "the NaN stays"


# ---- the reference ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.IDS)
def test_the_reference_round_trips(dtype):
    name = np.dtype(dtype).name
    for M in (R.base(name), R.full(name), R.eps_case(name)):
        crow, col, values = R.to_csr(M, None)
        assert crow.dtype == np.int64 and col.dtype == np.int32 and values.dtype == M.data.dtype
        assert crow[0] == 0 and crow[-1] == values.size == M.data.size and np.all(np.diff(crow) >= 0)
        assert all(np.all(np.diff(col[crow[i]:crow[i + 1]]) > 0) for i in range(len(crow) - 1)), "columns ascend strictly inside a row"
        area = np.full(M.data.size, np.nan, M.data.dtype)
        assert same_bits(R.from_csr(crow, col, values, M, area), M.data)
        assert R.blocks_of_csr(crow, col, M.row_sizes, M.col_sizes) == set(blocks_of(M))
    M = R.eps_case(name)
    crow, col, values = R.to_csr(M, R.EPS)
    back = R.from_csr(crow, col, values, M)
    keep = np.asarray([R.kept(x, R.EPS) for x in M.data])
    assert same_bits(back[keep], M.data[keep]) and same_bits(back[~keep], np.zeros(int((~keep).sum()), M.data.dtype)), "+0.0 where elements were dropped"


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.IDS)
def test_the_reference_against_torch_on_the_host(dtype):
    M = R.nonzero(np.dtype(dtype).name)
    assert not np.any(M.data == 0)
    crow, col, values = R.to_csr(M, None)
    T = torch.from_numpy(dense(M)).to_sparse_csr()
    assert np.array_equal(T.crow_indices().numpy(), crow) and np.array_equal(T.col_indices().numpy(), col.astype(np.int64))
    assert same_bits(T.values().numpy(), values)
    back = CSR.dbcsr_csr_to_torch(torch.from_numpy(crow), torch.from_numpy(col), torch.from_numpy(values), dense(M).shape)
    assert back.layout == torch.sparse_csr and back.col_indices().dtype == torch.int64 and same_bits(back.to_dense().numpy(), dense(M))


# ---- the entries -----------------------------------------------------------------------------------------------------------------------------------------
def test_the_entries_are_declared_and_listed():
    header = " ".join(open(os.path.join(ROOT, "include", "dbcsr_amd_mm.h")).read().split())
    want = {
        "dbcsr_amd_bcsr_to_csr_count": "void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* m, int use_eps, double eps, int64_t* crow, "
                                       "int64_t* nnz, void* stream",
        "dbcsr_amd_bcsr_to_csr_apply": "void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* m, int32_t* col, void* values, void* stream",
        "dbcsr_amd_bcsr_from_csr": "void* handle, libsmm_acc_data_t datatype, int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t* crow, "
                                   "const int32_t* col, const void* values, dbcsr_amd_bcsr* m, void* stream",
        "dbcsr_amd_bcsr_csr_name_blocks": "void* handle, int64_t n_rows, int64_t nnz, const int64_t* crow, const int32_t* col, const int32_t* row_blk_size, "
                                          "const int32_t* col_blk_size, int nblkrows, int nblkcols, int32_t* rows, int32_t* cols, void* stream",
    }
    assert "Element CSR" in header
    for name, args in want.items():
        m = re.search(r"int %s\(([^;]*)\);" % name, header)
        assert m and m.group(1) == args, name
        assert L.MM_SYMBOLS.count(name) == 1


def test_the_names_are_exported():
    for name in ("dbcsr_to_csr", "dbcsr_from_csr", "dbcsr_create_from_csr", "dbcsr_csr_to_torch"):
        assert name in dbcsr_amd.__all__ and getattr(dbcsr_amd, name) is getattr(CSR, name)
        assert name + "(" in CSR.__doc__
    assert "not available here" in CSR.__doc__ and "this library's semantics" in CSR.dbcsr_to_csr.__doc__


class Refuses:
    L = property(lambda self: (_ for _ in ()).throw(AssertionError("the library was called")))
    h = None

    def desymmetrized(self, *a, **k):
        raise AssertionError("the library was called")


def host_matrix(dtype=torch.float64):
    """a matrix whose tensors stay on the host: enough for every check that comes before the library"""
    M = GD.matrix("float64")
    t = torch.from_numpy
    return DbcsrMatrix(t(M.row_sizes), t(M.col_sizes), t(M.row_p), t(M.col_i), t(M.blk_p), t(M.data).to(dtype))


def test_refusals_that_need_no_device():
    eng = Refuses()
    dM = host_matrix()
    crow, col, values = (torch.from_numpy(a) for a in R.to_csr(GD.matrix("float64"), None))
    for eps in (-1.0, float("nan"), -0.5):
        with pytest.raises(ValueError, match="eps"):
            CSR.dbcsr_to_csr(dM, eps=eps, engine=eng)
    with pytest.raises(ValueError, match="host"):
        CSR.dbcsr_to_csr(dM, engine=eng)
    with pytest.raises(ValueError, match="host"):
        CSR.dbcsr_from_csr(crow, col, values, dM, engine=eng)
    for sym in ("X", "H"):   # unknown; not one of real data
        dM.symmetry = sym
        with pytest.raises(ValueError):
            CSR.dbcsr_to_csr(dM, engine=eng)
        with pytest.raises(ValueError):
            CSR.dbcsr_from_csr(crow, col, values, dM, engine=eng)
    with pytest.raises(TypeError):
        CSR.dbcsr_to_csr(host_matrix(torch.int32), engine=eng)
    rs, cs = GD.ROWS, GD.COLS
    for error, args in [(TypeError, (crow, col, values.numpy(), rs, cs)), (TypeError, (crow, col, values.to(torch.int32), rs, cs)),
                        (ValueError, (crow, col, values, rs, cs))]:   # (the last: tensors on the host)
        with pytest.raises(error):
            CSR.dbcsr_create_from_csr(*args, engine=eng)
    f = lambda **k: CSR._check_csr("t", k.get("crow", crow), k.get("col", col), k.get("values", values), torch.float64, crow.device, k.get("n", crow.numel() - 1))
    assert all(a is b for a, b in zip(f(), (crow, col, values)))
    for error, k in [(TypeError, {"crow": crow.to(torch.int32)}), (TypeError, {"col": col.to(torch.int64)}), (TypeError, {"values": values.to(torch.float32)}),
                     (TypeError, {"crow": crow.numpy()}), (ValueError, {"crow": crow[:-1]}), (ValueError, {"col": col[:-1]}),
                     (ValueError, {"values": values.reshape(1, -1)}), (ValueError, {"n": crow.numel()})]:
        with pytest.raises(error):
            f(**k)


def test_more_columns_than_int32_are_refused():
    """n_cols > 2^31 - 1: col is int32 (the sizes are checked before the library is reached; nothing of that size is allocated)"""
    rs = torch.tensor([1], dtype=torch.int32)
    cs = torch.tensor([2 ** 30, 2 ** 30], dtype=torch.int32)
    one = torch.zeros(1, dtype=torch.float64)
    M = DbcsrMatrix(rs, cs, torch.zeros(2, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.int64), one)
    assert CSR._full_size(cs) == 2 ** 31
    crow = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(ValueError, match="int32"):
        CSR.dbcsr_to_csr(M, engine=Refuses())
    with pytest.raises(ValueError, match="int32"):
        CSR.dbcsr_from_csr(crow, torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.float64), M, engine=Refuses())
