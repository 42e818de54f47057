"""What tests/test_gpu_dense.py compares with, checked without a GPU: the inputs of the eps cases keep every block norm outside [EPS / 2, 2 EPS] with kept and
dropped blocks both there (so no rounding of a norm decides a block); the host helpers round-trip (from_dense -> dense, the sign-flip reading of a stored
triangle against desymmetrized_dense); the bar of the eigenvalue workflow is met by numpy against torch on the host, with the measured figure printed; the three C
entries are declared in the header and listed in lib.MM_SYMBOLS (tests/test_cabi_symbols.py then checks the export); the three Python names are exported;
and the refusals that need no device come before any call of the library (matrices and tensors held on the host never reach it)."""
import os
import re

import numpy as np
import pytest
import torch

import dbcsr_amd
from dbcsr_amd import lib as L
from dbcsr_amd import operations as OPS
from dbcsr_amd.matrix import DbcsrMatrix
from tests import test_gpu_dense as GD
from tests.test_gpu_matrix_norms import blocks_of, dense, desymmetrized_dense, from_dense, same_bits, subset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("dtype", GD.DTYPES, ids=GD.IDS)
def test_eps_inputs_keep_every_norm_away_from_eps(dtype):
    D, keep = GD.eps_case(np.dtype(dtype).name)
    norms = GD.tile_norms(D, GD.ROWS, GD.COLS)
    assert np.isnan(norms[3, 2]) and np.isnan(norms).sum() == 1 and keep[3, 2], "one tile holds a NaN, and stays"
    known = ~np.isnan(norms)
    assert not np.any((norms[known] >= GD.EPS / 2) & (norms[known] <= 2 * GD.EPS))
    assert np.array_equal(keep[known], norms[known] > 2 * GD.EPS)
    assert keep.sum() >= 10 and (~keep).sum() >= 10 and np.any((norms > 0) & ~keep) and np.any(norms == 0), "kept, small and zero tiles all occur"
    assert not keep[list(GD.EMPTY_ROWS)].any(), "block rows without a kept block"
    H = GD.filtered_host(D, GD.ROWS, GD.COLS, GD.EPS)
    assert set(blocks_of(H)) == {(r, c) for r in range(len(GD.ROWS)) for c in range(len(GD.COLS)) if keep[r, c]}


@pytest.mark.parametrize("dtype", GD.DTYPES, ids=GD.IDS)
def test_host_helpers_round_trip(dtype):
    name = np.dtype(dtype).name
    M = GD.matrix(name)
    assert set(GD.ROWS.tolist()) | set(GD.COLS.tolist()) >= {1, 5, 13, 23, 32, 33, 40, 64, 96} and len(GD.ROWS) != len(GD.COLS)
    D = dense(M)
    full = from_dense(D, M.row_sizes, M.col_sizes, np.dtype(dtype))
    assert same_bits(dense(full), D)
    back = subset(full, lambda r, c: (r, c) in blocks_of(M))
    assert same_bits(back.data, M.data) and same_bits(back.col_i, M.col_i) and same_bits(back.blk_p, M.blk_p)
    assert same_bits(GD.expected_area(M, np.zeros_like(M.data), D), M.data)
    for symmetry in (("H", "K") if GD.is_complex(dtype) else ("S", "A")):
        T = GD.matrix(name, "triangle", zeros=False)
        assert same_bits(GD.twin_dense(T, symmetry), desymmetrized_dense(T, symmetry))
        Z = GD.matrix(name, "triangle", zeros=True)
        assert np.array_equal(GD.twin_dense(Z, symmetry), desymmetrized_dense(Z, symmetry))
        if symmetry in ("A", "K"):
            assert not same_bits(GD.twin_dense(Z, symmetry), desymmetrized_dense(Z, symmetry)), "the twin of +0.0 is -0.0; the helper's sum gives +0.0"


def test_the_eigenvalue_bar_is_met_on_the_host():
    M, A = GD.spd_case()
    assert same_bits(desymmetrized_dense(M, "S"), A) and np.linalg.eigvalsh(A).min() >= 1.0
    diff = float(np.max(np.abs(np.linalg.eigvalsh(A) - torch.linalg.eigvalsh(torch.from_numpy(A)).numpy())))
    print("numpy against torch on the host: %.3g, bar n u ||A||_2 = %.3g" % (diff, GD.eigenvalue_bar(A)))
    assert diff <= GD.eigenvalue_bar(A) <= 1e-13


def test_the_entries_are_declared_and_listed():
    header = " ".join(open(os.path.join(ROOT, "include", "dbcsr_amd_mm.h")).read().split())
    want = {
        "dbcsr_amd_bcsr_to_dense": "void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* m, int kind /* -1, or 0 ... 3: S A H K */, void* dense, "
                                   "int64_t n_rows, int64_t n_cols, int64_t ld, int col_major, void* stream",
        "dbcsr_amd_bcsr_from_dense_apply": "void* handle, libsmm_acc_data_t datatype, const void* dense, int64_t n_rows, int64_t n_cols, int64_t ld, "
                                           "int col_major, dbcsr_amd_bcsr* m, void* stream",
        "dbcsr_amd_bcsr_from_dense_count": "void* handle, libsmm_acc_data_t datatype, const void* dense, int64_t n_rows, int64_t n_cols, int64_t ld, "
                                           "int col_major, const int32_t* row_blk_size, const int32_t* col_blk_size, int nblkrows, int nblkcols, double eps, "
                                           "int32_t* dst_row_p, int32_t* dst_col_i, int64_t* dst_blk_p, int64_t* nblks, int64_t* nze, void* stream",
    }
    assert "Dense conversion" in header
    for name, args in want.items():
        m = re.search(r"int %s\(([^;]*)\);" % name, header)
        assert m and m.group(1) == args, name
        assert name in L.MM_SYMBOLS


def test_the_names_are_exported():
    for name in ("dbcsr_to_dense", "dbcsr_from_dense", "dbcsr_create_from_dense"):
        assert name in dbcsr_amd.__all__ and getattr(dbcsr_amd, name) is getattr(OPS, name)
        assert name + "(" in OPS.__doc__


class Refuses:
    L = property(lambda self: (_ for _ in ()).throw(AssertionError("the library was called")))
    h = None


def host_matrix(dtype=torch.float64):
    """a matrix whose tensors stay on the host: enough for every check that comes before the library"""
    M = GD.matrix("float64")
    t = torch.from_numpy
    return DbcsrMatrix(t(M.row_sizes), t(M.col_sizes), t(M.row_p), t(M.col_i), t(M.blk_p), t(M.data).to(dtype))


def test_refusals_that_need_no_device():
    eng = Refuses()
    dM = host_matrix()
    n_rows, n_cols = GD.full_shape(GD.matrix("float64"))
    good = torch.zeros((n_rows, n_cols), dtype=torch.float64)
    wide = torch.zeros((2 * n_rows, 2 * n_cols), dtype=torch.float64)
    for error, t in [(TypeError, good.numpy()), (TypeError, good.to(torch.float32)), (ValueError, good[:-1]), (ValueError, good.reshape(-1)),
                     (ValueError, wide[::2, ::2]), (ValueError, torch.zeros(n_cols, dtype=torch.float64).expand(n_rows, n_cols)),
                     (ValueError, torch.zeros(n_rows, dtype=torch.float64).expand(n_cols, n_rows).T)]:
        with pytest.raises(error):
            OPS.dbcsr_to_dense(dM, out=t, engine=eng)
        with pytest.raises(error):
            OPS.dbcsr_from_dense(t, dM, engine=eng)
    n = dM.data.numel()
    big = torch.zeros(n + n_rows * n_cols, dtype=torch.float64)
    inside = DbcsrMatrix(dM.row_blk_size, dM.col_blk_size, dM.row_p, dM.col_i, dM.blk_p, big[:n])
    over = torch.as_strided(big, (n_rows, n_cols), (n_cols, 1), n - 1)
    with pytest.raises(ValueError, match="overlap"):
        OPS.dbcsr_to_dense(inside, out=over, engine=eng)
    with pytest.raises(ValueError, match="overlap"):
        OPS.dbcsr_from_dense(over, inside, engine=eng)
    for sym in ("X", "H", "S"):   # unknown; not one of real data; a triangle of a non-square block structure
        dM.symmetry = sym
        with pytest.raises(ValueError):
            OPS.dbcsr_to_dense(dM, engine=eng)
        with pytest.raises(ValueError):
            OPS.dbcsr_from_dense(good, dM, engine=eng)
    with pytest.raises(TypeError):
        OPS.dbcsr_to_dense(host_matrix(torch.int32), engine=eng)
    rs, cs = GD.ROWS, GD.COLS
    for error, args, kw in [(TypeError, (good.numpy(), rs, cs), {}), (TypeError, (good.to(torch.int32), rs, cs), {}), (ValueError, (good.reshape(-1), rs, cs), {}),
                            (ValueError, (good, rs, cs), {"eps": -1.0}), (ValueError, (good, rs, cs), {"eps": float("nan")}),
                            (ValueError, (good, rs, cs), {})]:   # (the last: a tensor on the host)
        with pytest.raises(error):
            OPS.dbcsr_create_from_dense(*args, engine=eng, **kw)


def test_the_two_layouts_are_told_apart():
    f = lambda t: OPS._check_dense("t", t.dtype, t.device, t, t.shape[0], t.shape[1])
    t = torch.zeros((6, 10))
    assert f(t) == (10, 0) and f(t[:, 2:7]) == (10, 0) and f(t.T) == (10, 1) and f(t.T[1:4]) == (10, 1)
    assert f(t[:, 3:4]) == (10, 0) and f(t[2:3]) == (10, 0) and f(torch.zeros((6, 1))) == (1, 0) and f(torch.zeros((1, 6))) == (6, 0)
    assert f(torch.zeros((0, 0)))[0] >= 1 and f(torch.zeros((5, 0)))[0] >= 1 and f(torch.zeros((0, 5)))[0] >= 5
