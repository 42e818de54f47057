"""What tests/test_gpu_multiply_dense.py measures with, checked without a GPU: every listed count of columns reaches the path it is listed for; the row of X
that carries the NaN / Inf sits directly behind a block whose size is no multiple of 4, and some rows of op(A) store its column and some do not; tall70 /
tall67 have a block row above 64 (the chunk path) and mixed has sizes that are no multiples of 4 or 16; gappy has empty block rows either way; the bar
is one that plain double arithmetic meets; the layout detection of dbcsr_multiply_dense (operations._dense_layouts) on CPU tensors; the C entry is
declared in the header and listed in lib.MM_SYMBOLS (tests/test_cabi_symbols.py then checks the export)."""
import os
import re

import numpy as np
import pytest
import torch

from dbcsr_amd import lib as L
from dbcsr_amd.operations import _dense_layouts
from tests import test_gpu_multiply_dense as MD
from tests.test_gpu_matrix_norms import base
from tests.test_gpu_matvec import host_matrix, op_of, scalars

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_count_of_columns_reaches_its_path():
    assert MD.NCOLS == [1, 3, 16, 17, 64, 70]
    assert MD.paths(1) == (1, 1, 1) and MD.paths(3) == (1, 1, 3), "a partial tile"
    assert MD.paths(16) == (1, 1, 16), "one tile"
    assert MD.paths(17) == (1, 2, 1), "a tile and one column"
    assert MD.paths(64) == (1, 4, 16), "one full workgroup"
    assert MD.paths(70) == (2, 1, 6), "a second workgroup with one partial wave and three that only stage"
    text = open(os.path.join(ROOT, "dbcsr_amd", "csrc", "mm_spmm.h")).read()
    assert re.search(r"kSpmmTile = %d;" % MD.TILE, text) and re.search(r"kSpmmWaves = %d;" % MD.WAVES, text), "the tile and the waves of the kernel"


@pytest.mark.parametrize("trans", ["N", "T"])
def test_the_special_row_sits_behind_a_block_that_is_no_multiple_of_4(trans):
    M = host_matrix("mixed", "float64", "N")[0]
    r, size, hit = MD.special_row(M, trans)
    sizes = M.col_sizes if trans == "N" else M.row_sizes
    offs = np.concatenate([[0], np.cumsum(sizes)])
    assert size % 4 != 0 and size % 16 != 0 and r in offs[1:-1] and sizes[list(offs).index(r) - 1] == size
    assert hit.any() and not hit.all(), "at least one row of Y has that column and at least one lacks it"
    assert np.array_equal(hit, op_of(MD.host_pattern(M), "T" if trans != "N" else "N")[:, r])


def test_the_matrices_reach_the_chunk_and_padding_paths():
    for which in ("tall70", "tall67"):
        M = base(which)
        assert M.row_sizes.max() > 64 and M.col_sizes.max() > 64, "a block row (and a block column) above 64: chunks"
        assert M.row_sizes.max() % 16 != 0
    M = base("mixed")
    assert any(s % 4 for s in M.row_sizes) and any(s % 4 for s in M.col_sizes) and any(s % 16 for s in M.col_sizes)
    G = host_matrix("gappy", "float64", "N")[0]
    for trans in ("N", "T"):
        assert MD.empty_rows(G, trans).size >= 3
    assert set(MD.MATRICES) == {"mixed", "tiny", "tall70", "tall67", "gappy"}


@pytest.mark.parametrize("dtype", MD.DTYPES, ids=MD.IDS)
def test_double_arithmetic_meets_the_bar(dtype):
    """alpha op(F) X + beta Y0 in numpy's float64 / complex128 (float32 data: rounded once at the end) lies within the bar of case 1"""
    for trans in ("N", "T", "C"):
        M, F, _, _ = host_matrix("mixed", np.dtype(dtype).name, "N")
        alpha, beta = scalars(dtype)
        x, y0, ref, bar = MD.inputs("mixed", np.dtype(dtype).name, "N", trans)
        D = np.complex128 if MD.is_complex(dtype) else np.float64
        got = (alpha * (op_of(F.astype(D), trans) @ x.astype(D)) + beta * y0.astype(D)).astype(dtype)
        err = np.abs(got.astype(ref.dtype) - ref).astype(np.float64)
        assert np.all(err <= bar), float(np.max(err / bar))


def test_layout_detection():
    def of(t):
        return _dense_layouts(tuple(t.shape), t.stride())
    n, k = 7, 3
    assert of(torch.zeros(n, k)) == (k, None)
    assert of(torch.zeros(k, n).t()) == (None, n)
    assert of(torch.zeros(n, k + 2)[:, :k]) == (k + 2, None), "a column slice of a wider basis"
    assert of(torch.zeros(k, n + 4)[:, :n].t()) == (None, n + 4), "a window of a Fortran full matrix"
    assert of(torch.zeros(n, 1)) == (1, n), "one column fits both"
    assert of(torch.zeros(1, n).t()) == (1, n)
    assert of(torch.zeros(n, 5)[:, 2:3]) == (5, None), "one column of a row-by-row basis: its rows are 5 apart"
    assert of(torch.zeros(1, k)) == (k, 1), "one row fits both"
    assert of(torch.zeros(n, 2 * k)[:, ::2]) == (None, None)
    assert of(torch.zeros(n * k).as_strided((n, k), (2, 1))) == (None, None), "stride(0) below ncol"
    assert of(torch.zeros(n * k).as_strided((n, k), (1, 2))) == (None, None), "stride(1) below n"
    assert of(torch.zeros(n, 0)) [0] is not None and of(torch.zeros(0, k))[0] is not None


def test_the_entry_is_declared_and_listed():
    header = open(os.path.join(ROOT, "include", "dbcsr_amd_mm.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"int dbcsr_amd_bcsr_multiply_dense\(([^;]*)\);", header)
    assert m, "include/dbcsr_amd_mm.h declares dbcsr_amd_bcsr_multiply_dense"
    args = " ".join(m.group(1).split())
    assert args == ("void* handle, libsmm_acc_data_t datatype, char trans, const double alpha[2], const dbcsr_amd_bcsr* a, int kind , int ncol, "
                    "const void* x, int64_t n_x, int64_t ldx, const double beta[2], void* y, int64_t n_y, int64_t ldy, int layout , void* stream")
    assert "dbcsr_amd_bcsr_multiply_dense" in L.MM_SYMBOLS
