"""What tests/test_gpu_block_inverse.py measures with, checked without a GPU: the bar of the block inverse is one that plain double arithmetic meets --
LAPACK and the Gauss-Jordan elimination restated in numpy, on every input of the GPU file -- with the K that those two measure; it is not vacuous (it is
far below the inverse itself, the restated elimination WITHOUT pivoting misses it on the `permuted` family, and one element disturbed by 2^-40 |x| is
caught); the singular inputs have an exactly zero pivot column and no other input has one; the three C entries are declared in the header and listed in
lib.MM_SYMBOLS (tests/test_cabi_symbols.py then checks the export)."""
import os
import re

import numpy as np
import pytest

from dbcsr_amd import lib as L
from tests import test_gpu_block_inverse as BI
from tests.test_gpu_matrix_norms import blocks_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def in_double(A):
    return A.astype(np.complex128 if BI.is_complex(A.dtype) else np.float64)


def misses(got, A):
    """the elements of an inverse (in A's type) outside their bar"""
    X, w = BI.reference_of(A)
    return np.abs(got.astype(X.dtype) - X).astype(np.float64) > BI.bar_of(A, X, w)


def test_K_is_what_the_inputs_measure():
    k, lapack, restated = BI.measured_K()
    print("worst |got - X| / (n u w): LAPACK %.3f, restated Gauss-Jordan %.3f -> K = %d" % (lapack, restated, k))
    assert k == BI.K


@pytest.mark.parametrize("dtype", BI.DTYPES, ids=BI.IDS)
@pytest.mark.parametrize("family", BI.FAMILIES)
def test_double_arithmetic_meets_the_bar(family, dtype):
    for n in BI.DIMS:
        A = BI.block(family, n, np.dtype(dtype).name)
        for got in (np.linalg.inv(in_double(A)), BI.gauss_jordan(A)[0]):
            assert not np.any(misses(got.astype(A.dtype), A)), (family, n)   # (float32: the double result rounded once)


def test_every_matrix_of_the_gpu_file_takes_its_diagonal_blocks_from_the_input_set():
    known = {BI.block(*key).tobytes() for key in BI.input_set()}
    special = 0
    for dtype in BI.DTYPES:
        name = np.dtype(dtype).name
        matrices = [BI.full_matrix(name), BI.singular_matrix(dtype), BI.diagonal_matrix((5, 13, 23, 32, 33, 40), dtype),
                    BI.diagonal_matrix((5, 13, 23, 32, 33, 40, 17, 16, 3, 2, 31, 64), dtype)] + ([BI.overlap_matrix()] if dtype == np.float64 else [])
        for M in matrices:
            for (r, c), data in blocks_of(M).items():
                if r == c:
                    special += BI.block_of_data(data, int(M.row_sizes[r])).tobytes() not in known
    assert special == 2 * len(BI.DTYPES), "only the two singular blocks of singular_matrix are not of the set"


@pytest.mark.parametrize("dtype", BI.DTYPES, ids=BI.IDS)
def test_the_bar_is_far_below_the_inverse(dtype):
    for family in BI.FAMILIES:
        for n in BI.DIMS:
            X, w = BI.reference_of(BI.block(family, n, np.dtype(dtype).name))
            assert BI.K * n * BI.U53 * np.max(w) <= 2.0 ** -30 * float(np.max(np.abs(X))), (family, n)


@pytest.mark.parametrize("dtype", [np.float64, np.complex128], ids=["fp64", "z64"])
def test_elimination_without_pivoting_misses_the_bar(dtype):
    for n in BI.DIMS:
        if n >= 2:
            A = BI.block("permuted", n, np.dtype(dtype).name)
            got, at = BI.gauss_jordan(A, pivoting=False)
            assert got is None or np.any(misses(got, A)), n
            assert not np.any(misses(BI.gauss_jordan(A)[0], A)), n


@pytest.mark.parametrize("dtype", [np.float64, np.complex128], ids=["fp64", "z64"])
def test_an_error_of_2_to_the_minus_40_is_caught(dtype):
    """One element disturbed by 2^-40 |x_ij| leaves its bar, and only that element: on the element where |x_ij| / w_ij is largest, in the families spd and
    permuted (condition numbers of a few units: K n u w_ij stays below 2^-40 |x_ij| up to n = 96).  In the family general, condition number 10^3, w_ij is
    up to 10^3 |x_ij| and the bar at n = 96 is 4 * 96 * 2^-53 * 10^3 |x_ij| = 2^-34.5 |x_ij|: there the disturbance caught is 2^-30 |x_ij|, the margin of
    test_the_bar_is_far_below_the_inverse."""
    for family in BI.FAMILIES:
        for n in BI.DIMS:
            A = BI.block(family, n, np.dtype(dtype).name)
            X, w = BI.reference_of(A)
            good = BI.gauss_jordan(A)[0]
            i, j = np.unravel_index(np.argmax(np.abs(X).astype(np.float64) / w), w.shape)
            bad = good.copy()
            bad[i, j] += (2.0 ** -30 if family == "general" else 2.0 ** -40) * abs(good[i, j])
            out = misses(bad, A)
            assert out[i, j] and out.sum() == 1, (family, n)


def test_the_float32_bar_catches_two_units():
    for family in BI.FAMILIES:
        for n in BI.DIMS:
            A = BI.block(family, n, "float32")
            good = BI.gauss_jordan(A)[0].astype(np.float32)
            i, j = n // 2, (n * 7) // 10
            bad = good.copy()
            up = np.float32(np.inf) * np.sign(good[i, j])
            bad[i, j] = np.nextafter(np.nextafter(good[i, j], up), up)   # two units of float32: one more than the rounding
            assert misses(bad, A)[i, j] and not np.any(misses(good, A)), (family, n)


@pytest.mark.parametrize("dtype", BI.DTYPES, ids=BI.IDS)
def test_singular_inputs_have_a_zero_pivot_column_and_no_other_input_has(dtype):
    M = BI.singular_matrix(dtype)
    found = {}
    for (r, c), data in blocks_of(M).items():
        got, at = BI.gauss_jordan(BI.block_of_data(data, int(M.row_sizes[r])))
        if got is None:
            found[r] = at
    assert found == {2: 0, 5: 7}
    for key in BI.input_set():
        assert BI.gauss_jordan(BI.block(*key))[1] is None
    nan = np.full((5, 5), np.nan, dtype)
    assert BI.gauss_jordan(nan) == (None, 0), "a NaN never wins: no pivot"


def test_the_entries_are_declared_and_listed():
    header = " ".join(open(os.path.join(ROOT, "include", "dbcsr_amd_mm.h")).read().split())
    want = {
        "dbcsr_amd_bcsr_block_diag_count": "void* handle, const dbcsr_amd_bcsr* m, int32_t* dst_row_p, int32_t* dst_col_i, int64_t* dst_blk_p, "
                                           "int64_t* nblks, int64_t* nze, int32_t* max_dim, void* stream",
        "dbcsr_amd_bcsr_block_diag_apply": "void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* src, dbcsr_amd_bcsr* dst, void* stream",
        "dbcsr_amd_bcsr_block_diag_invert": "void* handle, libsmm_acc_data_t datatype, dbcsr_amd_bcsr* m, int max_dim, int64_t info[3], void* stream",
    }
    assert "Block diagonal" in header
    for name, args in want.items():
        m = re.search(r"int %s\(([^;]*)\);" % name, header)
        assert m and m.group(1) == args, name
        assert name in L.MM_SYMBOLS
