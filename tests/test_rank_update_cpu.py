"""What tests/test_gpu_rank_update.py measures with, checked without a GPU: the bar of the rank-k update is one that plain double arithmetic meets (so it is
not one only long double can meet) and one that catches an error of 2^-40 w in a single element (so it is not vacuous); the `tiles` matrix is what its
docstring promises; the C entry is declared in the header and listed in lib.MM_SYMBOLS (tests/test_cabi_symbols.py then checks the export)."""
import os
import re

import numpy as np
import pytest

from dbcsr_amd import lib as L
from tests import test_gpu_rank_update as RU
from tests.test_gpu_matrix_norms import base, blocks_of, dense, random_vector, typed  # noqa: F401
from tests.test_gpu_matvec import EPS_LD, U53, scalars
from tests.test_gpu_multivec import random_vectors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def errors(M, got_data, ref, mask):
    G = dense(RU.with_data(M, got_data))
    return np.abs(G.astype(ref.dtype) - ref).astype(np.float64)[mask]


@pytest.mark.parametrize("dtype", RU.DTYPES, ids=RU.IDS)
@pytest.mark.parametrize("which", RU.MATRICES)
def test_double_arithmetic_meets_the_bar_of_case_1(which, dtype):
    """the inputs of test_rank_update: every matrix, type, trans and nrhs, the update formed block by block with np.einsum in float64 / complex128"""
    M, F, absF, mask = RU.host_matrix(which, np.dtype(dtype).name)
    alpha, beta = scalars(dtype)
    for trans in ("T", "C") if RU.is_complex(dtype) else ("T",):   # (real data: the same arithmetic)
        for nrhs in RU.NRHS:
            x, y = RU.inputs(M, nrhs)
            ref, bar = RU.reference(F, absF, alpha, beta, x, y, trans)
            err = errors(M, RU.in_double(M, alpha, beta, x, y, trans), ref, mask)
            assert np.all(err <= bar[mask]), (which, trans, nrhs, float(np.max(err / bar[mask])))


@pytest.mark.parametrize("dtype", [np.float64, np.complex128], ids=["fp64", "z64"])
def test_double_arithmetic_meets_the_bar_of_case_7(dtype):
    """the inputs of test_the_two_halves_agree: sum_pattern a_ij (conj(X) X^T)_ij in float64 / complex128, any order numpy chooses"""
    M = typed(base("square"), dtype, 1)
    x = random_vectors(int(M.row_sizes.sum()), 17, dtype, 71)
    ref, scale, elements = RU.pattern_sum(M, x)
    D = np.complex128 if RU.is_complex(dtype) else np.float64
    mask = RU.parts_of(M)[2]
    got = (dense(M).astype(D) * (x.conj().astype(D) @ x.astype(D).T))[mask].sum()
    assert float(abs(RU.wide(dtype)(got) - ref)) <= (elements + 17 + 12) * U53 * scale
    assert float(abs(ref)) > 1e3 * (elements + 17 + 12) * U53 * scale, "the sum is not lost in its bar"


@pytest.mark.parametrize("dtype", RU.DTYPES, ids=RU.IDS)
def test_an_error_of_2_to_the_minus_40_w_is_caught(dtype):
    M, F, absF, mask = RU.host_matrix("mixed", np.dtype(dtype).name)
    alpha, beta = scalars(dtype)
    for nrhs in (1, 131):
        x, y = RU.inputs(M, nrhs)
        ref, bar = RU.reference(F, absF, alpha, beta, x, y, "C")
        w = abs(alpha) * (np.abs(x).astype(np.float64) @ np.abs(y).astype(np.float64).T) + abs(beta) * absF
        good = RU.in_double(M, alpha, beta, x, y, "C")
        assert np.all(errors(M, good, ref, mask) <= bar[mask])
        if dtype == np.float32:
            continue   # (2^-24 |ref| of the final rounding is above 2^-40 w: float32 data is checked with the larger error below)
        bad = good.copy()
        e = M.data.size // 2
        r, c = np.argwhere(dense(RU.with_data(M, np.arange(1, M.data.size + 1).astype(np.float64))) == e + 1)[0]
        bad[e] += 2.0 ** -40 * w[r, c]
        err = errors(M, bad, ref, mask)
        assert np.sum(err > bar[mask]) == 1, "exactly the one element is caught"
    if dtype == np.float32:
        x, y = RU.inputs(M, 17)
        ref, bar = RU.reference(F, absF, alpha, beta, x, y, "C")
        bad = RU.in_double(M, alpha, beta, x, y, "C")
        e = M.data.size // 2
        bad[e] = np.nextafter(np.nextafter(bad[e], np.float32(np.inf)), np.float32(np.inf))   # two units of float32: one more than the rounding
        assert np.sum(errors(M, bad, ref, mask) > bar[mask]) == 1


def test_the_tiles_matrix_is_what_it_promises():
    M = RU.tiles()
    assert M.row_sizes.tolist() == [16, 32, 33, 80, 16, 32, 33, 80, 16, 32] and np.array_equal(M.row_sizes, M.col_sizes)
    b = blocks_of(M)
    assert abs(len(b) - 50) <= 10, "about half of the hundred blocks"
    shape = {(int(M.row_sizes[r]), int(M.col_sizes[c])) for r, c in b}
    for s in RU.TILE_SIZES:
        assert any(m == s for m, _ in shape) and any(n == s for _, n in shape)
    assert {(80, 80), (16, 16), (32, 32)} <= shape and any(m != n for m, n in shape)
    assert all(np.all(np.diff(M.col_i[M.row_p[r]:M.row_p[r + 1]]) > 0) for r in range(M.nbr)), "ascending block columns in every block row"


def test_the_entry_is_declared_and_listed():
    header = open(os.path.join(ROOT, "include", "dbcsr_amd_mm.h")).read()
    m = re.search(r"int dbcsr_amd_bcsr_rank_update\(([^;]*)\);", header)
    assert m, "include/dbcsr_amd_mm.h declares dbcsr_amd_bcsr_rank_update"
    args = " ".join(m.group(1).split())
    assert args == ("void* handle, libsmm_acc_data_t datatype, char trans, const double alpha[2], int nrhs, const void* x, int64_t n_x, int64_t ldx, "
                    "const void* y, int64_t n_y, int64_t ldy, const double beta[2], dbcsr_amd_bcsr* a, void* stream")
    assert "dbcsr_amd_bcsr_rank_update" in L.MM_SYMBOLS
    for word in ("tile", "band", "group", "persistent", "dma_"):
        assert word not in "dbcsr_amd_bcsr_rank_update"
