"""What tests/test_gpu_block_scale.py measures with, checked without a GPU: the bars of one pass, of both passes and of the composition are bars that
plain float64 / complex128 block-by-block arithmetic (np.einsum, rounded once per pass) meets on every input of the GPU file -- not bars only long double
can meet; they are not vacuous (an error of 2^-40 w in one element -- float32: two units in the last place -- is caught, and exactly once); the `edge`
matrix is what its docstring promises; the C entry is declared in the header and listed in lib.MM_SYMBOLS (tests/test_cabi_symbols.py then checks the
export); and the refusals that need no device are raised with CPU tensors."""
import os
import re

import numpy as np
import pytest

from dbcsr_amd import lib as L
from tests import test_gpu_block_scale as BS
from tests.test_gpu_matrix_norms import blocks_of, dense, desymmetrized_dense, pattern_mask, symmetric_base, typed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def misses(got_data, M, ref, bar, mask):
    G = dense(BS.with_data(M, got_data))
    return (np.abs(G.astype(ref.dtype) - ref).astype(np.float64) > bar) & mask


@pytest.mark.parametrize("side", ["left", "right"])
@pytest.mark.parametrize("dtype", BS.DTYPES, ids=BS.IDS)
@pytest.mark.parametrize("which", BS.MATRICES)
def test_double_arithmetic_meets_the_bar_of_one_pass(which, dtype, side):
    M, F, mask = BS.host_matrix(which, np.dtype(dtype).name)
    D = BS.diag_for(M, side, dtype)
    alpha = BS.alpha_of(dtype)
    for trans in ("N", "T", "C"):
        ref, bar = BS.reference(F, D, side, trans, alpha, dtype)
        got = BS.in_double(M, D, side, trans, alpha)
        assert not np.any(misses(got, M, ref, bar, mask)), (which, side, trans)
        zero = BS.zeroed_mask(M, D, side)
        assert BS.positive_zero(got[zero]) and np.all(bar[mask][ref[mask] == 0] >= 0)


@pytest.mark.parametrize("dtype", BS.DTYPES, ids=BS.IDS)
@pytest.mark.parametrize("which", ["gappy", "edge"])
def test_double_arithmetic_meets_the_bar_of_both_passes(which, dtype):
    M, F, mask = BS.host_matrix(which, np.dtype(dtype).name)
    D = BS.diag_for(M, "left", dtype)
    alpha = BS.alpha_of(dtype)
    for trans in ("N", "T", "C"):
        T = BS.with_data(M, BS.in_double(M, D, "left", trans, alpha))
        got = BS.in_double(T, D, "right", BS.dagger(trans, dtype), 1.0)
        ref, bar = BS.reference_both(F, D, trans, alpha, dtype)
        assert not np.any(misses(got, M, ref, bar, mask)), (which, trans)


@pytest.mark.parametrize("dtype,symmetry", [(np.float64, "S"), (np.float32, "S"), (np.complex128, "H")], ids=["fp64_S", "fp32_S", "z64_H"])
def test_double_arithmetic_meets_the_bar_of_a_congruence(dtype, symmetry):
    M = typed(symmetric_base(symmetry), np.dtype(dtype), 3)
    D = BS.diag_for(M, "left", dtype)
    full = desymmetrized_dense(M, symmetry).astype(BS.wide(dtype))
    for trans in ("N", "T", "C"):
        T = BS.with_data(M, BS.in_double(M, D, "left", trans, -1.3))
        got = BS.in_double(T, D, "right", BS.dagger(trans, dtype), 1.0)
        ref, bar = BS.reference_both(full, D, trans, -1.3, dtype)
        bar = np.where(pattern_mask(M), bar, bar.T)
        mask = pattern_mask(M, symmetry)
        G = desymmetrized_dense(BS.with_data(M, got), symmetry)
        assert np.all(np.abs(G.astype(ref.dtype) - ref).astype(np.float64)[mask] <= bar[mask]), (symmetry, trans)


def host_inverse(S, dtype):
    """blockdiag(S)^-1 in double (LAPACK), rounded to the data's type: what the device's inverse is within its own bar of"""
    W = np.complex128 if BS.is_complex(dtype) else np.float64
    inv = {}
    for (r, c), v in blocks_of(S).items():
        if r == c:
            n = int(S.row_sizes[r])
            inv[(r, r)] = np.ascontiguousarray(np.linalg.inv(v.astype(W).reshape(n, n).T).T).reshape(-1).astype(dtype)
    from tests.test_gpu_matrix_norms import from_blocks
    return from_blocks(S.row_sizes, S.col_sizes, inv, np.dtype(dtype))


@pytest.mark.parametrize("dtype", BS.DTYPES, ids=BS.IDS)
def test_double_arithmetic_meets_the_composition(dtype):
    """blockdiag(S)^-1 S in plain double from a LAPACK inverse: within the bar, and its diagonal blocks within identity_margin of the identity"""
    S = BS.spd_matrix(np.dtype(dtype).name)
    D = host_inverse(S, dtype)
    got = BS.in_double(S, D, "left", "N", 1.0)
    ref, bar = BS.reference(dense(S).astype(BS.wide(dtype)), D, "left", "N", 1.0, dtype)
    assert not np.any(misses(got, S, ref, bar, pattern_mask(S)))
    worst = 0.0
    for (r, c), v in blocks_of(BS.with_data(S, got)).items():
        if r == c:
            n = int(S.row_sizes[r])
            q = float(np.max(np.abs(v.reshape(n, n).T - np.eye(n)))) / BS.identity_margin(n, dtype)
            worst = max(worst, q)
    print("diagonal blocks of D^-1 S: worst distance from the identity / margin = %.3g" % worst)
    assert worst <= 0.5, "plain double keeps half the margin free for the device's inverse"


@pytest.mark.parametrize("side", ["left", "right"])
@pytest.mark.parametrize("dtype", BS.DTYPES, ids=BS.IDS)
def test_a_small_error_in_one_element_is_caught_once(dtype, side):
    M, F, mask = BS.host_matrix("edge", np.dtype(dtype).name)
    D = BS.diag_for(M, side, dtype)
    alpha = BS.alpha_of(dtype)
    ref, bar = BS.reference(F, D, side, "N", alpha, dtype)
    good = BS.in_double(M, D, side, "N", alpha)
    B, absB, dims = BS.blockdiag_dense(D, "N")
    off = np.concatenate([[0], np.cumsum(D.row_sizes)])
    w = abs(alpha) * BS.block_product(absB, np.abs(F).astype(np.float64), off, side == "left")
    rows = M.rows()
    have = blocks_of(D)
    b = next(b for b in range(M.nblks) if ((int(rows[b]),) * 2 if side == "left" else (int(M.col_i[b]),) * 2) in have and M.row_sizes[rows[b]] == 96)
    e = M.blk_p[b] + 5
    at = np.zeros(M.data.size)
    at[e] = 1
    i, j = map(int, np.argwhere(dense(BS.with_data(M, at)) != 0)[0])
    bad = good.copy()
    if np.dtype(dtype) == np.float32:
        up = np.float32(np.inf) * np.sign(good[e])
        bad[e] = np.nextafter(np.nextafter(good[e], up), up)
    else:
        bad[e] += 2.0 ** -40 * w[i, j]
    out = misses(bad, M, ref, bar, mask)
    assert out[i, j] and out.sum() == 1 and not np.any(misses(good, M, ref, bar, mask))


def test_the_edge_matrix_is_what_it_promises():
    M = BS.edge()
    b = blocks_of(M)
    assert sorted(set(M.row_sizes.tolist())) == sorted(BS.EDGE_SIZES) and np.array_equal(M.row_sizes, M.col_sizes)
    for n in BS.EDGE_SIZES:
        assert any(M.row_sizes[r] == n for r, c in b) and any(M.col_sizes[c] == n for r, c in b), n
    assert any(M.row_sizes[r] == 96 and M.col_sizes[c] == 96 for r, c in b), "a 96 x 96 block is stored"
    assert any(M.row_sizes[r] != M.col_sizes[c] for r, c in b), "rectangular blocks are stored"
    for side in ("left", "right"):
        D = BS.diag_for(M, side, np.float64)
        zero = BS.zeroed_mask(M, D, side)
        assert zero.any() and not zero.all() and any(r != c for r, c in blocks_of(D))


def test_the_entry_is_declared_and_listed():
    header = open(os.path.join(ROOT, "include", "dbcsr_amd_mm.h")).read()
    assert "Block diagonal times matrix" in header
    header = " ".join(re.sub(r"/\*.*?\*/", "", header).split())   # (the declaration carries a comment on `side`)
    m = re.search(r"int dbcsr_amd_bcsr_block_diag_multiply\(([^;]*)\);", header)
    assert m and m.group(1).replace(" ,", ",") == ("void* handle, libsmm_acc_data_t datatype, char side, char trans, const double alpha[2], "
                                                   "const dbcsr_amd_bcsr* diag, dbcsr_amd_bcsr* m, int max_dim, void* stream")
    assert "dbcsr_amd_bcsr_block_diag_multiply" in L.MM_SYMBOLS


def test_refusals_need_no_device():
    class Engine:
        L = BS.Refuses()
        h = None

    BS.check_refusals(Engine(), "cpu")
