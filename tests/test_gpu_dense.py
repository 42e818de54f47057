"""Dense <-> block-sparse on the device (dbcsr_amd/operations.py: dbcsr_to_dense, dbcsr_from_dense, dbcsr_create_from_dense; the "Dense conversion" entries
of include/dbcsr_amd_mm.h; kernels of dbcsr_amd/csrc/mm_dense.h) for float64, float32 and complex128.

Everything is a copy, so everything is compared BIT FOR BIT with the host helpers: oracle.Bcsr.to_dense (through `dense`, which serves complex data too),
desymmetrized_dense, from_dense, from_blocks, blocks_of and subset of tests/test_gpu_matrix_norms.py.  No tolerance anywhere but in the eigenvalue
workflow, whose bar is stated there.

One remark on the stored triangles: desymmetrized_dense ADDS the mirrored part to the stored one, which turns every -0.0 into +0.0; the device flips sign
bits (the reading of dbcsr_amd_bcsr_desymmetrized: exact, an involution), so the twin of +0.0 under 'A' / 'K' is -0.0.  The matrices compared with
desymmetrized_dense hold no zero element -- there both readings give the same bits, the +0.0 of everything that is not stored included -- and
test_to_dense_of_a_triangle_flips_sign_bits checks the zeros against the sign-flip reading written out in numpy.

Matrices: 10 x 8 block rows / columns with the row sizes 5 13 1 23 32 33 40 64 1 5 and the column sizes 23 1 96 5 33 13 40 32 -- the sizes 1, 5, 13, 23,
32, 33, 40, 64 and 96, rectangular blocks, a non-square block structure, blocks of 1 x 1 (every alignment of the blocks behind them), blocks above 32 and above 64 in either
direction (several tiles, the per-column pieces of the transposing moves), block rows 2 and 8 without blocks; for the stored triangles 9 x 9 with the
sizes 5 13 1 23 32 33 40 64 1."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from dbcsr_amd import lib as L
from dbcsr_amd.matrix import DbcsrMatrix, StreamHandle
from dbcsr_amd.multiply import MultiplyEngine, dbcsr_multiply
from dbcsr_amd.operations import dbcsr_create_from_dense, dbcsr_from_dense, dbcsr_to_dense
from oracle import oracle as O
from tests.gpu_util import dev_to_bcsr, to_dev
from tests.test_gpu_matrix_norms import (TORCH, blocks_of, dense, desymmetrized_dense, from_blocks, from_dense, is_complex, misaligned, same_bits, subset,
                                         with_holes)

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32, np.complex128]
IDS = ["fp64", "fp32", "z64"]
LAYOUTS = ["rows", "cols"]
ROWS = np.asarray([5, 13, 1, 23, 32, 33, 40, 64, 1, 5], np.int32)
COLS = np.asarray([23, 1, 96, 5, 33, 13, 40, 32], np.int32)
SQUARE = np.asarray([5, 13, 1, 23, 32, 33, 40, 64, 1], np.int32)
EMPTY_ROWS = (2, 8)
ALWAYS = {(7, 2), (6, 4), (4, 7), (3, 0), (0, 1), (5, 2)}   # 64 x 96, 40 x 33, 32 x 32, 23 x 23, 5 x 1, 33 x 96: stored in every general matrix
EPS = 1e-3


@pytest.fixture(scope="module")
def eng():
    return MultiplyEngine()


# ---- host inputs (no GPU needed: tests/test_dense_cpu.py checks them) -----------------------------------------------------------------------------------
def random_values(rng, n, dtype):
    x = rng.uniform(-1.0, 1.0, n)
    if is_complex(dtype):
        x = x + 1j * rng.uniform(-1.0, 1.0, n)
    return x.astype(dtype)


@functools.lru_cache(maxsize=None)
def matrix(dtype_name, which="general", zeros=True):
    """general: 10 x 8 blocks, about half of them stored, block rows 2 and 8 empty, a few exact zeros of both signs in the blocks of at least four elements;
    triangle: 9 x 9, blocks with row <= column, about 60 % of them, some diagonal blocks missing, no zero element (zeros=True: zeros of both signs)"""
    dtype = np.dtype(dtype_name)
    rng = np.random.default_rng(11 if which == "general" else 12)
    rs, cs = (ROWS, COLS) if which == "general" else (SQUARE, SQUARE)
    blocks = {}
    for r in range(len(rs)):
        for c in range(len(cs)):
            if which == "general":
                stored = r not in EMPTY_ROWS and (rng.random() < 0.55 or (r, c) in ALWAYS)
            else:
                stored = c >= r and rng.random() < 0.6 and r != 2
            if not stored:
                continue
            v = random_values(rng, int(rs[r]) * int(cs[c]), dtype)
            if v.size >= 4 and (which == "general" or zeros):
                v[1], v[v.size - 2] = 0.0, (0.0 if is_complex(dtype) else -0.0)   # (the helper `dense` sums re + 1j * im: no -0.0 in complex data)
            blocks[(r, c)] = v
    M = from_blocks(rs, cs, blocks, dtype)
    if which == "general":
        assert all(M.row_p[r] == M.row_p[r + 1] for r in EMPTY_ROWS) and 25 <= M.nblks <= 50 and ALWAYS <= set(blocks)
    else:
        assert 0 < sum(1 for r, c in blocks if r == c) < len(rs) and any(c > r for r, c in blocks)
    return M


def full_shape(M):
    return int(M.row_sizes.sum()), int(M.col_sizes.sum())


def twin_dense(M, symmetry):
    """the full matrix of a stored triangle by the sign-flip reading: tile (c, r) = the transpose of block (r, c), conjugated for 'H' / 'K' (the imaginary
    part's sign bit flipped), negated for 'A' / 'K' (every sign bit flipped); stored blocks as they are"""
    D = dense(M)
    ro = np.concatenate([[0], np.cumsum(M.row_sizes)])
    for (r, c), v in blocks_of(M).items():
        if r == c:
            continue
        T = v.reshape(int(M.col_sizes[c]), int(M.row_sizes[r])).copy()   # [j][i] of the block = the transposed block, row by row
        if symmetry in ("H", "K"):
            T = np.conj(T)
        if symmetry in ("A", "K"):
            T = -T
        D[ro[c]:ro[c + 1], ro[r]:ro[r + 1]] = T
    return D


@functools.lru_cache(maxsize=None)
def eps_case(dtype_name):
    """(dense matrix over ROWS x COLS, keep[r, c]) for create_from_dense with EPS: every tile is either large (every |x| >= 0.5: norm >= 0.5), small (the
    large values times 1e-6: norm <= sqrt(96 * 64) * 1.5e-6 < EPS / 2), exactly zero, or -- tile (3, 2) -- small with one NaN, which stays"""
    dtype = np.dtype(dtype_name)
    rng = np.random.default_rng(13)
    n_rows, n_cols = int(ROWS.sum()), int(COLS.sum())
    x = random_values(rng, n_rows * n_cols, dtype).reshape(n_rows, n_cols)
    D = (np.sign(x.real) * (0.5 + 0.5 * np.abs(x.real)) + (1j * x.imag if is_complex(dtype) else 0)).astype(dtype)
    ro, co = np.concatenate([[0], np.cumsum(ROWS)]), np.concatenate([[0], np.cumsum(COLS)])
    keep = np.zeros((len(ROWS), len(COLS)), bool)
    for r in range(len(ROWS)):
        for c in range(len(COLS)):
            kind = rng.integers(0, 3) if r not in EMPTY_ROWS else 2
            tile = D[ro[r]:ro[r + 1], co[c]:co[c + 1]]
            if (r, c) == (3, 2):
                tile *= 1e-6
                tile[7, 50] = np.nan
                keep[r, c] = True
            elif kind == 0:
                keep[r, c] = True
            elif kind == 1:
                tile *= 1e-6
            else:
                tile[...] = 0
    return D, keep


def tile_norms(D, rs, cs):
    ro, co = np.concatenate([[0], np.cumsum(rs)]), np.concatenate([[0], np.cumsum(cs)])
    return np.asarray([[np.sqrt(np.sum(np.abs(D[ro[r]:ro[r + 1], co[c]:co[c + 1]].astype(np.complex128)) ** 2)) for c in range(len(cs))]
                       for r in range(len(rs))])


def filtered_host(D, rs, cs, eps):
    """what from_dense + subset give under the filter's rule: a tile is dropped iff its squared norm is below eps^2"""
    n2 = tile_norms(D, rs, cs) ** 2
    return subset(from_dense(D, rs, cs, D.dtype), lambda r, c: not (n2[r, c] < eps * eps))


@functools.lru_cache(maxsize=None)
def spd_case():
    """a small SPD matrix over SQUARE as a stored triangle 'S' with every block of the upper triangle, and its dense form"""
    rng = np.random.default_rng(5)
    n = int(SQUARE.sum())
    X = rng.uniform(-1.0, 1.0, (n, n))
    A = X @ X.T / n + np.eye(n)
    A = (A + A.T) / 2
    return subset(from_dense(A, SQUARE, SQUARE, np.float64), lambda r, c: r <= c), A


def eigenvalue_bar(A):
    """|computed - exact| <= n u ||A||_2 is what a backward-stable symmetric eigensolver promises up to a modest constant; two such solvers differ by at most
    twice that.  On the host, numpy and torch (both LAPACK) differ by 7.1e-15 on spd_case() -- 0.13 of this bar of 5.4e-14 (tests/test_dense_cpu.py
    measures it); nothing here is measured on the kernels, whose output is checked bit for bit before the solver sees it."""
    return A.shape[0] * 2.0 ** -53 * float(np.linalg.norm(A, 2))


# ---- device helpers ----------------------------------------------------------------------------------------------------------------------------------------
def nan_of(dtype):
    return complex(np.nan, np.nan) if is_complex(dtype) else np.nan


def on_device(D, layout):
    t = torch.from_numpy(np.ascontiguousarray(D)).cuda()
    return t if layout == "rows" else t.T.contiguous().T


def nan_out(shape, dtype, layout):
    td = TORCH[np.dtype(dtype)]
    if layout == "rows":
        return torch.full(shape, nan_of(dtype), dtype=td, device="cuda")
    return torch.full((shape[1], shape[0]), nan_of(dtype), dtype=td, device="cuda").T


def host(t):
    return t.cpu().numpy()


def window_in(buf, shape, ld, layout):
    """a window of `shape` one element and one guard row (column) into the 1-D storage buf, with row (column) stride ld"""
    major = shape[0] if layout == "rows" else shape[1]
    v = torch.as_strided(buf, (major, ld), (ld, 1), 1 + ld)
    return v[:, :shape[1]] if layout == "rows" else v[:, :shape[0]].T


def expected_area(M, area, D):
    """the data area after from_dense: the blocks M names hold D's elements, everything else what `area` held"""
    out = area.copy()
    ro, co = np.concatenate([[0], np.cumsum(M.row_sizes)]), np.concatenate([[0], np.cumsum(M.col_sizes)])
    rows = M.rows()
    for b in range(M.nblks):
        r, c = int(rows[b]), int(M.col_i[b])
        blk = D[ro[r]:ro[r + 1], co[c]:co[c + 1]].T.reshape(-1)
        out[M.blk_p[b]:M.blk_p[b] + blk.size] = blk
    return out


# ---- 1. to_dense, no symmetry --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_to_dense_allocates_and_fills(eng, dtype):
    M = matrix(np.dtype(dtype).name)
    dM = to_dev(M)
    stamp = dM.index_stamp()
    ref = dense(M)
    got = dbcsr_to_dense(dM, engine=eng)
    assert got.is_contiguous() and got.dtype == TORCH[np.dtype(dtype)] and tuple(got.shape) == full_shape(M)
    assert same_bits(host(got), ref)
    for layout in LAYOUTS:
        out = nan_out(full_shape(M), dtype, layout)
        assert dbcsr_to_dense(dM, out=out, engine=eng) is out
        assert same_bits(host(out), ref), layout
        assert same_bits(host(dbcsr_to_dense(dM, out=out, engine=eng)), ref), "the same bits on every call"
    assert dM.index_stamp() == stamp and same_bits(host(dM.data), M.data)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_to_dense_writes_the_window_and_nothing_else(eng, dtype, layout):
    M = matrix(np.dtype(dtype).name)
    n_rows, n_cols = full_shape(M)
    minor, major = (n_cols, n_rows) if layout == "rows" else (n_rows, n_cols)
    ld = minor + 5
    buf = torch.full(((major + 2) * ld + 1,), nan_of(dtype), dtype=TORCH[np.dtype(dtype)], device="cuda")
    before = host(buf).copy()
    out = window_in(buf, (n_rows, n_cols), ld, layout)
    assert out.storage_offset() == 1 + ld and out.stride() == ((ld, 1) if layout == "rows" else (1, ld))
    dbcsr_to_dense(to_dev(M), out=out, engine=eng)
    assert same_bits(host(out), dense(M))
    after = host(buf).copy()
    inside = np.zeros(after.size, bool)
    inside[1 + ld:1 + ld + major * ld].reshape(major, ld)[:, :minor] = True
    assert inside.sum() == n_rows * n_cols
    assert same_bits(after[~inside], before[~inside]), "the padding and the guard rows keep their NaN bits"


# ---- 2. to_dense of a stored triangle ------------------------------------------------------------------------------------------------------------------------
TRIANGLES = [("S", np.float64), ("A", np.float64), ("S", np.float32), ("A", np.float32), ("H", np.complex128), ("K", np.complex128)]


@pytest.mark.parametrize("symmetry,dtype", TRIANGLES, ids=["%s-%s" % (s, np.dtype(d).name) for s, d in TRIANGLES])
def test_to_dense_of_a_stored_triangle(eng, symmetry, dtype):
    M = matrix(np.dtype(dtype).name, "triangle", zeros=False)
    assert not np.any(M.data == 0)
    ref = desymmetrized_dense(M, symmetry)
    assert same_bits(ref, twin_dense(M, symmetry)), "without zeros in the data both readings agree"
    dM = to_dev(M)
    dM.symmetry = symmetry
    assert same_bits(host(dbcsr_to_dense(dM, engine=eng)), ref)
    for layout in LAYOUTS:
        out = nan_out(full_shape(M), dtype, layout)
        dbcsr_to_dense(dM, out=out, engine=eng)
        assert same_bits(host(out), ref), layout
    assert same_bits(host(dM.data), M.data)


@pytest.mark.parametrize("symmetry,dtype", TRIANGLES, ids=["%s-%s" % (s, np.dtype(d).name) for s, d in TRIANGLES])
def test_to_dense_of_a_triangle_flips_sign_bits(eng, symmetry, dtype):
    M = matrix(np.dtype(dtype).name, "triangle", zeros=True)
    assert np.any(M.data == 0)
    ref = twin_dense(M, symmetry)
    assert np.array_equal(ref, desymmetrized_dense(M, symmetry)), "the values are those of the helper; only signs of zeros differ"
    dM = to_dev(M)
    dM.symmetry = symmetry
    for layout in LAYOUTS:
        out = nan_out(full_shape(M), dtype, layout)
        dbcsr_to_dense(dM, out=out, engine=eng)
        assert same_bits(host(out), ref), layout


def test_to_dense_of_a_triangle_with_blocks_below_the_diagonal(eng):
    """any mix of upper and lower blocks, one per pair: the place that is stored is looked up first, then the mirrored one"""
    U = matrix("float64", "triangle", zeros=False)
    moved = {}
    for (r, c), v in blocks_of(U).items():
        if c > r and (r + c) % 2:
            moved[(c, r)] = v.reshape(int(SQUARE[c]), int(SQUARE[r])).T.reshape(-1)   # the transposed block, stored at the mirrored place
        else:
            moved[(r, c)] = v
    M = from_blocks(SQUARE, SQUARE, moved, np.float64)
    assert any(r > c for r, c in moved) and any(r < c for r, c in moved)
    dM = to_dev(M)
    dM.symmetry = "S"
    assert same_bits(host(dbcsr_to_dense(dM, engine=eng)), desymmetrized_dense(U, "S"))


# ---- 3. holes, alignment, empty matrices ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_to_dense_of_unpacked_and_misaligned_matrices(eng, dtype):
    M = matrix(np.dtype(dtype).name)
    hB, dB = with_holes(eng, M, dtype)
    for dX, hX in ((dB, hB), (misaligned(to_dev(M)), M)):
        area = dX.data.clone()
        for layout in LAYOUTS:
            out = nan_out(full_shape(M), dtype, layout)
            dbcsr_to_dense(dX, out=out, engine=eng)
            assert same_bits(host(out), dense(hX)), layout
        assert same_bits(host(dX.data), host(area)), "the source keeps its bits"
    assert same_bits(dense(hB), dense(M))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_empty_matrices(eng, dtype):
    td = TORCH[np.dtype(dtype)]
    E = to_dev(subset(matrix(np.dtype(dtype).name), lambda r, c: False))
    got = dbcsr_to_dense(E, engine=eng)
    assert same_bits(host(got), np.zeros(full_shape(matrix(np.dtype(dtype).name)), dtype)) and not np.any(np.signbit(host(got).real))
    dbcsr_from_dense(got, E, engine=eng)
    none = np.zeros(0, np.int32)
    Z = to_dev(from_blocks(none, none, {}, dtype))
    assert tuple(dbcsr_to_dense(Z, engine=eng).shape) == (0, 0)
    dbcsr_from_dense(torch.zeros((0, 0), dtype=td, device="cuda"), Z, engine=eng)
    W = to_dev(from_blocks(ROWS, none, {}, dtype))
    assert tuple(dbcsr_to_dense(W, engine=eng).shape) == (int(ROWS.sum()), 0)
    C0 = dbcsr_create_from_dense(torch.zeros((0, 0), dtype=td, device="cuda"), none, none, engine=eng)
    assert C0.nblks == 0 and host(C0.row_p).tolist() == [0]


# ---- 4. from_dense onto a pattern ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_from_dense_writes_the_stored_blocks_and_nothing_else(eng, dtype, layout):
    M = matrix(np.dtype(dtype).name)
    rng = np.random.default_rng(21)
    n_rows, n_cols = full_shape(M)
    D = random_values(rng, n_rows * n_cols, dtype).reshape(n_rows, n_cols)
    outside = dense(from_blocks(M.row_sizes, M.col_sizes, {k: np.ones(v.size) for k, v in blocks_of(M).items()}, np.float64)) == 0
    D2 = D.copy()
    D2[outside] = random_values(rng, int(outside.sum()), dtype)
    assert outside.any() and not same_bits(D, D2)
    hB, dB = with_holes(eng, M, dtype)
    for hX, dX in ((M, to_dev(M)), (hB, dB)):
        # the data area one element into a tensor of NaN: guard elements in front of and behind it
        n = dX.data.numel()
        big = torch.full((n + 3,), nan_of(dtype), dtype=dX.data.dtype, device="cuda")
        big[1:1 + n].copy_(dX.data)
        dG = DbcsrMatrix(dX.row_blk_size, dX.col_blk_size, dX.row_p, dX.col_i, dX.blk_p, big[1:1 + n], nze=dX.nze)
        before = host(big).copy()
        stamp, tensors = dG.index_stamp(), (dG.row_p, dG.col_i, dG.blk_p, dG.data)
        assert dbcsr_from_dense(on_device(D, layout), dG, engine=eng) is dG
        want = before.copy()
        want[1:1 + n] = expected_area(hX, before[1:1 + n], D)
        got = host(big).copy()
        assert same_bits(got, want), "stored blocks = the dense elements; holes and guard elements keep their bits"
        assert dG.index_stamp() == stamp and all(a is b for a, b in zip(tensors, (dG.row_p, dG.col_i, dG.blk_p, dG.data)))
        assert same_bits(host(dG.row_p), hX.row_p) and same_bits(host(dG.col_i), hX.col_i) and same_bits(host(dG.blk_p), hX.blk_p)
        big[1:1 + n].copy_(dX.data)
        dbcsr_from_dense(on_device(D2, layout), dG, engine=eng)
        assert same_bits(host(big), got), "a dense matrix that differs outside the pattern gives the same data area"


@pytest.mark.parametrize("symmetry,dtype", [("S", np.float64), ("A", np.float32), ("H", np.complex128)], ids=["S-fp64", "A-fp32", "H-z64"])
def test_from_dense_of_a_stored_triangle_reads_the_stored_side_only(eng, symmetry, dtype):
    M = matrix(np.dtype(dtype).name, "triangle", zeros=False)
    n = int(SQUARE.sum())
    D = random_values(np.random.default_rng(22), n * n, dtype).reshape(n, n)
    ro = np.concatenate([[0], np.cumsum(SQUARE)])
    for r in range(len(SQUARE)):
        D[ro[r]:ro[r + 1], :ro[r]] = nan_of(dtype)   # every tile below the block diagonal
    dM = to_dev(M)
    dM.symmetry = symmetry
    for layout in LAYOUTS:
        dM.data.zero_()
        dbcsr_from_dense(on_device(D, layout), dM, engine=eng)
        got = host(dM.data)
        assert not np.any(np.isnan(got)) and same_bits(got, expected_area(M, np.zeros_like(M.data), D)), layout


# ---- 5. round trips ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_round_trips(eng, dtype):
    M = matrix(np.dtype(dtype).name)
    dM = to_dev(M)
    for layout in LAYOUTS:
        out = nan_out(full_shape(M), dtype, layout)
        dbcsr_to_dense(dM, out=out, engine=eng)
        dM.data.fill_(nan_of(dtype))
        dbcsr_from_dense(out, dM, engine=eng)
        assert same_bits(host(dM.data), M.data), layout
    D = eps_case(np.dtype(dtype).name)[0]
    D = np.where(np.isnan(D), 1.0, D).astype(dtype)
    for layout in LAYOUTS:
        dC = dbcsr_create_from_dense(on_device(D, layout), ROWS, COLS, engine=eng)
        assert dC.nblks == len(ROWS) * len(COLS) and dC.packed and dC.symmetry == "N"
        assert same_bits(host(dbcsr_to_dense(dC, engine=eng)), D), layout


# ---- 6. create_from_dense under the filter ------------------------------------------------------------------------------------------------------------------------
def same_matrix(dC, H):
    G = dev_to_bcsr(dC)
    return (same_bits(G.row_p, H.row_p) and same_bits(G.col_i, H.col_i) and same_bits(G.blk_p, H.blk_p) and same_bits(G.data, H.data) and
            same_bits(G.row_sizes, H.row_sizes) and same_bits(G.col_sizes, H.col_sizes))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_create_from_dense_keeps_what_the_filter_keeps(eng, dtype, layout):
    D, keep = eps_case(np.dtype(dtype).name)
    H = filtered_host(D, ROWS, COLS, EPS)
    assert set(blocks_of(H)) == {(r, c) for r in range(len(ROWS)) for c in range(len(COLS)) if keep[r, c]} and (3, 2) in blocks_of(H)
    dD = on_device(D, layout)
    rs, cs = torch.from_numpy(ROWS).cuda(), torch.from_numpy(COLS).cuda()
    dC = dbcsr_create_from_dense(dD, rs, cs, eps=EPS, name="from dense", engine=eng)
    assert dC.row_blk_size is rs and dC.col_blk_size is cs and dC.name == "from dense" and dC.packed
    assert same_matrix(dC, H), "the index and the blocks of from_dense + subset; the block with a NaN stays"
    assert same_matrix(dbcsr_create_from_dense(dD, rs, cs, eps=EPS, engine=eng), H), "the same bits on every call"
    full = dbcsr_create_from_dense(dD, ROWS.tolist(), COLS.tolist(), eps=0.0, engine=eng)
    assert same_matrix(full, from_dense(D, ROWS, COLS, np.dtype(dtype))), "eps = 0 keeps every block"
    zero = dbcsr_create_from_dense(torch.zeros_like(dD), rs, cs, eps=EPS, engine=eng)
    assert zero.nblks == 0 and zero.data.numel() == 0 and not host(zero.row_p).any()
    assert dbcsr_create_from_dense(torch.zeros_like(dD), rs, cs, engine=eng).nblks == len(ROWS) * len(COLS)


# ---- 7. offsets beyond 2^31 -------------------------------------------------------------------------------------------------------------------------------------
def test_row_offsets_beyond_2_to_the_31(eng):
    """float32, 19 rows (blocks 5, 13, 1), a row-by-row window with ld = 2^27 + 3: rows 16 ... 18 start beyond 2^31 elements.  About 10 GB are allocated and
    only the window is touched."""
    rs, cs = np.asarray([5, 13, 1], np.int32), np.asarray([23, 1, 5, 33], np.int32)
    ld = 2 ** 27 + 3
    n_rows, n_cols = int(rs.sum()), int(cs.sum())
    try:
        buf = torch.empty(n_rows * ld, dtype=torch.float32, device="cuda")
    except (RuntimeError, MemoryError) as e:
        pytest.skip("no room for the 10 GB tensor: %s" % str(e).splitlines()[0])
    assert (n_rows - 1) * ld > 2 ** 31
    rng = np.random.default_rng(31)
    blocks = {(r, c): random_values(rng, int(rs[r]) * int(cs[c]), np.float32) for r in range(3) for c in range(4) if (r, c) not in ((0, 1), (2, 2))}
    M = from_blocks(rs, cs, blocks, np.float32)
    dM = to_dev(M)
    out = torch.as_strided(buf, (n_rows, n_cols), (ld, 1))
    out.fill_(np.nan)
    dbcsr_to_dense(dM, out=out, engine=eng)
    assert same_bits(host(out), dense(M))
    D = random_values(rng, n_rows * n_cols, np.float32).reshape(n_rows, n_cols)
    out.copy_(torch.from_numpy(D).cuda())
    dbcsr_from_dense(out, dM, engine=eng)
    assert same_bits(host(dM.data), expected_area(M, M.data, D))
    assert same_matrix(dbcsr_create_from_dense(out, rs, cs, eps=0.0, engine=eng), from_dense(D, rs, cs, np.dtype(np.float32)))
    del out, buf
    torch.cuda.empty_cache()


# ---- 8. between two multiplies --------------------------------------------------------------------------------------------------------------------------------
def test_dense_conversion_between_multiplies_keeps_the_plan(monkeypatch):
    monkeypatch.delenv("DBCSR_AMD_MM_PLAN", raising=False)
    eng = MultiplyEngine()
    rng = np.random.default_rng(41)
    A = matrix("float64", "triangle", zeros=False)   # (taken as a matrix without symmetry: an upper block triangle)
    B = from_blocks(SQUARE, SQUARE, {(r, c): random_values(rng, int(SQUARE[r]) * int(SQUARE[c]), np.float64)
                                     for r in range(9) for c in range(9) if (r + 2 * c) % 3}, np.float64)
    dA, dB = to_dev(A), to_dev(B)
    dC = to_dev(subset(A, lambda r, c: False))
    dbcsr_multiply("N", "N", 1.0, dA, dB, 0.0, dC, engine=eng)
    assert eng.plan_stats() == (0, 1)
    torch.cuda.synchronize()
    first = dev_to_bcsr(dC)
    tensors = [(m.row_p, m.col_i, m.blk_p, m.data) for m in (dA, dC)]
    stamps = (dA.index_stamp(), dC.index_stamp())
    D = dbcsr_to_dense(dA, engine=eng)
    dA.data.fill_(np.nan)
    dbcsr_from_dense(D, dA, engine=eng)
    dbcsr_to_dense(dC, engine=eng)   # (of its result, too)
    assert (dA.index_stamp(), dC.index_stamp()) == stamps
    assert all(a is b for m, t in zip((dA, dC), tensors) for a, b in zip((m.row_p, m.col_i, m.blk_p, m.data), t))
    dbcsr_multiply("N", "N", 1.0, dA, dB, 0.0, dC, engine=eng)
    assert eng.plan_stats() == (1, 1), "a multiply after a dense conversion must reuse its plan"
    torch.cuda.synchronize()
    assert same_bits(host(dA.data), A.data)
    again = dev_to_bcsr(dC)
    assert same_bits(again.col_i, first.col_i) and same_bits(again.blk_p, first.blk_p) and same_bits(again.data, first.data)


# ---- 9. a workflow ------------------------------------------------------------------------------------------------------------------------------------------------
def test_eigenvalues_of_a_stored_triangle(eng):
    M, A = spd_case()
    dS = to_dev(M)
    dS.symmetry = "S"
    D = dbcsr_to_dense(dS, engine=eng)
    assert same_bits(host(D), A) and same_bits(desymmetrized_dense(M, "S"), A)
    got = host(torch.linalg.eigvalsh(D))
    ref = np.linalg.eigvalsh(A)
    print("eigenvalues: max |torch on the device - numpy| = %.3g, bar %.3g" % (np.max(np.abs(got - ref)), 2 * eigenvalue_bar(A)))
    assert np.max(np.abs(got - ref)) <= 2 * eigenvalue_bar(A)


# ---- 10. refusals -----------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_call(monkeypatch):
    class Refuses:
        def __getattr__(self, name):
            raise AssertionError("the library was called (%s)" % name)

    eng = MultiplyEngine()
    monkeypatch.setattr(eng, "L", Refuses())
    M = matrix("float64")
    n_rows, n_cols = full_shape(M)
    dM = to_dev(M)
    good = torch.zeros((n_rows, n_cols), dtype=torch.float64, device="cuda")
    wide = torch.zeros((2 * n_rows, 2 * n_cols), dtype=torch.float64, device="cuda")
    # the matrix' data area inside a larger tensor, and a window over the same storage
    n = dM.data.numel()
    big = torch.zeros(n + n_rows * n_cols, dtype=torch.float64, device="cuda")
    inside = DbcsrMatrix(dM.row_blk_size, dM.col_blk_size, dM.row_p, dM.col_i, dM.blk_p, big[:n])
    over = torch.as_strided(big, (n_rows, n_cols), (n_cols, 1), n - 1)
    bad = [
        (TypeError, np.zeros((n_rows, n_cols))),                                              # not a tensor
        (TypeError, good.to(torch.float32)),                                                  # wrong data type
        (ValueError, good.cpu()),                                                             # wrong device
        (ValueError, good[:-1]),                                                              # wrong shape
        (ValueError, good.reshape(-1)),
        (ValueError, wide[::2, ::2]),                                                         # neither stride is 1
        (ValueError, torch.zeros(n_cols, dtype=torch.float64, device="cuda").expand(n_rows, n_cols)),   # rows that overlap: ld too small
        (ValueError, torch.zeros(n_rows, dtype=torch.float64, device="cuda").expand(n_cols, n_rows).T),
    ]
    stamp, area = dM.index_stamp(), dM.data.clone()
    for error, t in bad:
        with pytest.raises(error):
            dbcsr_to_dense(dM, out=t, engine=eng)
        with pytest.raises(error):
            dbcsr_from_dense(t, dM, engine=eng)
    for f in (lambda: dbcsr_to_dense(inside, out=over, engine=eng), lambda: dbcsr_from_dense(over, inside, engine=eng)):
        with pytest.raises(ValueError, match="overlap"):
            f()
    for sym, error in (("X", ValueError), ("H", ValueError)):   # an unknown symmetry; a symmetry that real data does not have
        dM.symmetry = sym
        with pytest.raises(error):
            dbcsr_to_dense(dM, engine=eng)
        with pytest.raises(error):
            dbcsr_from_dense(good, dM, engine=eng)
    dM.symmetry = "S"   # a stored triangle needs a square block structure
    with pytest.raises(ValueError):
        dbcsr_to_dense(dM, engine=eng)
    dM.symmetry = "N"
    ints = DbcsrMatrix(dM.row_blk_size, dM.col_blk_size, dM.row_p, dM.col_i, dM.blk_p, torch.zeros(n, dtype=torch.int32, device="cuda"))
    with pytest.raises(TypeError):
        dbcsr_to_dense(ints, engine=eng)
    assert dM.index_stamp() == stamp and torch.equal(dM.data, area)
    rs, cs = dM.row_blk_size, dM.col_blk_size
    for error, args, kw in [
        (TypeError, (np.zeros((n_rows, n_cols)), rs, cs), {}),
        (TypeError, (good.to(torch.int32), rs, cs), {}),
        (ValueError, (good.cpu(), rs, cs), {}),
        (ValueError, (good.reshape(-1), rs, cs), {}),
        (ValueError, (good, cs, rs), {}),                       # block-size sums that are not the shape
        (ValueError, (good[:-1], rs, cs), {}),
        (ValueError, (wide[::2, ::2], rs, cs), {}),
        (ValueError, (good, rs, cs), {"eps": -1.0}),
        (ValueError, (good, rs, cs), {"eps": float("nan")}),
        (TypeError, (good, [5.5, 2.0], cs), {}),
        (ValueError, (good, [n_rows + 1, -1], cs), {}),
    ]:
        with pytest.raises(error):
            dbcsr_create_from_dense(*args, engine=eng, **kw)


# ---- 11. C-ABI answers ---------------------------------------------------------------------------------------------------------------------------------------------
def test_c_abi_answers(eng):
    M = matrix("float64")
    n_rows, n_cols = full_shape(M)
    dM = to_dev(M)
    out = torch.full((n_rows, n_cols), np.nan, dtype=torch.float64, device="cuda")
    untouched = host(out).copy()
    lib, h, st, code = eng.L, eng.h, StreamHandle(), L.dbcsr_type_real_8
    d = dM.desc()
    area = host(dM.data).copy()

    def to_dense(handle=h, datatype=code, m=C.byref(d), kind=-1, ptr=out.data_ptr(), rows=n_rows, cols=n_cols, ld=n_cols, col_major=0):
        return lib.dbcsr_amd_bcsr_to_dense(handle, datatype, m, kind, ptr, rows, cols, ld, col_major, st.ptr)

    def from_dense_apply(handle=h, datatype=code, m=C.byref(d), ptr=out.data_ptr(), rows=n_rows, cols=n_cols, ld=n_cols, col_major=0):
        return lib.dbcsr_amd_bcsr_from_dense_apply(handle, datatype, ptr, rows, cols, ld, col_major, m, st.ptr)

    for f in (to_dense, from_dense_apply):
        assert f(handle=None) == -1 and f(m=None) == -1
        assert f(rows=n_rows - 1) == -1 and f(cols=n_cols + 1) == -1 and f(rows=-1) == -1, "n_rows / n_cols are the block-size sums"
        assert f(ld=n_cols - 1) == -1 and f(ld=n_rows - 1, col_major=1) == -1, "ld below the window's extent"
        assert f(ptr=None) == -1, "a null tensor with a window that has elements"
        assert f(datatype=99) == -10
    assert to_dense(kind=4) == -1 and to_dense(kind=-2) == -1 and to_dense(kind=0) == -1, "an unknown kind; a triangle of a non-square structure"
    torch.cuda.synchronize()
    assert same_bits(host(out), untouched) and same_bits(host(dM.data), area), "a refused call writes nothing"
    none = np.zeros(0, np.int32)
    dZ = to_dev(from_blocks(none, none, {}, np.float64))
    z = dZ.desc()
    assert to_dense(m=C.byref(z), ptr=None, rows=0, cols=0, ld=0) == 0 and from_dense_apply(m=C.byref(z), ptr=None, rows=0, cols=0, ld=0) == 0
    assert to_dense(m=C.byref(z), ptr=None, rows=1, cols=0, ld=0) == -1

    row_p = torch.full((len(ROWS) + 1,), -7, dtype=torch.int32, device="cuda")
    nt = len(ROWS) * len(COLS)
    col_i = torch.full((nt,), -7, dtype=torch.int32, device="cuda")
    blk_p = torch.full((nt,), -7, dtype=torch.int64, device="cuda")
    nb, nz = C.c_int64(-1), C.c_int64(-1)

    def count(handle=h, datatype=code, ptr=out.data_ptr(), rows=n_rows, cols=n_cols, ld=n_cols, col_major=0, rs=dM.row_blk_size.data_ptr(),
              cs=dM.col_blk_size.data_ptr(), nbr=len(ROWS), nbc=len(COLS), eps=0.0, rp=row_p.data_ptr(), ci=col_i.data_ptr(), bp=blk_p.data_ptr()):
        return lib.dbcsr_amd_bcsr_from_dense_count(handle, datatype, ptr, rows, cols, ld, col_major, rs, cs, nbr, nbc, eps, rp, ci, bp, C.byref(nb),
                                                   C.byref(nz), st.ptr)

    assert count(handle=None) == -1 and count(rp=None) == -1 and count(ci=None) == -1 and count(rs=None) == -1
    assert count(rows=n_rows + 1) == -1 and count(cols=n_cols - 1) == -1 and count(ld=n_cols - 1) == -1 and count(ptr=None) == -1
    assert count(eps=-1.0) == -1 and count(eps=float("nan")) == -1 and count(nbr=-1) == -1
    assert count(datatype=99) == -10
    torch.cuda.synchronize()
    assert (host(col_i) == -7).all() and (host(blk_p) == -7).all(), "a refused count names no block"
    out.zero_()
    assert count(eps=1.0) == 0 and (nb.value, nz.value) == (0, 0) and not host(row_p).any()
    assert count() == 0 and (nb.value, nz.value) == (nt, n_rows * n_cols)
    assert count(ptr=None, rows=0, cols=0, ld=0, rs=None, cs=None, nbr=0, nbc=0, ci=None, bp=None) == 0 and (nb.value, nz.value) == (0, 0)
