"""The element CSR form in numpy, entry by entry, and the inputs of tests/test_gpu_csr.py (checked without a GPU by tests/test_csr_cpu.py).

to_csr(M, eps)                         (crow int64, col int32, values) of a host matrix (oracle.Bcsr): every element the index names (eps None), or every
                                       element that is not dropped -- an element is DROPPED iff |x| <= eps, real types in their own precision, complex ones
                                       hypot(re, im) in double; the holes of an unpacked matrix are never read
from_csr(crow, col, values, M, area)   the data area after dbcsr_from_csr: every element of every block M names is the CSR value at its (row, column) or
                                       +0.0; everything else keeps what `area` held; entries outside the pattern or outside [0, n_cols) are ignored
blocks_of_csr(crow, col, rs, cs)       the set of blocks (R, C) of the structure rs x cs that hold at least one entry

They are written for reading, not speed.  The matrices: the block-size mix of tests/test_gpu_dense.py (GD.ROWS x GD.COLS: the sizes 1, 5, 13, 23, 32, 33,
40, 64, 96, unequal row and column counts, block rows 2 and 8 empty) -- the smallest shapes that reach one tile, the tile loops in both directions (33, 40,
64, 96) and a block of one element."""
import functools

import numpy as np

from tests import test_gpu_dense as GD
from tests.test_gpu_matrix_norms import blocks_of, from_blocks, is_complex

EPS = GD.EPS
DTYPES = GD.DTYPES
IDS = GD.IDS
LOSING_ROW = (7, 3)   # (block row, row inside it) of eps_case that loses every element


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, np.int64))]).astype(np.int64)


def kept(x, eps):
    """the filter's rule: dropped iff |x| <= eps (eps None: nothing is dropped); a NaN stays"""
    if eps is None:
        return True
    if np.iscomplexobj(x):
        return not (np.hypot(np.float64(x.real), np.float64(x.imag)) <= np.float64(eps))
    return not (np.abs(x) <= x.dtype.type(eps))


def to_csr(M, eps=None):
    ro, co = offsets(M.row_sizes), offsets(M.col_sizes)
    rows = M.rows()
    entries = [[] for _ in range(int(ro[-1]))]
    for b in range(M.nblks):   # (block columns ascend inside a block row, so the element columns of a row arrive ascending)
        r, c = int(rows[b]), int(M.col_i[b])
        m, n = int(M.row_sizes[r]), int(M.col_sizes[c])
        for p in range(m):
            for q in range(n):
                x = M.data[int(M.blk_p[b]) + p + q * m]   # column by column
                if kept(x, eps):
                    entries[ro[r] + p].append((co[c] + q, x))
    crow = np.zeros(len(entries) + 1, np.int64)
    crow[1:] = np.cumsum([len(e) for e in entries])
    col = np.asarray([j for e in entries for j, _ in e], np.int32).reshape(-1)
    values = np.asarray([x for e in entries for _, x in e], M.data.dtype).reshape(-1)
    return crow, col, values


def from_csr(crow, col, values, M, area=None):
    ro, co = offsets(M.row_sizes), offsets(M.col_sizes)
    n_cols = int(co[-1])
    at = {}
    for i in range(len(crow) - 1):
        for t in range(int(crow[i]), int(crow[i + 1])):
            if 0 <= int(col[t]) < n_cols:
                at[(i, int(col[t]))] = values[t]
    out = (M.data if area is None else area).copy()
    rows = M.rows()
    zero = M.data.dtype.type(0)
    for b in range(M.nblks):
        r, c = int(rows[b]), int(M.col_i[b])
        m, n = int(M.row_sizes[r]), int(M.col_sizes[c])
        for p in range(m):
            for q in range(n):
                out[int(M.blk_p[b]) + p + q * m] = at.get((int(ro[r]) + p, int(co[c]) + q), zero)
    return out


def blocks_of_csr(crow, col, rs, cs):
    ro, co = offsets(rs), offsets(cs)
    out = set()
    for i in range(len(crow) - 1):
        for t in range(int(crow[i]), int(crow[i + 1])):
            j = int(col[t])
            if 0 <= i < ro[-1] and 0 <= j < co[-1]:
                out.add((int(np.searchsorted(ro, i, side="right")) - 1, int(np.searchsorted(co, j, side="right")) - 1))
    return out


# ---- the cases -------------------------------------------------------------------------------------------------------------------------------------------
def base(dtype_name):
    """the partial pattern: GD.matrix -- about half of the 10 x 8 blocks, block rows 2 and 8 empty, zeros of both signs"""
    return GD.matrix(dtype_name)


@functools.lru_cache(maxsize=None)
def full(dtype_name, zeros=True):
    """every block of GD.ROWS x GD.COLS; zeros: a few exact zeros of both signs (False: no zero and no NaN anywhere)"""
    dtype = np.dtype(dtype_name)
    rng = np.random.default_rng(61)
    blocks = {}
    for r in range(len(GD.ROWS)):
        for c in range(len(GD.COLS)):
            v = GD.random_values(rng, int(GD.ROWS[r]) * int(GD.COLS[c]), dtype)
            v[v == 0] = 1.0
            if zeros and v.size >= 4:
                v[1], v[v.size - 2] = 0.0, (0.0 if is_complex(dtype) else -0.0)
            blocks[(r, c)] = v
    return from_blocks(GD.ROWS, GD.COLS, blocks, dtype)


@functools.lru_cache(maxsize=None)
def nonzero(dtype_name):
    """the partial pattern without a zero element"""
    M = base(dtype_name)
    blocks = {k: np.where(v == 0, v.dtype.type(0.25), v) for k, v in blocks_of(M).items()}
    return from_blocks(M.row_sizes, M.col_sizes, blocks, M.data.dtype)


def large(rng, n, dtype):
    """|x| >= 0.5: far above 2 EPS"""
    x = GD.random_values(rng, n, dtype)
    return (np.sign(x.real) * (0.5 + 0.5 * np.abs(x.real)) + (1j * x.imag if is_complex(dtype) else 0)).astype(dtype)


@functools.lru_cache(maxsize=None)
def eps_case(dtype_name):
    """base's pattern with every block either kept whole (|x| >= 0.5), dropped whole (those values times 1e-6: |x| <= 1.5e-6, far below EPS / 2) or mixed
    element by element; row LOSING_ROW loses every element in every block of its block row; block (4, 7) holds +0.0, -0.0, NaN, +Inf and -Inf"""
    dtype = np.dtype(dtype_name)
    rng = np.random.default_rng(62)
    M = base(dtype_name)
    blocks = {}
    for i, ((r, c), old) in enumerate(sorted(blocks_of(M).items())):
        m = int(M.row_sizes[r])
        v = large(rng, old.size, dtype)
        kind = i % 3 if (r, c) != (4, 7) else 2
        if kind == 1:
            v = (v * 1e-6).astype(dtype)
        elif kind == 2:
            small = rng.random(v.size) < 0.5
            v[small] = (v[small] * 1e-6).astype(dtype)
        if r == LOSING_ROW[0]:
            v[LOSING_ROW[1]::m] = (large(rng, v.size // m, dtype) * 1e-6).astype(dtype)
        if (r, c) == (4, 7):
            if is_complex(dtype):
                v[:5] = [0.0, complex(-0.0, 0.0), complex(np.nan, 0.0), complex(np.inf, 0.0), complex(-np.inf, 1.0)]
            else:
                v[:5] = [0.0, -0.0, np.nan, np.inf, -np.inf]
        blocks[(r, c)] = v
    return from_blocks(M.row_sizes, M.col_sizes, blocks, dtype)


def magnitudes(M):
    return np.hypot(M.data.real.astype(np.float64), M.data.imag.astype(np.float64)) if is_complex(M.data.dtype) else np.abs(M.data.astype(np.float64))


def same_csr(got, ref):
    """crow, col and values each equal the reference; values by bits"""
    return all(g.dtype == r.dtype and g.shape == r.shape and g.tobytes() == r.tobytes() for g, r in zip(got, ref))
