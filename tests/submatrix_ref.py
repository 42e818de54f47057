"""The submatrix method restated in numpy: what tests/test_gpu_submatrix.py compares the device with, bit for bit, and what tests/test_submatrix_cpu.py
checks without a GPU.  Built on blocks_of / from_blocks / dense / same_bits of tests/test_gpu_matrix_norms.py and on twin_dense of tests/test_gpu_dense.py
(the sign-flip reading of a stored triangle).

Matrices: 9 x 9 blocks with the sizes 5 13 1 23 32 33 40 64 1 (GD.SQUARE) -- every alignment behind a 1 x 1 block, both sides of the 32-element tile,
several tiles per block.  `general`: about half of the blocks, the diagonal blocks 1, 4 and 8 missing, block column 6 (and block row 6) holding nothing at
all, exact zeros of both signs.  The triangles are GD.matrix(..., "triangle") (block row 2 empty, some diagonal blocks missing)."""
import functools

import numpy as np

from tests import test_gpu_dense as GD
from tests.test_gpu_matrix_norms import blocks_of, dense, from_blocks, from_dense, is_complex, subset

SQUARE = GD.SQUARE
NB = len(SQUARE)
EMPTY = 6                 # the block column (and block row) without any block
NO_DIAG = (1, 4, 6, 8)    # block rows without a stored diagonal block
GROUPED = [0, 0, 1, 2, 2, 2, 3, -1, 3]
SYMMETRIES = {"float64": ("S", "A"), "float32": ("S", "A"), "complex128": ("H", "K")}


@functools.lru_cache(maxsize=None)
def general(dtype_name):
    dtype = np.dtype(dtype_name)
    rng = np.random.default_rng(61)
    blocks = {}
    for r in range(NB):
        for c in range(NB):
            stored = rng.random() < 0.5 or (r == c and r not in NO_DIAG) or (r, c) in ((7, 4), (3, 7), (5, 0))
            if not stored or EMPTY in (r, c) or (r == c and r in NO_DIAG):
                continue
            v = GD.random_values(rng, int(SQUARE[r]) * int(SQUARE[c]), dtype)
            if v.size >= 4:
                v[1], v[v.size - 2] = 0.0, (0.0 if is_complex(dtype) else -0.0)   # (the helper `dense` sums re + 1j * im: no -0.0 in complex data)
            blocks[(r, c)] = v
    M = from_blocks(SQUARE, SQUARE, blocks, dtype)
    assert 25 <= M.nblks <= 50 and not any(EMPTY in k for k in blocks) and not any((r, r) in blocks for r in NO_DIAG)
    return M


def triangle(dtype_name, below=False):
    """a stored triangle with zeros of both signs; below=True: every second block off the diagonal stored at the mirrored place (transposed), so that what
    it stands for under 'S' is the same full matrix"""
    U = GD.matrix(dtype_name, "triangle", zeros=True)
    if not below:
        return U
    moved = {}
    for (r, c), v in blocks_of(U).items():
        if c > r and (r + c) % 2:
            moved[(c, r)] = v.reshape(int(SQUARE[c]), int(SQUARE[r])).T.reshape(-1)
        else:
            moved[(r, c)] = v
    return from_blocks(SQUARE, SQUARE, moved, U.data.dtype)


def full_dense(M, symmetry="N"):
    """the full matrix; of a stored triangle (one block per pair, on either side of the diagonal) by the sign-flip reading"""
    return dense(M) if symmetry == "N" else GD.twin_dense(M, symmetry)


# ---- the index sets ------------------------------------------------------------------------------------------------------------------------------------------
def brute_sets(M, groups=None, symmetry="N"):
    """(sets, owner): the members of every submatrix by the definition, one block at a time"""
    nb = len(M.col_sizes)
    owner = list(range(nb)) if groups is None else [int(g) for g in groups]
    nsub = max(owner, default=-1) + 1
    sets = [set() for _ in range(nsub)]
    stored = set(blocks_of(M))
    for j in range(nb):
        if owner[j] < 0:
            continue
        S = sets[owner[j]]
        S.add(j)
        for i in range(nb):
            if (i, j) in stored or (symmetry != "N" and (j, i) in stored):
                S.add(i)
    return [sorted(S) for S in sets], owner


def plan_arrays(sets, sizes):
    """set_ptr, set_idx, set_off, sub_dim of the sets"""
    set_ptr, set_idx, set_off, sub_dim = [0], [], [], []
    for S in sets:
        off = 0
        for i in S:
            set_idx.append(i)
            set_off.append(off)
            off += int(sizes[i])
        sub_dim.append(off)
        set_ptr.append(len(set_idx))
    return tuple(np.asarray(x, np.int32) for x in (set_ptr, set_idx, set_off, sub_dim))


def elements_of(S, sizes):
    ro = np.concatenate([[0], np.cumsum(sizes)])
    return np.concatenate([np.arange(ro[i], ro[i + 1]) for i in S]).astype(np.int64) if S else np.zeros(0, np.int64)


# ---- the two copies ------------------------------------------------------------------------------------------------------------------------------------------
def window(D, S, sizes, n, pad_diag):
    """blockdiag(D[S, S], pad_diag I) of side n: the principal submatrix of the full matrix D on the elements of the block rows S"""
    e = elements_of(S, sizes)
    W = np.zeros((n, n), D.dtype)
    W[:e.size, :e.size] = D[np.ix_(e, e)]
    k = np.arange(e.size, n)
    W[k, k] = pad_diag
    return W


def gathered(M, symmetry, sets, subs, n, pad_diag):
    D = full_dense(M, symmetry)
    ids = range(len(sets)) if subs is None else subs
    return np.stack([window(D, sets[g], M.row_sizes, n, pad_diag) for g in ids]) if len(ids) else np.zeros((0, n, n), D.dtype)


def scattered_area(M, area, sets, owner, batch, subs=None):
    """the data area after the scatter: a stored block (r, c) with owner[c] = g in the batch and r in S_g holds the window's elements, everything else what
    `area` held.  Returns (area, the blocks written)."""
    out = area.copy()
    ids = list(range(len(sets))) if subs is None else list(subs)
    rows = M.rows()
    written = set()
    for b in range(M.nblks):
        r, c = int(rows[b]), int(M.col_i[b])
        g = owner[c]
        if g < 0 or g not in ids or r not in sets[g]:
            continue
        _, _, off, _ = plan_arrays([sets[g]], M.row_sizes)
        ro, co = int(off[sets[g].index(r)]), int(off[sets[g].index(c)])
        m, w = int(M.row_sizes[r]), int(M.col_sizes[c])
        blk = batch[ids.index(g)][ro:ro + m, co:co + w].T.reshape(-1)
        out[M.blk_p[b]:M.blk_p[b] + blk.size] = blk
        written.add((r, c))
    return out, written


# ---- the inverse workflow ----------------------------------------------------------------------------------------------------------------------------------
CLOSED = [0, 0, 0, 1, 1, 2, 2, 3, 3]   # groups whose sets are closed: the matrix below is block diagonal by group


@functools.lru_cache(maxsize=None)
def spd_closed():
    """(stored matrix 'N', its dense form): SPD, block diagonal by the groups of CLOSED, every block inside a group stored, eigenvalues >= 1 -- the submatrix
    of a group is the group's diagonal part, so the submatrix method gives the exact inverse on the pattern"""
    rng = np.random.default_rng(62)
    n = int(SQUARE.sum())
    ro = np.concatenate([[0], np.cumsum(SQUARE)])
    A = np.zeros((n, n))
    for g in sorted(set(CLOSED)):
        mem = [j for j in range(NB) if CLOSED[j] == g]
        e = elements_of(mem, SQUARE)
        X = rng.uniform(-1.0, 1.0, (e.size, e.size))
        B = X @ X.T / e.size + np.eye(e.size)
        A[np.ix_(e, e)] = (B + B.T) / 2
    M = subset(from_dense(A, SQUARE, SQUARE, np.float64), lambda r, c: CLOSED[r] == CLOSED[c])
    assert np.array_equal(dense(M), A) and ro[-1] == n
    return M, A


def inverse_bar(A, n_window):
    """|computed - exact| of an inverse by a backward-stable solver is bounded by about n u kappa_2(A) ||A^-1||_2 (Higham, Accuracy and Stability, 14.1: the
    forward error of each column is kappa times the backward error n u, relative to ||A^-1||); two such results differ by at most twice that.  n is the
    largest window side: a window's inverse is computed from that many rows.  Derived as GD.eigenvalue_bar is; nothing of it is measured on the device."""
    inv_norm = float(np.linalg.norm(np.linalg.inv(A), 2))
    return n_window * 2.0 ** -53 * float(np.linalg.cond(A, 2)) * inv_norm
