"""Re-blocking in numpy, and the inputs of tests/test_gpu_reblock.py (checked without a GPU by tests/test_reblock_cpu.py).

The two rules (dbcsr_amd/reblock.py): a new block is stored iff its element rectangle intersects the rectangle of a block the source's index names --
values play no part; an element of a stored new block is the source's element at the same (row, column), bit for bit, where the index names a block there,
and +0.0 elsewhere.

pattern(M, rs, cs)             the set of new blocks, from the RECTANGLES of the source's blocks (no element is looked at)
images(M)                      (values, named): the source as a full array, and per element whether the index names it -- a stored zero and a hole differ
reblock(M, rs, cs)             the new packed matrix (oracle.Bcsr)
reblock_into(A, T, area)       T's data area after dbcsr_reblock_into(A, T): every element of every block T names by the values rule, the rest as in `area`
dense_way(M, rs, cs)           the same matrix the straightforward way, for the CPU test: tile by tile of the full arrays, a tile stored iff it holds a named element

Written for reading, not speed.  The source: the block-size mix of tests/test_gpu_dense.py (10 x 8 blocks of 1, 5, 13, 23, 32, 33, 40, 64, 96, block rows 2
and 8 empty), at the partial pattern with -0.0, NaN and +-Inf (csr_ref.eps_case) and at the full pattern (csr_ref.full)."""
import functools

import numpy as np

from tests import csr_ref as CR
from tests import test_gpu_dense as GD
from tests.test_gpu_matrix_norms import blocks_of, from_blocks

DTYPES, IDS = CR.DTYPES, CR.IDS
ROWS, COLS = GD.ROWS, GD.COLS


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, np.int64))]).astype(np.int64)


def span(off, lo, hi):
    """the blocks of the structure with running sums `off` that the elements lo ... hi - 1 meet"""
    return range(int(np.searchsorted(off, lo, side="right")) - 1, int(np.searchsorted(off, hi - 1, side="right")))


def pattern(M, rs, cs):
    ro, co, nro, nco = offsets(M.row_sizes), offsets(M.col_sizes), offsets(rs), offsets(cs)
    out = set()
    for r, c in zip(M.rows().tolist(), M.col_i.tolist()):
        if ro[r + 1] > ro[r] and co[c + 1] > co[c]:
            out |= {(i, j) for i in span(nro, ro[r], ro[r + 1]) for j in span(nco, co[c], co[c + 1])}
    return out


def images(M):
    ro, co = offsets(M.row_sizes), offsets(M.col_sizes)
    values = np.zeros((int(ro[-1]), int(co[-1])), M.data.dtype)
    named = np.zeros(values.shape, bool)
    for (r, c), v in blocks_of(M).items():
        m, n = int(M.row_sizes[r]), int(M.col_sizes[c])
        values[ro[r]:ro[r + 1], co[c]:co[c + 1]] = v.reshape(n, m).T   # (column by column)
        named[ro[r]:ro[r + 1], co[c]:co[c + 1]] = True
    return values, named


def tile(values, named, r0, r1, c0, c1):
    """the block of the rectangle, column by column: the values where named, +0.0 elsewhere"""
    out = np.zeros((r1 - r0, c1 - c0), values.dtype)
    mask = named[r0:r1, c0:c1]
    out[mask] = values[r0:r1, c0:c1][mask]
    return np.ascontiguousarray(out.T).reshape(-1)


def reblock(M, rs, cs):
    rs, cs = np.asarray(rs, np.int32), np.asarray(cs, np.int32)
    assert int(rs.sum()) == int(M.row_sizes.sum()) and int(cs.sum()) == int(M.col_sizes.sum()) and (rs >= 1).all() and (cs >= 1).all()
    values, named = images(M)
    nro, nco = offsets(rs), offsets(cs)
    return from_blocks(rs, cs, {(i, j): tile(values, named, nro[i], nro[i + 1], nco[j], nco[j + 1]) for i, j in pattern(M, rs, cs)}, M.data.dtype)


def reblock_into(A, T, area=None):
    assert int(T.row_sizes.sum()) == int(A.row_sizes.sum()) and int(T.col_sizes.sum()) == int(A.col_sizes.sum())
    values, named = images(A)
    ro, co = offsets(T.row_sizes), offsets(T.col_sizes)
    out = (T.data if area is None else area).copy()
    rows = T.rows()
    for b in range(T.nblks):
        r, c = int(rows[b]), int(T.col_i[b])
        v = tile(values, named, ro[r], ro[r + 1], co[c], co[c + 1])
        out[int(T.blk_p[b]):int(T.blk_p[b]) + v.size] = v
    return out


def dense_way(M, rs, cs):
    values, named = images(M)
    full = np.where(named, values, np.zeros((), values.dtype))
    nro, nco = offsets(rs), offsets(cs)
    blocks = {}
    for i in range(len(rs)):
        for j in range(len(cs)):
            if named[nro[i]:nro[i + 1], nco[j]:nco[j + 1]].any():
                blocks[(i, j)] = np.ascontiguousarray(full[nro[i]:nro[i + 1], nco[j]:nco[j + 1]].T).reshape(-1)
    return from_blocks(np.asarray(rs, np.int32), np.asarray(cs, np.int32), blocks, M.data.dtype)


def same_matrix(X, Y):
    """index and data, bit for bit"""
    index = ((X.row_sizes, Y.row_sizes), (X.col_sizes, Y.col_sizes), (X.row_p, Y.row_p), (X.col_i, Y.col_i), (X.blk_p, Y.blk_p))
    return all(np.array_equal(np.asarray(a, np.int64), np.asarray(b, np.int64)) for a, b in index) and X.data.dtype == Y.data.dtype and \
        X.data.tobytes() == Y.data.tobytes()


# ---- the cases -------------------------------------------------------------------------------------------------------------------------------------------
def uniform(total, size):
    return [size] * (total // size) + ([total % size] if total % size else [])


def shifted(total):
    """a first block of 7, then 16s: no boundary but the last is one of the source's"""
    return [7] + uniform(total - 7, 16)


def pairs(sizes):
    return [int(sum(sizes[i:i + 2])) for i in range(0, len(sizes), 2)]


def halves(sizes):
    return [h for s in sizes for h in ([int(s)] if s == 1 else [int(s) - int(s) // 2, int(s) // 2])]


def fixed(total, head):
    rest = total - sum(head)
    assert rest > 0
    return list(head) + [rest]


NR, NC = int(ROWS.sum()), int(COLS.sum())
STRUCTURES = {
    "same": (ROWS.tolist(), COLS.tolist()),
    "ones": ([1] * NR, [1] * NC),
    "one": ([NR], [NC]),
    "u32": (uniform(NR, 32), uniform(NC, 32)),
    "shifted": (shifted(NR), shifted(NC)),
    "pairs": (pairs(ROWS), pairs(COLS)),
    "halves": (halves(ROWS), halves(COLS)),
    "big": (fixed(NR, [96, 100]), fixed(NC, [100, 96])),
}
NAMES = list(STRUCTURES)
CASES = ("partial", "full")


def source(case, dtype_name):
    """partial: csr_ref.eps_case -- about half of the blocks, block rows 2 and 8 empty, +0.0, -0.0, NaN, +Inf and -Inf in block (4, 7); full: csr_ref.full"""
    return CR.eps_case(dtype_name) if case == "partial" else CR.full(dtype_name)


@functools.lru_cache(maxsize=None)
def reference(case, dtype_name, name):
    """the re-blocked source, computed once per (case, type, structure) and shared by the tests: never written"""
    return reblock(source(case, dtype_name), *STRUCTURES[name])


def half_pattern(M, rs, cs):
    """every second block of the structure rs x cs, zero-filled: a destination that stores blocks the source does not meet and lacks blocks it meets"""
    keys = [(r, c) for r in range(len(rs)) for c in range(len(cs))][::2]
    return from_blocks(np.asarray(rs, np.int32), np.asarray(cs, np.int32), {(r, c): np.zeros(int(rs[r]) * int(cs[c])) for r, c in keys}, M.data.dtype)
