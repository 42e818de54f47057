"""Host reference of the element-wise operations on two patterns (dbcsr_hadamard_product, dbcsr_copy with keep_sparsity,
dbcsr_function_of_elements) and the seeded inputs of their tests: numpy on dicts of blocks, nothing here needs a device.  Shared by
tests/test_gpu_elementwise.py (which runs the device against it) and tests/test_elementwise_cpu.py (which checks the reference against
dense numpy and asserts what the GPU test relies on about these inputs).

A matrix is an oracle.Bcsr; as a dict it is {(block row, block column): its elements, column-major, a view of the data area}."""
import functools

import numpy as np

from oracle import oracle as O

F64, F32, Z64 = np.float64, np.float32, np.complex128
DTYPES = [F64, F32, Z64]
IDS = ["fp64", "fp32", "z64"]
U53 = 2.0 ** -53
CANARY = -77.25   # what the holes of an unpacked matrix hold


def unit(dtype):
    return 2.0 ** -24 if np.dtype(dtype) == np.float32 else U53


# ---- a matrix as a dict of blocks ---------------------------------------------------------------------------------------------------------------
def sizes_of(M):
    return M.row_sizes[M.rows()].astype(np.int64) * M.col_sizes[M.col_i].astype(np.int64)


def blocks_of(M):
    rows, size = M.rows(), sizes_of(M)
    return {(int(rows[b]), int(M.col_i[b])): M.data[M.blk_p[b]:M.blk_p[b] + size[b]] for b in range(M.nblks)}


def from_blocks(rs, cs, blocks, dtype):
    """packed matrix of the blocks given: sorted block columns per row, blk_p the running sum of the block sizes"""
    keys = sorted(blocks)
    rr = np.asarray([k[0] for k in keys], np.int64)
    cc = np.asarray([k[1] for k in keys], np.int32)
    nze = np.asarray([int(rs[r]) * int(cs[c]) for r, c in keys], np.int64)
    blk_p = np.concatenate([[0], np.cumsum(nze)[:-1]]).astype(np.int64) if keys else np.zeros(0, np.int64)
    data = np.concatenate([np.asarray(blocks[k], dtype) for k in keys]) if keys else np.zeros(0, dtype)
    row_p = np.zeros(len(rs) + 1, np.int64)
    np.add.at(row_p, rr + 1, 1)
    return O.Bcsr(rs, cs, np.cumsum(row_p).astype(np.int32), cc, blk_p, data.astype(dtype))


def typed(M, dtype, seed=7):
    """the oracle's float64 matrix in another data type, with both signs; complex: uniform(-1, 1) imaginary parts laid over it"""
    if np.dtype(dtype).kind == "c":
        rng = np.random.default_rng(seed)
        data = M.data * rng.choice([-1.0, 1.0], M.data.size) + 1j * rng.uniform(-1.0, 1.0, M.data.size)
    else:
        data = M.data - 0.4
    return O.Bcsr(M.row_sizes, M.col_sizes, M.row_p, M.col_i, M.blk_p, data.astype(dtype))


def with_data(M, data):
    return O.Bcsr(M.row_sizes, M.col_sizes, M.row_p, M.col_i, M.blk_p, data)


def dense(M):
    """the full matrix (blocks the index names, zero elsewhere); any blk_p"""
    ro = np.concatenate([[0], np.cumsum(M.row_sizes)])
    co = np.concatenate([[0], np.cumsum(M.col_sizes)])
    D = np.zeros((ro[-1], co[-1]), M.data.dtype)
    for (r, c), v in blocks_of(M).items():
        D[ro[r]:ro[r + 1], co[c]:co[c + 1]] = v.reshape(int(M.col_sizes[c]), int(M.row_sizes[r])).T
    return D


def same_bits(x, y):
    return x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


def subset(M, keep):
    """M without the blocks for which keep(r, c) is false (packed again)"""
    return from_blocks(M.row_sizes, M.col_sizes, {k: v for k, v in blocks_of(M).items() if keep(*k)}, M.data.dtype)


def with_holes(M):
    """M with the same blocks at offsets that leave gaps: 3 or 4 elements in front of every block (so blocks start at odd elements too) and 5
    behind the last one, the gaps filled with CANARY.  named_mask(result) tells the blocks from the gaps."""
    size = sizes_of(M)
    packed = np.concatenate([[0], np.cumsum(size)[:-1]]).astype(np.int64) if M.nblks else np.zeros(0, np.int64)
    idx = np.arange(M.nblks, dtype=np.int64)
    blk_p = packed + 3 * (idx + 1) + (idx + 1) // 2
    extent = int((blk_p + size).max()) + 5 if M.nblks else 5
    data = np.full(extent, CANARY, M.data.dtype)
    for b in range(M.nblks):
        data[blk_p[b]:blk_p[b] + size[b]] = M.data[M.blk_p[b]:M.blk_p[b] + size[b]]
    return O.Bcsr(M.row_sizes, M.col_sizes, M.row_p, M.col_i, blk_p, data)


def named_mask(M, extent=None):
    """True for the elements of the data area that the index names"""
    mask = np.zeros(M.data.size if extent is None else extent, bool)
    size = sizes_of(M)
    for b in range(M.nblks):
        mask[M.blk_p[b]:M.blk_p[b] + size[b]] = True
    return mask


# ---- the seeded inputs ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mixed_pair():
    """two matrices of 230 x 260 with the block-size mixes [1, 13, 1, 5] x [1, 23, 1, 4], sparsity 0.5 each, from different counters of the oracle's
    generator: independent patterns, so intersection, A-only and B-only are all populated"""
    rs, cs = O.make_block_sizes(230, [1, 13, 1, 5]), O.make_block_sizes(260, [1, 23, 1, 4])
    return O.make_random_matrix(rs, cs, 0.5, O.RANDMAT_SEED_INIT + 61), O.make_random_matrix(rs, cs, 0.5, O.RANDMAT_SEED_INIT + 62)


@functools.lru_cache(maxsize=None)
def tiny_pair():
    """tiny blocks ([1, 1, 1, 3], 76 block columns, fill 0.9): rows with more than 64 blocks, blocks at odd offsets"""
    rs = O.make_block_sizes(152, [1, 1, 1, 3])
    return O.make_random_matrix(rs, rs, 0.1, O.RANDMAT_SEED_INIT + 63), O.make_random_matrix(rs, rs, 0.1, O.RANDMAT_SEED_INIT + 64)


EDGE_SIZES = (np.asarray([2, 1, 3, 1, 2], np.int32), np.asarray([1, 3, 2, 1, 2], np.int32))
FULL5 = frozenset((r, c) for r in range(5) for c in range(5))
# hand-made patterns on 5 x 5 blocks: name -> (blocks of A, blocks of B)
EDGE_PATTERNS = {
    "a_empty": (frozenset(), FULL5),
    "b_empty": (FULL5, frozenset()),
    "both_empty": (frozenset(), frozenset()),
    "disjoint": (frozenset(k for k in FULL5 if (k[0] + k[1]) % 2 == 0), frozenset(k for k in FULL5 if (k[0] + k[1]) % 2 == 1)),
    # row 1: A has blocks and B none; row 3: the reverse; row 0: the partner is the first block of B's row; row 2: the last; row 4: both
    "rows": (frozenset({(0, 1), (0, 3), (1, 0), (1, 2), (1, 4), (2, 0), (2, 4), (4, 0), (4, 2), (4, 4)}),
             frozenset({(0, 1), (0, 2), (0, 4), (2, 1), (2, 3), (2, 4), (3, 0), (3, 3), (4, 0), (4, 1), (4, 4)})),
}


def edge_pair(name, dtype):
    rs, cs = EDGE_SIZES
    rng = np.random.default_rng(sorted(EDGE_PATTERNS).index(name) + 100)
    out = []
    for keys in EDGE_PATTERNS[name]:
        blocks = {}
        for k in sorted(keys):
            n = int(rs[k[0]]) * int(cs[k[1]])
            v = rng.uniform(-1.0, 1.0, n)
            blocks[k] = v + 1j * rng.uniform(-1.0, 1.0, n) if np.dtype(dtype).kind == "c" else v
        out.append(from_blocks(rs, cs, blocks, dtype))
    return out


# ---- hadamard product ---------------------------------------------------------------------------------------------------------------------------------
def reference_hadamard(A, B, assume=None):
    """(result, scale): the blocks both store (assume given: every block of A, B's missing block filled with it), a * b in the data's own precision,
    packed in sorted order; scale = |a| |b| per element.  assume == 1 where B has no block: A's block as it is"""
    dtype = A.data.dtype
    ba, bb = blocks_of(A), blocks_of(B)
    out, scale = {}, {}
    for k, a in ba.items():
        if k in bb:
            out[k], scale[k] = (a * bb[k]).astype(dtype), np.abs(a) * np.abs(bb[k])
        elif assume is not None:
            out[k] = a.copy() if assume == 1 else (a * np.asarray(assume, dtype)).astype(dtype)
            scale[k] = np.abs(a) * abs(assume)
    return from_blocks(A.row_sizes, A.col_sizes, out, dtype), from_blocks(A.row_sizes, A.col_sizes, scale, np.float64).data


def hadamard_bar(dtype, scale):
    """per element: 0 for real data (one multiplication: bit for bit); complex128: 4 u |a| |b| -- each part is two products and one sum, within
    2 u (|ar br| + |ai bi|) <= 2 u |a| |b| with or without contraction, and so is numpy's complex128 reference"""
    return 4 * U53 * scale if np.dtype(dtype).kind == "c" else np.zeros_like(scale)


# ---- copy onto a pattern ------------------------------------------------------------------------------------------------------------------------------
def reference_copy_onto(A, B):
    """B's data area after B <- A on B's pattern: A's block where A stores it, +0.0 where it does not, every other element as it was"""
    data = B.data.copy()
    ba, size = blocks_of(A), sizes_of(B)
    rows = B.rows()
    for b in range(B.nblks):
        src = ba.get((int(rows[b]), int(B.col_i[b])))
        data[B.blk_p[b]:B.blk_p[b] + size[b]] = 0 if src is None else src
    return data


# ---- functions of elements ----------------------------------------------------------------------------------------------------------------------------
FUNC_NAMES = ["inverse", "tanh", "dtanh", "ddtanh", "artanh", "sin", "dsin", "ddsin", "asin", "cos", "dcos", "ddcos"]
PARAMS = [(0.0, 1.0), (0.25, -0.5), (-0.125, 2.0)]   # (a0, a1)


def y_range(name):
    """(smallest, largest) |y| the inputs of the function may have"""
    return (0.25, 4.0) if name == "inverse" else ((0.0, 0.9) if name in ("artanh", "asin") else (0.0, 4.0))


def function_input(M, name, a0, a1, dtype):
    """M's pattern with elements x for which y = a1 x + a0 lies inside y_range(name) with a margin that the rounding of x to the type cannot use up:
    the oracle's values in [0, 1) spread over both signs of y"""
    lo, hi = y_range(name)
    lo, hi = (lo * 1.2 if lo else 0.0), hi * 0.95
    u = M.data.astype(np.float64)
    assert u.min() >= 0.0 and u.max() < 1.0
    sign = np.where((np.arange(u.size) % 3) == 1, -1.0, 1.0)
    y = sign * (lo + (hi - lo) * u)
    return with_data(M, ((y - a0) / a1).astype(dtype))


def y_of(x, a0, a1):
    return np.longdouble(a1) * x.astype(np.longdouble) + np.longdouble(a0)


def reference_function(name, x, a0, a1):
    """(f, f') in np.longdouble: the function's value at y = a1 x + a0 and its derivative by y.  1 - tanh^2 y is formed as 1 / cosh^2 y, the same
    function without the cancellation of the difference (at |y| = 4 it would cost the long double ten of its 64 bits)"""
    L = np.longdouble
    y, a1 = y_of(x, a0, a1), L(a1)
    t, s2 = np.tanh(y), 1 / np.cosh(y) ** 2
    return {
        "inverse": lambda: (1 / y, -1 / y ** 2),
        "tanh": lambda: (t, s2),
        "dtanh": lambda: (a1 * s2, -2 * a1 * t * s2),
        "ddtanh": lambda: (-2 * a1 ** 2 * t * s2, -2 * a1 ** 2 * s2 * (1 - 3 * t ** 2)),
        "artanh": lambda: (np.arctanh(y), 1 / (1 - y ** 2)),
        "sin": lambda: (np.sin(y), np.cos(y)),
        "dsin": lambda: (a1 * np.cos(y), -a1 * np.sin(y)),
        "ddsin": lambda: (-a1 ** 2 * np.sin(y), -a1 ** 2 * np.cos(y)),
        "asin": lambda: (np.arcsin(y), 1 / np.sqrt(1 - y ** 2)),
        "cos": lambda: (np.cos(y), -np.sin(y)),
        "dcos": lambda: (-a1 * np.sin(y), -a1 * np.cos(y)),
        "ddcos": lambda: (-a1 ** 2 * np.cos(y), a1 ** 2 * np.sin(y)),
    }[name]()


def function_errors(name, x, a0, a1, got):
    """(excess, ref): what the bar's first term has to cover, in units of u |ref| -- (|got - ref| - 2 u |f'(y)| (|a1 x| + |a0|)) / (u |ref|), the second
    term being the rounding of y itself, contracted or not -- and the reference: the formula in np.longdouble, rounded once to the type"""
    dtype = x.dtype
    u = np.longdouble(unit(dtype))
    f, df = reference_function(name, x, a0, a1)
    ref = f.astype(dtype)
    err = np.abs(got.astype(np.longdouble) - ref.astype(np.longdouble))
    slack = 2 * u * np.abs(df) * (np.abs(np.longdouble(a1) * x.astype(np.longdouble)) + abs(np.longdouble(a0)))
    return ((err - slack) / (u * np.abs(ref.astype(np.longdouble)))).astype(np.float64), ref
