"""Block lists (dbcsr_reserve_blocks, dbcsr_put_blocks, dbcsr_get_blocks) without a GPU: the numpy reference that tests/test_gpu_blocklist.py compares
against, the matrices and lists it uses -- with the conditions on them that make the GPU test able to fail --, the declarations of the C entries,
the exported names and the argument checks that need no device.

The reference is a dict {(block row, block column): 1-D array, column-major} and goes through a list ENTRY BY ENTRY in list order, in the data's own
type: what the device must reproduce bit for bit with alpha == 1, whatever order its lanes arrive in."""
import os
import re

import numpy as np
import pytest
import torch

import dbcsr_amd
from dbcsr_amd import lib as L
from dbcsr_amd import operations as OPS
from dbcsr_amd.matrix import DbcsrMatrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [np.float64, np.float32, np.complex128]
IDS = ["fp64", "fp32", "z64"]
NAMES = ["dbcsr_reserve_blocks", "dbcsr_put_blocks", "dbcsr_get_blocks", "dbcsr_reserve_diag_blocks", "dbcsr_reserve_all_blocks",
         "dbcsr_create_from_blocks"]
ODD, TINY, B23, BIG = [1, 13, 1, 5, 1, 7], [1, 1, 1, 3], [1, 23], [1, 33, 1, 80]
# name -> (row mix, block rows, column mix, block columns).  31 ... 65 block columns: both sides of a bitmap word (32 bits) and of two; "tiny": blocks
# shorter than one 16-byte pack of float32, a block row with more than 128 blocks and one with more than 64; "none": no block at all
MATRICES = {"w31": (ODD, 5, ODD, 31), "w32": (ODD, 5, ODD, 32), "w33": (ODD, 5, ODD, 33), "w64": (ODD, 5, ODD, 64), "w65": (ODD, 5, ODD, 65),
            "tiny": (TINY, 4, TINY, 150), "b23": (B23, 5, B23, 6), "big": (BIG, 4, BIG, 4), "none": (ODD, 5, ODD, 33)}
LISTS = ["n0", "n1", "perm", "present", "absent", "mix", "dup3", "dup65", "dup130"]
DUPLICATES = {"dup3": 3, "dup65": 65, "dup130": 130}


def is_complex(dtype):
    return np.dtype(dtype).kind == "c"


def block_sizes(mix, n):
    """n block sizes from a mix (count, size, count, size, ...), repeated"""
    one = [s for k, s in zip(mix[0::2], mix[1::2]) for _ in range(k)]
    return np.asarray([one[i % len(one)] for i in range(n)], np.int32)


def values(rng, n, dtype):
    """n values of both signs whose magnitudes spread over seventeen binades: sums of them depend on the order"""
    x = rng.uniform(1.0, 2.0, n) * rng.choice([-1.0, 1.0], n) * 2.0 ** rng.integers(-8, 9, n)
    if is_complex(dtype):
        x = x + 1j * rng.uniform(1.0, 2.0, n) * rng.choice([-1.0, 1.0], n) * 2.0 ** rng.integers(-8, 9, n)
    return x.astype(dtype)


def make_matrix(name, dtype, seed=3):
    """(row sizes, column sizes, blocks): block row 2 is empty in every matrix"""
    rmix, nbr, cmix, nbc = MATRICES[name]
    rs, cs = block_sizes(rmix, nbr), block_sizes(cmix, nbc)
    rng = np.random.default_rng(seed + sum(map(ord, name)))
    coords = []
    if name == "tiny":
        coords += [(0, c) for c in range(nbc) if c % 11 != 3]
        coords += [(1, c) for c in range(0, nbc, 2)]
        coords += [(3, c) for c in range(nbc) if rng.random() < 0.1]
    elif name != "none":
        coords += [(r, c) for r in range(nbr) for c in range(nbc) if r != 2 and rng.random() < 0.45]
    return rs, cs, {(r, c): values(rng, int(rs[r]) * int(cs[c]), dtype) for r, c in coords}


def make_list(kind, rs, cs, blocks, seed=5):
    """(rows, cols) int32 of one of LISTS"""
    rng = np.random.default_rng(seed + sum(map(ord, kind)))
    present = sorted(blocks)
    absent = [(r, c) for r in range(len(rs)) for c in range(len(cs)) if (r, c) not in blocks]
    pick = lambda pool, k: [pool[i] for i in rng.permutation(len(pool))[:k]]
    if kind == "n0":
        out = []
    elif kind == "n1":
        out = pick(present or absent, 1)
    elif kind == "perm":
        out = pick(present, len(present))
    elif kind == "present":
        out = pick(present, 17)
        out = out + out[:3]
    elif kind == "absent":
        out = pick(absent, 40)
    elif kind == "mix":
        out = pick(present, 12) + pick(absent, 12)
        out = out + out[::5]
    else:
        k = DUPLICATES[kind]
        pool = present or absent
        target = [max(pool, key=lambda p: int(rs[p[0]]) * int(cs[p[1]]))]   # (the largest block: many elements whose sums can differ)
        out = target * k + pick([p for p in present if p != target[0]], k // 4 + 2) + pick([p for p in absent if p != target[0]], k // 4 + 2)
    out = [out[i] for i in rng.permutation(len(out))]
    return np.asarray([p[0] for p in out], np.int32), np.asarray([p[1] for p in out], np.int32)


def make_windows(rs, cs, rows, cols, dtype, seed=9):
    rng = np.random.default_rng(seed)
    return [values(rng, int(rs[r]) * int(cs[c]), dtype) for r, c in zip(rows, cols)]


def lay_out(windows, style, dtype, poison, seed=13):
    """(flat array, offsets): the windows in one array filled with poison.  "odd": one after another from element 1 on (blocks of odd sizes then start
    at odd and even elements alike); "gaps": 0 ... 4 elements of poison in front of every window"""
    rng = np.random.default_rng(seed)
    offsets, at = [], 1 if style == "odd" else 0
    for w in windows:
        at += int(rng.integers(0, 5)) if style == "gaps" else 0
        offsets.append(at)
        at += w.size
    flat = np.full(at + 3, poison, dtype)
    for o, w in zip(offsets, windows):
        flat[o:o + w.size] = w
    return flat, np.asarray(offsets, np.int64)


# ---- the reference ----------------------------------------------------------------------------------------------------------------------------------
def ref_reserve(rs, cs, blocks, rows, cols, upper_only=False):
    """(blocks afterwards, number created); ValueError for a coordinate outside the matrix (below the diagonal with upper_only), nothing changed"""
    for r, c in zip(rows, cols):
        if not (0 <= r < len(rs) and 0 <= c < len(cs)) or (upper_only and c < r):
            raise ValueError((int(r), int(c)))
    out = dict(blocks)
    dtype = next(iter(blocks.values())).dtype if blocks else None
    for r, c in zip(rows, cols):
        if (int(r), int(c)) not in out:
            out[(int(r), int(c))] = np.zeros(int(rs[r]) * int(cs[c]), dtype)
    return out, len(out) - len(blocks)


def ref_put(rs, cs, blocks, rows, cols, windows, dtype, summation=False, alpha=1.0, keep_sparsity=False, order=None):
    """blocks afterwards: entry by entry in list order (order: another order, for the checks of this file), in the data's own type; with alpha == 1
    nothing is multiplied"""
    out = {k: v.copy() for k, v in blocks.items()}
    a = np.dtype(dtype).type(alpha)
    for i in (range(len(rows)) if order is None else order):
        k = (int(rows[i]), int(cols[i]))
        if not (0 <= k[0] < len(rs) and 0 <= k[1] < len(cs)):
            continue
        if k not in out:
            if keep_sparsity:
                continue
            out[k] = np.zeros(int(rs[k[0]]) * int(cs[k[1]]), dtype)
        x = windows[i] if alpha == 1 else a * windows[i]
        out[k] = (out[k] + x) if summation else x.copy()
        assert out[k].dtype == np.dtype(dtype)
    return out


def ref_get(rs, cs, blocks, rows, cols, dtype):
    """(windows, found): a coordinate outside the matrix has an empty window"""
    wins, found = [], []
    for r, c in zip(rows, cols):
        inside = 0 <= r < len(rs) and 0 <= c < len(cs)
        have = (int(r), int(c)) in blocks
        wins.append(blocks[(int(r), int(c))] if have else np.zeros(int(rs[r]) * int(cs[c]) if inside else 0, dtype))
        found.append(1 if have else 0)
    return wins, np.asarray(found, np.int32)


def wide(dtype):
    return np.clongdouble if is_complex(dtype) else np.longdouble


def ref_put_wide(rs, cs, blocks, rows, cols, windows, dtype, summation, alpha):
    """(reference in long double, bar) per block of the matrix after a put with any alpha onto stored blocks: bar = u (k + 2) (|old| + sum |alpha| |x|)
    per element, u the unit roundoff of the type and k the number of contributions the result holds -- every contribution is rounded once as a product
    (or not at all when it is fused into the add) and once per addition that follows it, k at the most; alpha itself is rounded once to the type."""
    W = wide(dtype)
    u = 2.0 ** -24 if np.dtype(dtype) == np.float32 else 2.0 ** -53
    ref = {k: v.astype(W) for k, v in blocks.items()}
    mass = {k: np.abs(v).astype(np.float64) for k, v in blocks.items()}
    count = {k: 0 for k in blocks}
    for i in range(len(rows)):
        k = (int(rows[i]), int(cols[i]))
        if k not in ref:
            continue
        x = W(alpha) * windows[i].astype(W)
        m = abs(alpha) * np.abs(windows[i]).astype(np.float64)
        ref[k], mass[k], count[k] = (ref[k] + x, mass[k] + m, count[k] + 1) if summation else (x, m, 1)
    return ref, {k: u * (count[k] + 2) * mass[k] for k in ref}


# ---- the inputs can make the GPU test fail ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", sorted(DUPLICATES))
def test_the_order_of_duplicates_shows_in_the_bits(dtype, kind):
    """for every matrix the GPU test puts duplicates into: the contributions added in reverse order change at least one bit of the block that is hit
    several times, and without summation the first and the last contribution differ"""
    for name in MATRICES:
        rs, cs, blocks = make_matrix(name, dtype)
        rows, cols = make_list(kind, rs, cs, blocks)
        wins = make_windows(rs, cs, rows, cols, dtype)
        hits = {}
        for i, k in enumerate(zip(rows.tolist(), cols.tolist())):
            hits.setdefault(k, []).append(i)
        target = max(hits, key=lambda k: len(hits[k]))
        assert len(hits[target]) == DUPLICATES[kind]
        back = list(range(len(rows)))[::-1]
        for summation in (True, False):
            fwd = ref_put(rs, cs, blocks, rows, cols, wins, dtype, summation=summation)
            rev = ref_put(rs, cs, blocks, rows, cols, wins, dtype, summation=summation, order=back)
            assert fwd[target].tobytes() != rev[target].tobytes(), (name, summation)


@pytest.mark.parametrize("name", sorted(MATRICES))
def test_the_matrices_and_lists_are_what_they_claim(name):
    rs, cs, blocks = make_matrix(name, np.float64)
    per_row = [sum(1 for k in blocks if k[0] == r) for r in range(len(rs))]
    assert per_row[2] == 0, "an empty block row"
    assert int(rs.sum()) <= 600 and int(cs.sum()) <= 600
    if name == "tiny":
        assert per_row[0] > 128 and 64 < per_row[1] <= 128
        assert any(v.size * 4 < 16 for v in blocks.values()), "float32 blocks shorter than one 16-byte pack"
    if name == "none":
        assert not blocks
    for kind in LISTS:
        rows, cols = make_list(kind, rs, cs, blocks)
        have = [(r, c) in blocks for r, c in zip(rows.tolist(), cols.tolist())]
        assert rows.dtype == np.int32 and len(rows) == len(cols)
        if kind == "n0":
            assert len(rows) == 0
        if kind == "n1":
            assert len(rows) == 1
        if name == "none":
            assert not any(have)
            continue
        if kind == "perm":
            assert sorted(zip(rows.tolist(), cols.tolist())) == sorted(blocks)
            assert list(zip(rows.tolist(), cols.tolist())) != sorted(blocks), "not in index order"
        if kind == "present":
            assert all(have) and len(set(zip(rows.tolist(), cols.tolist()))) < len(rows)
        if kind == "absent":
            assert len(have) > 0 and not any(have)
        if kind == "mix":
            assert any(have) and not all(have), "the mix holds present and absent blocks"
        if kind in DUPLICATES:
            assert any(have) and not all(have)


def test_the_layouts_start_blocks_at_odd_offsets_and_leave_gaps():
    rs, cs, blocks = make_matrix("w33", np.float64)
    rows, cols = make_list("mix", rs, cs, blocks)
    wins = make_windows(rs, cs, rows, cols, np.float64)
    flat, off = lay_out(wins, "odd", np.float64, -7.25e33)
    assert np.any(off % 2 == 1) and np.any(off % 2 == 0) and off[0] == 1
    flat, off = lay_out(wins, "gaps", np.float64, -7.25e33)
    ends = off + np.asarray([w.size for w in wins])
    assert np.any(off[1:] > ends[:-1]) and np.count_nonzero(flat == -7.25e33) >= 3


def test_the_reference_restated():
    rs, cs = np.asarray([2, 1], np.int32), np.asarray([1, 3], np.int32)
    blocks = {(0, 1): np.arange(6, dtype=np.float64)}
    grown, n_new = ref_reserve(rs, cs, blocks, [1, 0, 1], [0, 1, 0])
    assert n_new == 1 and sorted(grown) == [(0, 1), (1, 0)] and grown[(1, 0)].tobytes() == np.zeros(1).tobytes()
    with pytest.raises(ValueError):
        ref_reserve(rs, cs, blocks, [2], [0])
    with pytest.raises(ValueError):
        ref_reserve(rs, cs, blocks, [1], [0], upper_only=True)
    x, y = np.full(6, 0.5), np.full(6, 2.0)
    rows, cols = np.asarray([0, 0, 1], np.int32), np.asarray([1, 1, 1], np.int32)
    wins = [x, y, np.ones(3)]
    assert np.array_equal(ref_put(rs, cs, blocks, rows, cols, wins, np.float64)[(0, 1)], y), "the last one wins"
    assert np.array_equal(ref_put(rs, cs, blocks, rows, cols, wins, np.float64, summation=True)[(0, 1)], np.arange(6) + 2.5)
    assert np.array_equal(ref_put(rs, cs, blocks, rows, cols, wins, np.float64, summation=True, alpha=2.0)[(1, 1)], np.full(3, 2.0))
    assert (1, 1) not in ref_put(rs, cs, blocks, rows, cols, wins, np.float64, keep_sparsity=True)
    got, found = ref_get(rs, cs, blocks, [0, 1, 5], [1, 1, 0], np.float64)
    assert found.tolist() == [1, 0, 0] and got[1].tobytes() == np.zeros(3).tobytes() and got[2].size == 0
    ref, bar = ref_put_wide(rs, cs, blocks, rows, cols, wins, np.float64, True, 0.5)
    assert np.allclose(np.asarray(ref[(0, 1)], np.float64), np.arange(6) + 1.25) and np.allclose(bar[(0, 1)], 2.0 ** -53 * 4 * (np.arange(6) + 1.25))


# ---- the C entries and the Python names ----------------------------------------------------------------------------------------------------------------
ENTRIES = {
    "dbcsr_amd_bcsr_reserve_count": ["void* handle", "const dbcsr_amd_bcsr* m", "int64_t n", "const int32_t* rows", "const int32_t* cols", "int upper_only",
                                     "int32_t* dst_row_p", "int64_t* nblks", "int64_t* nze", "int64_t* n_new", "int64_t* n_invalid", "void* stream"],
    "dbcsr_amd_bcsr_reserve_apply": ["void* handle", "libsmm_acc_data_t datatype", "const dbcsr_amd_bcsr* m", "dbcsr_amd_bcsr* dst", "void* stream"],
    "dbcsr_amd_bcsr_put_blocks": ["void* handle", "libsmm_acc_data_t datatype", "dbcsr_amd_bcsr* m", "int64_t n", "const int32_t* rows", "const int32_t* cols",
                                  "const int64_t* src_off", "const void* src", "const double alpha[2]", "int summation", "void* stream"],
    "dbcsr_amd_bcsr_get_blocks": ["void* handle", "libsmm_acc_data_t datatype", "const dbcsr_amd_bcsr* m", "int64_t n", "const int32_t* rows",
                                  "const int32_t* cols", "const int64_t* dst_off", "void* dst", "int32_t* found", "void* stream"],
}


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_the_c_entries_are_declared_and_listed(entry):
    header = open(os.path.join(ROOT, "include", "dbcsr_amd_mm.h")).read()
    assert "/* Block lists (" in header
    m = re.search(r"\bint %s\(([^)]*)\);" % entry, header)
    assert m, "%s is not declared in include/dbcsr_amd_mm.h" % entry
    assert [" ".join(a.split()) for a in m.group(1).split(",")] == ENTRIES[entry]
    assert header.index("/* Block lists (") < m.start()
    assert entry in L.MM_SYMBOLS and L.MM_SYMBOLS.count(entry) == 1


@pytest.mark.parametrize("name", NAMES)
def test_the_python_names_are_exported_and_documented(name):
    assert name in dbcsr_amd.__all__ and getattr(dbcsr_amd, name) is getattr(OPS, name)
    assert name + "(" in OPS.__doc__, "the module docstring lists %s" % name
    assert len(getattr(OPS, name).__doc__) > 100


# ---- argument checks that need no device -----------------------------------------------------------------------------------------------------------------
def host_matrix():
    i32 = lambda a: torch.tensor(a, dtype=torch.int32)
    return DbcsrMatrix(i32([2, 1]), i32([1, 3]), i32([0, 1, 1]), i32([1]), torch.tensor([0], dtype=torch.int64), torch.zeros(6, dtype=torch.float64))


def test_the_argument_checks_come_before_any_device_call(monkeypatch):
    monkeypatch.setattr(OPS, "default_engine", lambda: pytest.fail("an engine was asked for"))
    M = host_matrix()
    i32 = lambda a: torch.tensor(a, dtype=torch.int32)
    good, data = i32([0, 1]), torch.zeros(9, dtype=torch.float64)
    calls = {"reserve": lambda r, c: OPS.dbcsr_reserve_blocks(M, r, c), "put": lambda r, c: OPS.dbcsr_put_blocks(M, r, c, data),
             "get": lambda r, c: OPS.dbcsr_get_blocks(M, r, c)}
    for what, call in calls.items():
        for bad in (torch.tensor([0, 1]), torch.tensor([0.0, 1.0]), [0, 1], np.asarray([0, 1], np.int32)):   # int64, float, a list, numpy
            with pytest.raises(TypeError):
                call(bad, good)
            with pytest.raises(TypeError):
                call(good, bad)
        with pytest.raises(ValueError):
            call(i32([[0, 1]]), good)   # 2-D
        with pytest.raises(ValueError):
            call(good, i32(1))          # 0-D
        with pytest.raises(ValueError):
            call(good, i32([0, 1, 1]))  # differing lengths
    for off in (i32([0, 6]), torch.tensor([0.0, 6.0]), [0, 6]):
        with pytest.raises(TypeError):
            OPS.dbcsr_put_blocks(M, good, good, data, offsets=off)
        with pytest.raises(TypeError):
            OPS.dbcsr_get_blocks(M, good, good, out=data, offsets=off)
    with pytest.raises(ValueError):
        OPS.dbcsr_put_blocks(M, good, good, data, offsets=torch.tensor([0, 6, 9]))   # one offset per entry
    with pytest.raises(TypeError):
        OPS.dbcsr_put_blocks(M, good, good, data.float())          # another data type
    with pytest.raises(ValueError):
        OPS.dbcsr_put_blocks(M, good, good, data.reshape(3, 3))    # not flat
    with pytest.raises(TypeError):
        OPS.dbcsr_put_blocks(M, good, good, data, alpha=1j)        # a complex scalar with real data
    with pytest.raises(ValueError):
        OPS.dbcsr_put_blocks(M, good, good, M.data[:3])            # shares memory with the matrix
    with pytest.raises(ValueError):
        OPS.dbcsr_get_blocks(M, good, good, out=M.data)
    assert M.nblks == 1 and M.data.numel() == 6
