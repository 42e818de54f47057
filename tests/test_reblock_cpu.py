"""What tests/test_gpu_reblock.py compares with, checked without a GPU: the numpy restatement of re-blocking (tests/reblock_ref.py: the pattern from block
rectangles, the values from an image that marks "named" per element) agrees with a straightforward dense one and round-trips; the two size helpers; the
test inputs meet the conditions the GPU tests rely on -- a source block cut into at least 2 x 2 pieces, a new block fed by at least 2 x 2 source blocks, a
new block only partly covered (it holds +0.0 that the value rule put there), a new block above 32 in both directions, a source block and a new block of one
element, block rows that are really empty; the three C entries are declared in the header and listed once in lib.MM_SYMBOLS (tests/test_cabi_symbols.py then
checks the export); the four Python names are exported; and the refusals that need no device come before any call of the library."""
import os
import re

import numpy as np
import pytest
import torch

import dbcsr_amd
from dbcsr_amd import lib as L
from dbcsr_amd import reblock as RB
from dbcsr_amd.matrix import DbcsrMatrix
from tests import reblock_ref as R
from tests.test_gpu_matrix_norms import blocks_of, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.NAMES)
@pytest.mark.parametrize("case", R.CASES)
def test_the_restatement_agrees_with_the_dense_way(case, name):
    """the source has no block of no element, so a rectangle is met iff one of its elements is named: two routes to one matrix"""
    for dtype in R.DTYPES:
        M = R.source(case, np.dtype(dtype).name)
        rs, cs = R.STRUCTURES[name]
        got = R.reference(case, np.dtype(dtype).name, name)
        assert R.same_matrix(got, R.dense_way(M, rs, cs))
        assert sorted(blocks_of(got)) == sorted(R.pattern(M, rs, cs))
        assert got.blk_p.tolist() == np.concatenate([[0], np.cumsum([v.size for v in blocks_of(got).values()])[:-1]]).tolist(), "packed"


@pytest.mark.parametrize("name", R.NAMES)
def test_the_way_back_gives_the_source(name):
    for case in R.CASES:
        M = R.source(case, "float64")
        back = R.reblock_into(R.reference(case, "float64", name), M, area=np.full(M.data.size, np.nan))
        assert same_bits(back, M.data)


def test_the_same_sizes_give_the_source():
    for case in R.CASES:
        for dtype in R.DTYPES:
            assert R.same_matrix(R.reference(case, np.dtype(dtype).name, "same"), R.source(case, np.dtype(dtype).name))


def test_the_pattern_does_not_look_at_values():
    M = R.source("partial", "float64")
    Z = type(M)(M.row_sizes, M.col_sizes, M.row_p, M.col_i, M.blk_p, np.zeros_like(M.data))
    for name in R.NAMES:
        got = R.reblock(Z, *R.STRUCTURES[name])
        assert sorted(blocks_of(got)) == sorted(blocks_of(R.reference("partial", "float64", name))) and not got.data.any()


# ---- the conditions on the inputs ------------------------------------------------------------------------------------------------------------------------
def spans(M, rs, cs):
    """per source block the number of new block rows and columns it meets"""
    ro, co, nro, nco = R.offsets(M.row_sizes), R.offsets(M.col_sizes), R.offsets(rs), R.offsets(cs)
    return [(len(R.span(nro, ro[r], ro[r + 1])), len(R.span(nco, co[c], co[c + 1]))) for r, c in zip(M.rows().tolist(), M.col_i.tolist())]


def feeders(M, rs, cs):
    """per new block (I, J) the source block rows and columns that feed it"""
    ro, co, nro, nco = R.offsets(M.row_sizes), R.offsets(M.col_sizes), R.offsets(rs), R.offsets(cs)
    out = {}
    for r, c in zip(M.rows().tolist(), M.col_i.tolist()):
        for i in R.span(nro, ro[r], ro[r + 1]):
            for j in R.span(nco, co[c], co[c + 1]):
                rr, cc = out.setdefault((i, j), (set(), set()))
                rr.add(r), cc.add(c)
    return out


def test_the_inputs_reach_what_the_kernel_can_get_wrong():
    M = R.source("partial", "float64")
    cut = [n for n in R.NAMES if any(a >= 2 and b >= 2 for a, b in spans(M, *R.STRUCTURES[n]))]
    assert {"ones", "u32", "shifted", "halves"} <= set(cut), "a source block cut into at least 2 x 2 pieces"
    fed = [n for n in R.NAMES if any(len(rr) >= 2 and len(cc) >= 2 for rr, cc in feeders(M, *R.STRUCTURES[n]).values())]
    assert {"one", "u32", "shifted", "pairs", "big"} <= set(fed), "a new block fed by at least 2 x 2 source blocks"
    # a new block only partly covered: it holds elements no source block names, which the value rule made +0.0
    _, named = R.images(M)
    for n in ("one", "u32", "shifted", "pairs", "big"):
        rs, cs = R.STRUCTURES[n]
        nro, nco = R.offsets(rs), R.offsets(cs)
        partly = [(i, j) for i, j in R.pattern(M, rs, cs) if not named[nro[i]:nro[i + 1], nco[j]:nco[j + 1]].all()]
        assert partly, n
        i, j = partly[0]
        v = blocks_of(R.reference("partial", "float64", n))[(i, j)].reshape(cs[j], rs[i]).T
        hole = ~named[nro[i]:nro[i + 1], nco[j]:nco[j + 1]]
        assert same_bits(v[hole], np.zeros(int(hole.sum())))
    for n in ("one", "big", "pairs"):
        rs, cs = R.STRUCTURES[n]
        assert any(rs[i] > 32 and cs[j] > 32 for i, j in R.pattern(M, rs, cs)), "a new block above 32 in both directions"
    assert (1, 1) in [(int(M.row_sizes[r]), int(M.col_sizes[c])) for r, c in blocks_of(R.source("full", "float64"))], "a source block of one element"
    assert any(M.row_sizes[r] == 1 or M.col_sizes[c] == 1 for r, c in blocks_of(M))
    assert blocks_of(R.reference("partial", "float64", "ones")), "new blocks of one element"
    # the empty block rows are really empty, in the source and -- under the same sizes and under the halves -- in the result
    assert all(M.row_p[r] == M.row_p[r + 1] for r in (2, 8))
    same, halves = R.reference("partial", "float64", "same"), R.reference("partial", "float64", "halves")
    assert all(same.row_p[r] == same.row_p[r + 1] for r in (2, 8))
    assert sum(1 for r in range(halves.nbr) if halves.row_p[r] == halves.row_p[r + 1]) == 2
    # the special values sit in a block that every structure but the same sizes cuts or merges
    special = blocks_of(M)[(4, 7)][:5]
    assert np.signbit(special[1]) and np.isnan(special[2]) and np.isinf(special[3]) and np.isinf(special[4])


# ---- the size helpers ------------------------------------------------------------------------------------------------------------------------------------
def test_merged_block_sizes():
    f = RB.dbcsr_merged_block_sizes
    assert f([5, 13, 23, 5, 13, 23], 32) == [18, 28, 13, 23]
    assert f([23] * 5, 32) == [23] * 5 and f([23] * 5, 64) == [46, 46, 23] and f([23] * 4, 46) == [46, 46]
    assert f([40, 5, 5, 64, 1], 32) == [40, 10, 64, 1], "a block larger than the target stays alone"
    assert f([], 32) == [] and f([7], 1) == [7]
    assert f(R.ROWS, 32) == [19, 23, 32, 33, 40, 64, 6] and all(isinstance(s, int) for s in f(R.ROWS, 32))
    assert f(np.asarray([1, 1, 1], np.int64), 2) == [2, 1]
    for sizes, target in (([5, 13], 0), ([5, 0], 8), ([5, -1], 8)):
        with pytest.raises(ValueError):
            f(sizes, target)
    with pytest.raises(TypeError):
        f([5.5, 2], 8)


def test_split_block_sizes():
    f = RB.dbcsr_split_block_sizes
    assert f([23], 12) == [12, 11] and f([23, 23], 12) == [12, 11, 12, 11]
    assert f([64], 32) == [32, 32] and f([65], 32) == [22, 22, 21] and f([5], 32) == [5] and f([7], 1) == [1] * 7
    assert f([1, 5, 96], 40) == [1, 5, 32, 32, 32] and f([], 3) == []
    for sizes in ([5, 13, 1, 23, 32, 33, 40, 64, 96], list(range(1, 70))):
        for mx in (1, 2, 7, 12, 32, 100):
            out = f(sizes, mx)
            assert sum(out) == sum(sizes) and max(out) <= mx and min(out) >= 1
            at = 0
            for s in sizes:   # the pieces of one block are consecutive, as few as possible, and differ by at most one
                k = -(-s // mx)
                piece = out[at:at + k]
                assert sum(piece) == s and max(piece) - min(piece) <= 1 and piece == sorted(piece, reverse=True)
                at += k
    assert f(RB.dbcsr_merged_block_sizes([12, 11, 12, 11], 23), 12) == [12, 11, 12, 11]
    for sizes, mx in (([5], 0), ([0], 4)):
        with pytest.raises(ValueError):
            f(sizes, mx)


# ---- the interface ---------------------------------------------------------------------------------------------------------------------------------------
ENTRIES = ("dbcsr_amd_bcsr_reblock_name_blocks", "dbcsr_amd_bcsr_reserve_apply_index", "dbcsr_amd_bcsr_reblock_gather")
NAMES = ("dbcsr_reblock", "dbcsr_reblock_into", "dbcsr_merged_block_sizes", "dbcsr_split_block_sizes")


def test_the_entries_are_declared_and_listed_once():
    header = open(os.path.join(ROOT, "include", "dbcsr_amd_mm.h")).read()
    assert "Re-blocking" in header
    for e in ENTRIES:
        assert len(re.findall(r"^int %s\(" % e, header, flags=re.M)) == 1, e
        assert L.MM_SYMBOLS.count(e) == 1, e


def test_the_python_names_are_exported():
    for n in NAMES:
        assert getattr(dbcsr_amd, n) is getattr(RB, n) and n in dbcsr_amd.__all__


def host_matrix(dtype=torch.float64, symmetry="N"):
    M = R.source("partial", "float64")
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt)
    return DbcsrMatrix(t(M.row_sizes, torch.int32), t(M.col_sizes, torch.int32), t(M.row_p, torch.int32), t(M.col_i, torch.int32), t(M.blk_p, torch.int64),
                       torch.as_tensor(M.data).to(dtype), symmetry=symmetry)


def test_refusals_that_need_no_device(monkeypatch):
    """a matrix on the host, an unknown symmetry, no matrix at all: each refused before the engine is asked for (no library is loaded for them)"""
    def no_engine():
        raise AssertionError("a refusal must come before any call of the library")
    monkeypatch.setattr(RB, "default_engine", no_engine)
    rs, cs = R.STRUCTURES["u32"]
    with pytest.raises(ValueError, match="on the host"):
        RB.dbcsr_reblock(host_matrix(), rs, cs)
    with pytest.raises(ValueError, match="on the host"):
        RB.dbcsr_reblock_into(host_matrix(), host_matrix())
    with pytest.raises(ValueError, match="symmetry"):
        RB.dbcsr_reblock(host_matrix(symmetry="X"), rs, cs)
    with pytest.raises(ValueError, match="symmetry"):
        RB.dbcsr_reblock_into(host_matrix(symmetry="X"), host_matrix())
    with pytest.raises(TypeError):
        RB.dbcsr_reblock(host_matrix(dtype=torch.float16), rs, cs)
    with pytest.raises(TypeError):
        RB.dbcsr_reblock(None, rs, cs)
    with pytest.raises(TypeError):
        RB.dbcsr_reblock_into(None, host_matrix())
