"""The placements of tests/test_gpu_far_offsets.py reach what they are meant to -- checked on the host indices alone, without a GPU.

For every (case, data type, plan) of the GPU file, on both arena sizes, the block products (r, k, c) are enumerated from the indices of A and B and
the far offsets of tests/far_arena.place are taken apart as the product records do (low 32 bits, bits 32-39).  These are conditions on the inputs of
the GPU tests: if a case misses one, the case or the placement changes, not the condition."""
import functools

import numpy as np
import pytest

from tests import far_arena as FA
from tests import test_gpu_far_offsets as G

TWO31, TWO32 = 2 ** 31, 2 ** 32


@functools.lru_cache(maxsize=None)
def products(i):
    """(index of the A block, index of the B block, index r * nbc + c of the C block) of every block product of entry i"""
    A, B, _ = G.operands(i)
    ar = A.rows().astype(np.int64)
    nb = np.diff(B.row_p).astype(np.int64)[A.col_i]                 # B blocks in the block row each A block meets
    ia = np.repeat(np.arange(A.nblks, dtype=np.int64), nb)
    first = np.repeat(B.row_p[:-1].astype(np.int64)[A.col_i], nb)
    ib = first + (np.arange(ia.size, dtype=np.int64) - np.repeat(np.cumsum(nb) - nb, nb))
    return ia, ib, ar[ia] * B.nbc + B.col_i[ib].astype(np.int64)


def intervals(M, blk_p):
    return [(s, e) for s, e, _ in FA.runs_of(blk_p, FA.block_sizes(M))]


def sizes_for(dtype):
    return [FA.ARENA_LARGE] if np.dtype(dtype).kind == "c" else [FA.ARENA_LARGE, FA.ARENA_SMALL]


@pytest.mark.parametrize("i", range(len(G.ENTRIES)), ids=G.entry_id)
def test_placement_reaches_every_boundary_and_high_byte(i):
    env, case, dtype, expect, lab = G.ENTRIES[i]
    A, B, Cm = G.operands(i)
    ia, ib, cb = products(i)
    assert ia.size > 0
    for nbytes in sizes_for(dtype):
        nelem = FA.view_elements(dtype, nbytes)
        bnd = FA.boundaries(nelem)
        large_f32 = np.dtype(dtype) == np.float32 and nbytes == FA.ARENA_LARGE
        assert TWO31 in bnd and TWO32 in bnd
        assert max(bnd) // TWO32 == {4: {FA.ARENA_LARGE: 4, FA.ARENA_SMALL: 2}, 8: {FA.ARENA_LARGE: 2, FA.ARENA_SMALL: 1}, 16: {FA.ARENA_LARGE: 1}}[np.dtype(dtype).itemsize][nbytes]
        straddled = {0: set(), 1: set()}   # the boundaries A / B have a straddling block at, over the plans the GPU file runs
        for plan in G.plans_of(i):
            pa, pb, pc = G.placements(A, B, Cm, dtype, plan, nbytes)
            mats = ((A, pa), (B, pb), (Cm, pc))
            # no two blocks overlap, every block lies inside the arena
            iv = [x for M, p in mats for x in intervals(M, p)]
            assert not FA.overlaps(iv), plan
            assert min(s for s, _ in iv) >= 0 and max(e for _, e in iv) <= nelem, plan
            # exactly one block straddles each boundary, A's and B's in turn
            owners = []
            for b in bnd:
                hit = [(w, int(x)) for w, (M, p) in enumerate(mats) for x in FA.straddlers(M, p, b)]
                assert len(hit) == 1 and hit[0][0] in (0, 1), (plan, b, hit)
                owners.append(hit[0][0])
                straddled[hit[0][0]].add(b)
            assert all(owners[k] != owners[k + 1] for k in range(len(owners) - 1)), (plan, owners)
            # zones start at odd element offsets for half of the boundaries (the slots beside the straddling run: C_in's)
            odd = [int(np.min(pc[np.abs(pc - b) < 4 * FA.SLOT])) % 2 for b in bnd if np.any(np.abs(pc - b) < 4 * FA.SLOT)]
            assert 0 < sum(odd) < len(odd) or len(odd) < 2, (plan, odd)
            # what the product records hold
            a_hi, a_lo, b_hi, b_lo = pa[ia] >> 32, pa[ia] & 0xffffffff, pb[ib] >> 32, pb[ib] & 0xffffffff
            pairs = set(zip(a_hi.tolist(), b_hi.tolist()))
            want = [(0, 1), (1, 0), (1, 1)] + ([(2, 1), (1, 2)] if large_f32 else [])
            assert all(w in pairs for w in want), (plan, sorted(pairs))
            if large_f32:
                assert max(max(p) for p in pairs) >= 3, (plan, sorted(pairs))
            assert np.any((a_lo >= TWO31) & (a_hi == 0)) and np.any((a_lo < TWO31) & (a_hi >= 1)), plan
            assert np.any((b_lo >= TWO31) & (b_hi == 0)) and np.any((b_lo < TWO31) & (b_hi >= 1)), plan
            # per C block: the product lists
            order = np.argsort(cb, kind="stable")
            starts = np.flatnonzero(np.concatenate([[True], np.diff(cb[order]) != 0]))
            lo_a, hi_a = np.minimum.reduceat(a_hi[order], starts), np.maximum.reduceat(a_hi[order], starts)
            lo_b, hi_b = np.minimum.reduceat(b_hi[order], starts), np.maximum.reduceat(b_hi[order], starts)
            count = np.diff(np.concatenate([starts, [cb.size]]))
            if plan.startswith("lines"):
                # one (a_hi, b_hi) per C block, whichever product comes first -- but for the lines whose run straddles 2^32, 2^33 or 2^34
                one = (lo_a == hi_a) & (lo_b == hi_b)
                assert 2 * one.sum() >= one.size, (plan, int(one.sum()), one.size)
                blocks_with = set(zip(lo_a[one].tolist(), lo_b[one].tolist()))
                assert all(w in blocks_with for w in want), (plan, sorted(blocks_with))
                if large_f32:
                    assert max(max(p) for p in blocks_with) >= 3
            else:
                several = count >= 2
                varied = several & ((lo_a != hi_a) | (lo_b != hi_b))
                assert several.sum() > 0 and 4 * varied.sum() >= several.sum(), (plan, int(varied.sum()), int(several.sum()))
        for w in (0, 1):
            assert TWO31 in straddled[w] and TWO32 in straddled[w], "each of A and B has a block straddling 2^31 and one straddling 2^32 in one of the plans"


def test_helpers_of_the_arena():
    assert FA.boundaries(FA.view_elements(np.float32, FA.ARENA_LARGE)) == [2 ** 29, 2 ** 31, 2 ** 32, 2 ** 32 + 2 ** 31, 2 ** 33, 2 ** 33 + 2 ** 31, 2 ** 34]
    assert FA.boundaries(FA.view_elements(np.float64, FA.ARENA_LARGE)) == [2 ** 29, 2 ** 31, 2 ** 32, 2 ** 32 + 2 ** 31, 2 ** 33]
    assert FA.boundaries(FA.view_elements(np.complex128, FA.ARENA_LARGE)) == [2 ** 29, 2 ** 31, 2 ** 32]
    assert FA.subtract((10, 50), [(0, 12), (20, 30), (45, 60)]) == [(12, 20), (30, 45)]
    assert FA.subtract((10, 50), []) == [(10, 50)] and FA.subtract((10, 50), [(0, 100)]) == []
    assert FA.overlaps([(0, 5), (4, 6)]) and not FA.overlaps([(0, 5), (5, 6)])
    # a run above 2^32 has its aliases under every other high byte, one that crosses 2^33 is cut there
    al = FA.alias_windows([(TWO32 + 7, TWO32 + 9)], 3 * TWO32)
    assert sorted(al) == [(7, 9), (2 * TWO32 + 7, 2 * TWO32 + 9)]
    al = FA.alias_windows([(2 * TWO32 - 2, 2 * TWO32 + 3)], 3 * TWO32)
    assert sorted(al) == [(0, 3), (TWO32 - 2, TWO32), (TWO32, TWO32 + 3), (3 * TWO32 - 2, 3 * TWO32)]
    assert FA.alias_windows([(5, 100)], 3 * TWO32) == []


def test_acc_sites_are_disjoint_and_reach_the_last_element_a_stack_can_name():
    for sizes in ([[529] * 60, [529] * 60, [529] * 12], [[91] * 60, [35] * 60, [65] * 12]):
        offs, guards, iv = G.acc_sites(sizes)
        assert not FA.overlaps(iv) and min(s for s, _ in iv) == 0
        assert max(o + sizes[2][0] for o in offs[2]) == 2 ** 31 - 1 and max(e for _, e in iv) == 2 ** 31 - 1 + FA.GUARD
        assert any(o < 2 ** 29 < o + sizes[0][0] for o in offs[0])
        assert all(any(o < FA.SLOT for o in offs[w]) and any(2 ** 28 < o < 2 ** 30 for o in offs[w]) and any(o > 2 ** 31 - FA.SLOT for o in offs[w]) for w in range(3))
