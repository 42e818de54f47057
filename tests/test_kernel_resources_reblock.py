"""The kernels of re-blocking (dbcsr_amd/csrc/mm_reblock.h: reblock_gather and the index kernels reblock_count_pieces, reblock_name_pieces), read from the
code object of the shipping build (no GPU needed).  DESIGN 3.20 claims: reblock_gather is there once per data type, the two index kernels once; none uses
scratch; none needs more registers than what the build shows rounded up to the allocation granule of 8 -- 64 / 56 / 40 for reblock_gather (float64,
float32, complex128), at most 24 for the index kernels -- all at most 128, so registers allow at least four waves per SIMD; reblock_gather holds exactly
its lookup table in LDS -- 32 x 32 data offsets of 8 bytes (the source block of every pair of slots), as many column bases (where each column of the
tile begins inside the source block of every row slot) and seven lists of 32 integers that lead an element of the tile to its entry (per row and per
column the slot and the place inside the source block; per slot the source block row, the source block column and the leading dimension): 17280 bytes
whatever the type, at most 32 KB -- and no tile of elements: nothing is staged; the index kernels hold no LDS."""
import pytest

from tests.test_kernel_resources import demangle, kernels_of_library

ALL = ("double", "float", "dbcsr_amd::z64")
INDEX = ("reblock_count_pieces", "reblock_name_pieces")
VGPRS = {"double": 64, "float": 56, "dbcsr_amd::z64": 40}
TABLE_BYTES = 2 * 32 * 32 * 8 + 7 * 32 * 4
MINE = "reblock_"


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    ks = kernels_of_library(tmp_path_factory.mktemp("reblock_kernels"))
    pretty = demangle(sorted(ks))
    return {pretty[n]: k for n, k in ks.items()}


@pytest.mark.parametrize("t", ALL)
def test_reblock_gather_fits_its_registers_without_scratch(kernels, t):
    mine = [k for n, k in kernels.items() if n.startswith("void dbcsr_amd::reblock_gather<%s>(" % t)]
    assert len(mine) == 1, sorted(n for n in kernels if MINE in n)
    k = mine[0]
    print(t, {f: k[f] for f in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
    assert k["private_segment_fixed_size"] == 0
    assert k["vgpr_count"] <= VGPRS[t] <= 128, k
    assert k["group_segment_fixed_size"] == TABLE_BYTES <= 32 * 1024, k


@pytest.mark.parametrize("name", INDEX)
def test_reblock_index_kernel_is_small(kernels, name):
    mine = [k for n, k in kernels.items() if n.startswith("dbcsr_amd::%s(" % name)]
    assert len(mine) == 1, sorted(n for n in kernels if MINE in n)
    k = mine[0]
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_count"] <= 24 <= 128 and k["group_segment_fixed_size"] == 0, k


def test_nothing_else_of_reblocking_ships(kernels):
    assert len([n for n in kernels if MINE in n]) == len(ALL) + len(INDEX)


def test_the_names_keep_clear_of_the_other_resource_tests(kernels):
    """no new kernel, and no struct in its signature, carries a word that the earlier resource tests count kernels by"""
    mine = [n for n in kernels if MINE in n]
    assert mine
    for word in ("algebra", "diag_", "dense_", "blocklist_", "elementwise_", "submatrix_", "block_scale", "block_inverse", "block_diag", "tensor_",
                 "dbcsr_amd::csr_", "twin_fill"):
        assert not [n for n in mine if word in n], word
