"""The kernels of the element CSR form (dbcsr_amd/csrc/mm_csr.h: csr_count, csr_emit, csr_scatter and the index kernels csr_row_slots, csr_slot_widths,
csr_crow, csr_name_blocks), read from the code object of the shipping build (no GPU needed).  DESIGN 3.18 claims: the three typed kernels are there once
per data type, the four index kernels once; none uses scratch; none needs more registers than what the build shows rounded up to the allocation granule
of 8 -- 64 / 80 / 48 for csr_count (float64, float32, complex128), 72 / 88 / 72 for csr_emit, 80 / 112 / 72 for csr_scatter, at most 24 for the index
kernels -- all at most 128, so registers allow at least four waves per SIMD; the typed kernels hold exactly one tile of 32 x 33 elements in LDS: 8448 /
4224 / 16896 bytes, at most 32 KB; the index kernels hold none.

The namespace itself contains "csr_" (dbcsr_amd::), so the kernels are matched on "dbcsr_amd::csr_"."""
import pytest

from tests.test_kernel_resources import demangle, kernels_of_library

ALL = ("double", "float", "dbcsr_amd::z64")
TYPED = ("csr_count", "csr_emit", "csr_scatter")
INDEX = ("csr_row_slots", "csr_slot_widths", "csr_crow", "csr_name_blocks")
VGPRS = {("csr_count", "double"): 64, ("csr_count", "float"): 80, ("csr_count", "dbcsr_amd::z64"): 48,
         ("csr_emit", "double"): 72, ("csr_emit", "float"): 88, ("csr_emit", "dbcsr_amd::z64"): 72,
         ("csr_scatter", "double"): 80, ("csr_scatter", "float"): 112, ("csr_scatter", "dbcsr_amd::z64"): 72}
TILE_BYTES = {"double": 32 * 33 * 8, "float": 32 * 33 * 4, "dbcsr_amd::z64": 32 * 33 * 16}
MINE = "dbcsr_amd::csr_"


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    ks = kernels_of_library(tmp_path_factory.mktemp("csr_kernels"))
    pretty = demangle(sorted(ks))
    return {pretty[n]: k for n, k in ks.items()}


def the_one(kernels, name, t):
    mine = [k for n, k in kernels.items() if n.startswith("void dbcsr_amd::%s<%s>(" % (name, t))]
    assert len(mine) == 1, sorted(n for n in kernels if MINE in n)
    return mine[0]


@pytest.mark.parametrize("t", ALL)
@pytest.mark.parametrize("name", TYPED)
def test_csr_kernel_fits_its_registers_without_scratch(kernels, name, t):
    k = the_one(kernels, name, t)
    print(name, t, {f: k[f] for f in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
    assert k["private_segment_fixed_size"] == 0
    assert k["vgpr_count"] <= VGPRS[(name, t)] <= 128, k
    assert k["group_segment_fixed_size"] == TILE_BYTES[t] <= 32 * 1024, k


@pytest.mark.parametrize("name", INDEX)
def test_csr_index_kernel_is_small(kernels, name):
    mine = [k for n, k in kernels.items() if n.startswith("dbcsr_amd::%s(" % name)]
    assert len(mine) == 1, sorted(n for n in kernels if MINE in n)
    k = mine[0]
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_count"] <= 24 and k["group_segment_fixed_size"] == 0, k


def test_nothing_else_of_the_csr_conversion_ships(kernels):
    assert len([n for n in kernels if MINE in n]) == len(TYPED) * len(ALL) + len(INDEX)


def test_the_names_keep_clear_of_the_other_resource_tests(kernels):
    """no new kernel carries a word that the earlier resource tests count kernels by"""
    mine = [n for n in kernels if MINE in n]
    for word in ("dense_", "algebra", "blocklist_", "elementwise_", "submatrix_", "block_scale", "block_inverse", "block_diag_"):
        assert not [n for n in mine if word in n], word
