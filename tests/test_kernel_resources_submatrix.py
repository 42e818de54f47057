"""The kernels of the submatrix method (dbcsr_amd/csrc/mm_submatrix.h: submatrix_gather, submatrix_scatter), read from the code object of the shipping build
(no GPU needed).  DESIGN 3.15 claims: the two kernels are there once per data type and nothing else begins with submatrix_; none uses scratch; none needs
more registers than what the build shows rounded up to the allocation granule of 8 -- 64 / 80 / 48 for submatrix_gather (float64, float32, complex128),
56 / 96 / 40 for submatrix_scatter -- all at most 128, so registers allow at least four waves per SIMD; each holds exactly the one tile of 32 x 33
elements in LDS: 8448 / 4224 / 16896 bytes.  The counts the earlier resource tests rely on are unchanged."""
import pytest

from tests.test_kernel_resources import demangle, kernels_of_library

ALL = ("double", "float", "dbcsr_amd::z64")
NAMES = ("submatrix_gather", "submatrix_scatter")
VGPRS = {("submatrix_gather", "double"): 64, ("submatrix_gather", "float"): 80, ("submatrix_gather", "dbcsr_amd::z64"): 48,
         ("submatrix_scatter", "double"): 56, ("submatrix_scatter", "float"): 96, ("submatrix_scatter", "dbcsr_amd::z64"): 40}
TILE_BYTES = {"double": 32 * 33 * 8, "float": 32 * 33 * 4, "dbcsr_amd::z64": 32 * 33 * 16}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    ks = kernels_of_library(tmp_path_factory.mktemp("submatrix_kernels"))
    pretty = demangle(sorted(ks))
    return {pretty[n]: k for n, k in ks.items()}


def the_one(kernels, name, t):
    mine = [k for n, k in kernels.items() if n.startswith("void dbcsr_amd::%s<%s>(" % (name, t))]
    assert len(mine) == 1, sorted(n for n in kernels if "submatrix_" in n)
    return mine[0]


@pytest.mark.parametrize("t", ALL)
@pytest.mark.parametrize("name", NAMES)
def test_submatrix_kernel_fits_its_registers_without_scratch(kernels, name, t):
    k = the_one(kernels, name, t)
    print(name, t, {f: k[f] for f in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
    assert k["private_segment_fixed_size"] == 0
    assert k["vgpr_count"] <= VGPRS[(name, t)] <= 128, k
    assert VGPRS[(name, t)] - k["vgpr_count"] < 8, "the bound is what the build shows, rounded up to 8"
    assert k["group_segment_fixed_size"] == TILE_BYTES[t], k


def test_nothing_else_of_the_submatrix_method_ships(kernels):
    mine = [n for n in kernels if "submatrix_" in n]
    assert len(mine) == len(NAMES) * len(ALL), mine
    assert all(n.startswith("void dbcsr_amd::submatrix_gather<") or n.startswith("void dbcsr_amd::submatrix_scatter<") for n in mine), mine


def test_the_other_kernels_keep_their_counts(kernels):
    """no new kernel carries a name that the earlier resource tests count by"""
    mine = [n for n in kernels if "submatrix_" in n]
    for word in ("algebra", "dense_", "diag_", "block_inverse", "block_diag", "block_scale"):
        assert not [n for n in mine if word in n.split("(")[0]], word
    assert len([n for n in kernels if "dbcsr_amd::dense_" in n]) == 3 * len(ALL) + 1
    assert len([n for n in kernels if "block_inverse_" in n]) == 2 * len(ALL)
    assert len([n for n in kernels if "block_diag_" in n]) == len(ALL) + 1
    assert len([n for n in kernels if "algebra_matvec" in n]) == 3 * len(ALL)
    assert len([n for n in kernels if "algebra_multivec" in n]) == 3 * len(ALL)
    assert len([n for n in kernels if "algebra_rank_update" in n]) == 2 * len(ALL)
    assert len([n for n in kernels if "algebra_col_sums<" in n]) == len(ALL)
    for name in ("diag_get<", "diag_set<", "diag_fill<", "diag_shift<"):
        assert len([n for n in kernels if n.startswith("void dbcsr_amd::" + name)]) == len(ALL), name
