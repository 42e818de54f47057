"""The kernels of the block diagonal (dbcsr_amd/csrc/mm_block_inverse.h: block_inverse_wave, block_inverse_wide, block_diag_copy, block_diag_find), read
from the code object of the shipping build (no GPU needed).  DESIGN 3.12 claims: the two inversion kernels and the copy are there once per data type, the
index kernel once; none uses scratch (the choice between two complex values is made part by part, and no complex value waits in a stack slot); the
inversion kernels need no more registers than what the build shows rounded up to the allocation granule of 8 -- 48 / 56 / 56 for the wave kernel (float64,
float32, complex128) and 40 / 40 / 48 for the workgroup kernel, all at most 64, so registers allow eight waves per SIMD and the LDS of the launch, not
the registers, sets the occupancy; their LDS is dynamic (sized by the caller's bound on the block dimension), none is static."""
import pytest

from tests.test_kernel_resources import demangle, kernels_of_library

ALL = ("double", "float", "dbcsr_amd::z64")
TYPED = ("block_inverse_wave", "block_inverse_wide", "block_diag_copy")
VGPRS = {("block_inverse_wave", "double"): 48, ("block_inverse_wave", "float"): 56, ("block_inverse_wave", "dbcsr_amd::z64"): 56,
         ("block_inverse_wide", "double"): 40, ("block_inverse_wide", "float"): 40, ("block_inverse_wide", "dbcsr_amd::z64"): 48,
         ("block_diag_copy", "double"): 24, ("block_diag_copy", "float"): 40, ("block_diag_copy", "dbcsr_amd::z64"): 16}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    ks = kernels_of_library(tmp_path_factory.mktemp("block_inverse_kernels"))
    pretty = demangle(sorted(ks))
    return {pretty[n]: k for n, k in ks.items()}


def the_one(kernels, name, t):
    mine = [k for n, k in kernels.items() if n.startswith("void dbcsr_amd::%s<%s>(" % (name, t))]
    assert len(mine) == 1, sorted(n for n in kernels if "block_inverse" in n or "block_diag" in n)
    return mine[0]


@pytest.mark.parametrize("t", ALL)
@pytest.mark.parametrize("name", TYPED)
def test_block_diagonal_kernel_fits_its_registers_without_scratch(kernels, name, t):
    k = the_one(kernels, name, t)
    print(name, t, {f: k[f] for f in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
    assert k["private_segment_fixed_size"] == 0
    assert k["vgpr_count"] <= VGPRS[(name, t)] <= 64, k
    assert k["group_segment_fixed_size"] == 0, k


def test_nothing_else_of_the_block_diagonal_ships(kernels):
    assert len([n for n in kernels if "block_inverse_" in n]) == 2 * len(ALL)
    assert len([n for n in kernels if "block_diag_" in n]) == len(ALL) + 1
    find = [k for n, k in kernels.items() if n.startswith("dbcsr_amd::block_diag_find(")]
    assert len(find) == 1 and find[0]["private_segment_fixed_size"] == 0 and find[0]["vgpr_count"] <= 16


def test_the_other_kernels_keep_their_counts(kernels):
    """no new kernel carries a name that the earlier resource tests count by"""
    assert len([n for n in kernels if "algebra_matvec" in n]) == 3 * len(ALL)
    assert len([n for n in kernels if "algebra_multivec" in n]) == 3 * len(ALL)
    assert len([n for n in kernels if "algebra_rank_update" in n]) == 2 * len(ALL)
    assert len([n for n in kernels if "algebra_col_sums<" in n]) == len(ALL)
    for name in ("diag_get<", "diag_set<", "diag_fill<", "diag_shift<"):
        assert len([n for n in kernels if n.startswith("void dbcsr_amd::" + name)]) == len(ALL), name
