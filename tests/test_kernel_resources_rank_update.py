"""The kernels of the rank-k update on the stored pattern (dbcsr_amd/csrc/mm_rank_update.h: algebra_rank_update_blocks, algebra_rank_update_scale), read
from the code object of the shipping build (no GPU needed).  DESIGN 3.11 claims: each is there once per data type; none uses scratch -- the accumulators
of two 16 x 16 tiles (complex data: four chains) and the runs of X and Y stay in registers; the update kernel needs no more than 96 registers for
float64 (five waves per SIMD of the 512 a SIMD has, allocated in eights), 104 for float32 and 128 for complex data (four waves), and no LDS at all (its
operands never pass through LDS); the scaling pass no more than 64."""
import pytest

from tests.test_kernel_resources import demangle, kernels_of_library

ALL = ("double", "float", "dbcsr_amd::z64")
NAMES = ("algebra_rank_update_blocks", "algebra_rank_update_scale")
VGPRS = {("algebra_rank_update_blocks", "double"): 96, ("algebra_rank_update_blocks", "float"): 104, ("algebra_rank_update_blocks", "dbcsr_amd::z64"): 128}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    ks = kernels_of_library(tmp_path_factory.mktemp("rank_update_kernels"))
    pretty = demangle(sorted(ks))
    return {pretty[n]: k for n, k in ks.items()}


def the_one(kernels, name, t):
    mine = [k for n, k in kernels.items() if n.startswith("void dbcsr_amd::%s<%s>(" % (name, t))]
    assert len(mine) == 1, sorted(n for n in kernels if "algebra_rank_update" in n)
    return mine[0]


@pytest.mark.parametrize("t", ALL)
@pytest.mark.parametrize("name", NAMES)
def test_rank_update_kernel_fits_its_occupancy_without_scratch(kernels, name, t):
    k = the_one(kernels, name, t)
    print(name, t, {f: k[f] for f in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
    assert k["private_segment_fixed_size"] == 0
    assert k["vgpr_count"] <= VGPRS.get((name, t), 64), k
    assert k["group_segment_fixed_size"] == 0, k


def test_nothing_else_of_the_update_ships(kernels):
    assert len([n for n in kernels if "algebra_rank_update" in n]) == len(NAMES) * len(ALL)


def test_the_other_products_keep_their_counts(kernels):
    """no new kernel carries the name of the matrix-vector product or of the matrix times several vectors: three kernels per type each, as before"""
    assert len([n for n in kernels if "algebra_matvec" in n]) == 3 * len(ALL)
    assert len([n for n in kernels if "algebra_multivec" in n]) == 3 * len(ALL)
