"""The kernels of the block diagonal applied to a matrix (dbcsr_amd/csrc/mm_block_scale.h: block_scale_left, block_scale_right, block_scale_zero), read
from the code object of the shipping build (no GPU needed).  DESIGN 3.14 claims: each is there once per data type; none uses scratch or LDS -- the
accumulators of the six 16 x 16 tiles of a strip (48 registers, complex data 96) and the operands of a step stay in registers; block_scale_left needs no
more than 80 registers for float64 and float32 (six waves per SIMD of the 512 a SIMD has, allocated in eights) and 168 for complex data (three waves);
block_scale_right, which looks its diagonal block up per block, 136 for float64 (three waves), 128 for float32 (four) and 216 for complex data (two);
block_scale_zero no more than 32.  The kernels of the other families keep their counts."""
import pytest

from tests.test_kernel_resources import demangle, kernels_of_library

ALL = ("double", "float", "dbcsr_amd::z64")
NAMES = ("block_scale_left", "block_scale_right", "block_scale_zero")
VGPRS = {("block_scale_left", "double"): 80, ("block_scale_left", "float"): 80, ("block_scale_left", "dbcsr_amd::z64"): 168,
         ("block_scale_right", "double"): 136, ("block_scale_right", "float"): 128, ("block_scale_right", "dbcsr_amd::z64"): 216}
OTHERS = {"block_inverse_": 6, "block_diag_": 4, "algebra_matvec": 9, "algebra_multivec": 9, "algebra_rank_update": 6, "dbcsr_amd::dense_": 10}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    ks = kernels_of_library(tmp_path_factory.mktemp("block_scale_kernels"))
    pretty = demangle(sorted(ks))
    return {pretty[n]: k for n, k in ks.items()}


@pytest.mark.parametrize("t", ALL)
@pytest.mark.parametrize("name", NAMES)
def test_block_scale_kernel_fits_its_occupancy_without_scratch(kernels, name, t):
    mine = [k for n, k in kernels.items() if n.startswith("void dbcsr_amd::%s<%s>(" % (name, t))]
    assert len(mine) == 1, sorted(n for n in kernels if "block_scale" in n)
    k = mine[0]
    print(name, t, {f: k[f] for f in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
    assert k["private_segment_fixed_size"] == 0
    assert k["vgpr_count"] <= VGPRS.get((name, t), 32), k
    assert k["group_segment_fixed_size"] == 0, k


def test_nothing_else_of_it_ships(kernels):
    assert len([n for n in kernels if "block_scale" in n]) == len(NAMES) * len(ALL)


def test_the_other_families_keep_their_counts(kernels):
    for family, count in OTHERS.items():
        assert len([n for n in kernels if family in n]) == count, family
