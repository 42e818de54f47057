"""The kernels of the matrix-vector product (dbcsr_amd/csrc/mm_algebra.h over the block walk of mm_block_walk.h: algebra_matvec_rows, algebra_matvec_cols, algebra_matvec_combine), read from
the code object of the shipping build (no GPU needed): each is there once per data type, uses no scratch and no more than 128 registers (four waves
per SIMD), and the two passes keep their LDS -- the row pass' accumulators at the end of a block row, the column pass' staged piece of 1024 real or 512
complex terms per wave -- within the 32 KB per workgroup that tests/test_kernel_resources_norms.py sets for the sums they are made from."""
import pytest

from tests.test_kernel_resources import demangle, kernels_of_library

ALL = ("double", "float", "dbcsr_amd::z64")
NAMES = ("algebra_matvec_rows", "algebra_matvec_cols", "algebra_matvec_combine")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    ks = kernels_of_library(tmp_path_factory.mktemp("matvec_kernels"))
    pretty = demangle(sorted(ks))
    return {pretty[n]: k for n, k in ks.items()}


def the_one(kernels, name, t):
    mine = [k for n, k in kernels.items() if n.startswith("void dbcsr_amd::%s<%s>(" % (name, t))]
    assert len(mine) == 1, sorted(n for n in kernels if "algebra_matvec" in n)
    return mine[0]


@pytest.mark.parametrize("t", ALL)
@pytest.mark.parametrize("name", NAMES)
def test_matvec_kernel_is_there_without_scratch(kernels, name, t):
    k = the_one(kernels, name, t)
    assert k["private_segment_fixed_size"] == 0
    assert k["vgpr_count"] <= 128, k


@pytest.mark.parametrize("t", ALL)
@pytest.mark.parametrize("name", NAMES[:2])
def test_lds_slices_leave_room_for_many_workgroups(kernels, name, t):
    assert 0 < the_one(kernels, name, t)["group_segment_fixed_size"] <= 32768


def test_nothing_else_of_the_product_ships(kernels):
    assert len([n for n in kernels if "algebra_matvec" in n]) == len(NAMES) * len(ALL)
