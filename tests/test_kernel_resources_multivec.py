"""The kernels of the matrix times several dense vectors (dbcsr_amd/csrc/mm_multivec.h: algebra_multivec_rows, algebra_multivec_cols,
algebra_multivec_combine), read from the code object of the shipping build (no GPU needed): each is there once per data type, uses no scratch -- the 16
accumulators of a lane stay in registers -- and no more than 128 registers (four waves per SIMD).  The two passes size their LDS at the launch (8 KB per
wave of the workgroup, at most four waves: dbcsr_amd/csrc/mm_multivec.h asserts the 32 KB at compile time), so the code object records no fixed LDS for
them: whatever it records must stay within the 32 KB all the same."""
import pytest

from tests.test_kernel_resources import demangle, kernels_of_library

ALL = ("double", "float", "dbcsr_amd::z64")
NAMES = ("algebra_multivec_rows", "algebra_multivec_cols", "algebra_multivec_combine")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    ks = kernels_of_library(tmp_path_factory.mktemp("multivec_kernels"))
    pretty = demangle(sorted(ks))
    return {pretty[n]: k for n, k in ks.items()}


def the_one(kernels, name, t):
    mine = [k for n, k in kernels.items() if n.startswith("void dbcsr_amd::%s<%s>(" % (name, t))]
    assert len(mine) == 1, sorted(n for n in kernels if "algebra_multivec" in n)
    return mine[0]


@pytest.mark.parametrize("t", ALL)
@pytest.mark.parametrize("name", NAMES)
def test_multivec_kernel_is_there_without_scratch(kernels, name, t):
    k = the_one(kernels, name, t)
    print(name, t, {f: k[f] for f in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
    assert k["private_segment_fixed_size"] == 0
    assert k["vgpr_count"] <= 128, k


@pytest.mark.parametrize("t", ALL)
@pytest.mark.parametrize("name", NAMES[:2])
def test_lds_stays_within_32_kb(kernels, name, t):
    assert 0 <= the_one(kernels, name, t)["group_segment_fixed_size"] <= 32768


def test_nothing_else_of_the_product_ships(kernels):
    assert len([n for n in kernels if "algebra_multivec" in n]) == len(NAMES) * len(ALL)


def test_the_matvec_kernels_are_not_counted_among_them(kernels):
    """the matrix-vector product keeps its own three kernels per type: no new kernel carries its name"""
    assert len([n for n in kernels if "algebra_matvec" in n]) == 3 * len(ALL)
