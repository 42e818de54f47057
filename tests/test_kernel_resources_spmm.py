"""The kernels of the matrix times a dense matrix (dbcsr_amd/csrc/mm_spmm.h: spmm_product, spmm_scale), read from the code object of the shipping build (no
GPU needed).  DESIGN 3.21 claims: spmm_product is there once per data type and layout (2 x 3 instances), spmm_scale once per data type; none uses
scratch -- four strips of accumulators (complex data: eight), the runs of X and the operand of the block stay in registers; the product kernel needs no
more than 128 registers for any data type (four waves per SIMD of the 512 registers a SIMD has: four workgroups per CU, whose 4 x 24 KB of LDS fit
the CU's 160 KB) and 24 KB of LDS per workgroup -- at most 32 KB --; the scaling pass no more than 32 registers and no LDS."""
import pytest

from tests.test_kernel_resources import demangle, kernels_of_library

ALL = ("double", "float", "dbcsr_amd::z64")
LAYOUTS = (0, 1)
VGPRS = {"double": 128, "float": 128, "dbcsr_amd::z64": 128}
LDS_MAX = 32768


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    ks = kernels_of_library(tmp_path_factory.mktemp("spmm_kernels"))
    pretty = demangle(sorted(ks))
    return {pretty[n]: k for n, k in ks.items()}


def the_one(kernels, prefix):
    mine = [k for n, k in kernels.items() if n.startswith(prefix)]
    assert len(mine) == 1, sorted(n for n in kernels if "spmm_" in n)
    return mine[0]


def show(name, k):
    print(name, {f: k[f] for f in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("t", ALL)
def test_product_kernel_fits_its_budget_without_scratch(kernels, t, layout):
    k = the_one(kernels, "void dbcsr_amd::spmm_product<%s, %d>(" % (t, layout))
    show("spmm_product<%s, %d>" % (t, layout), k)
    assert k["private_segment_fixed_size"] == 0
    assert k["vgpr_count"] <= VGPRS[t], k
    assert 0 < k["group_segment_fixed_size"] <= LDS_MAX, k


@pytest.mark.parametrize("t", ALL)
def test_scale_kernel_is_small(kernels, t):
    k = the_one(kernels, "void dbcsr_amd::spmm_scale<%s>(" % t)
    show("spmm_scale<%s>" % t, k)
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_count"] <= 32 and k["group_segment_fixed_size"] == 0, k


def test_nothing_else_of_it_ships(kernels):
    assert len([n for n in kernels if "spmm_" in n]) == len(ALL) * len(LAYOUTS) + len(ALL)


def test_the_names_other_resource_tests_count_are_unchanged(kernels):
    """a new kernel carries none of the substrings by which the other resource tests count their kernels, and the products they count keep their numbers"""
    for n in kernels:
        if "spmm_" in n:
            for word in ("algebra", "dense_", "tensor_", "block_scale", "block_inverse", "block_diag_", "submatrix_", "elementwise_", "blocklist_"):
                assert word not in n, (word, n)
    assert len([n for n in kernels if "algebra_matvec" in n]) == 3 * len(ALL)
    assert len([n for n in kernels if "algebra_multivec" in n]) == 3 * len(ALL)
    assert len([n for n in kernels if "algebra_rank_update" in n]) == 2 * len(ALL)
