"""The kernels of the element-wise operations on two patterns (dbcsr_amd/csrc/mm_elementwise.h), read from the code object of the shipping build (no GPU
needed).  DESIGN 3.16 claims: elementwise_mul_blocks, elementwise_mul_flat and elementwise_copy_onto are there once per data type,
elementwise_function once per real type, elementwise_match and elementwise_emit once; none uses scratch or LDS.  The register bars are what the
cross-compiled code object shows, rounded up to the next allocation step of eight:

    kernel                      double   float   z64            kernel               registers
    elementwise_mul_blocks      43 -> 48 45 -> 48 30 -> 32      elementwise_match    18 -> 24
    elementwise_mul_flat        12 -> 16 16 -> 16 16 -> 16      elementwise_emit     30 -> 32
    elementwise_copy_onto       32 -> 32 32 -> 32 22 -> 24
    elementwise_function        78 -> 80 106 -> 112   --

(elementwise_function chooses the function once per wave, outside the block walk: it needs the registers of the largest of the twelve, not of all of
them -- six waves per SIMD for float64, four for float32, whose pack holds four elements.)  The kernels of the other families keep their counts, the add's among them."""
import pytest

from tests.test_kernel_resources import demangle, kernels_of_library

D, F, Z = "double", "float", "dbcsr_amd::z64"
TYPED = {("elementwise_mul_blocks", D): 48, ("elementwise_mul_blocks", F): 48, ("elementwise_mul_blocks", Z): 32,
         ("elementwise_mul_flat", D): 16, ("elementwise_mul_flat", F): 16, ("elementwise_mul_flat", Z): 16,
         ("elementwise_copy_onto", D): 32, ("elementwise_copy_onto", F): 32, ("elementwise_copy_onto", Z): 24,
         ("elementwise_function", D): 80, ("elementwise_function", F): 112}
UNTYPED = {"elementwise_match": 24, "elementwise_emit": 32}
OTHERS = {"algebra_matvec": 9, "algebra_multivec": 9, "algebra_rank_update": 6, "algebra_col_sums<": 3, "block_diag_": 4, "block_inverse_": 6,
          "block_scale": 9, "dbcsr_amd::dense_": 10, "submatrix_": 6, "algebra_union": 1, "algebra_emit": 1, "algebra_add_blocks": 3,
          "algebra_add_flat": 3, "algebra_compare": 1}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    ks = kernels_of_library(tmp_path_factory.mktemp("elementwise_kernels"))
    pretty = demangle(sorted(ks))
    return {pretty[n]: k for n, k in ks.items()}


def check(k, bar):
    print({f: k[f] for f in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
    assert k["private_segment_fixed_size"] == 0, k
    assert k["group_segment_fixed_size"] == 0, k
    assert k["vgpr_count"] <= bar, k


@pytest.mark.parametrize("name,t", sorted(TYPED))
def test_typed_kernel_is_there_once_without_scratch_or_lds(kernels, name, t):
    mine = [k for n, k in kernels.items() if n.startswith("void dbcsr_amd::%s<%s>(" % (name, t))]
    assert len(mine) == 1, sorted(n for n in kernels if "elementwise_" in n)
    check(mine[0], TYPED[(name, t)])


@pytest.mark.parametrize("name", sorted(UNTYPED))
def test_untyped_kernel_is_there_once_without_scratch_or_lds(kernels, name):
    mine = [k for n, k in kernels.items() if n.startswith("dbcsr_amd::%s(" % name)]
    assert len(mine) == 1, sorted(n for n in kernels if "elementwise_" in n)
    check(mine[0], UNTYPED[name])


def test_nothing_else_of_it_ships(kernels):
    assert len([n for n in kernels if "elementwise_" in n]) == len(TYPED) + len(UNTYPED)


def test_the_other_families_keep_their_counts(kernels):
    for family, count in OTHERS.items():
        assert len([n for n in kernels if family in n]) == count, family
