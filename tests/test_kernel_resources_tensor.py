"""The kernel of the block-sparse tensors (dbcsr_amd/csrc/mm_tensor.h: tensor_permute_blocks), read from the code object of the shipping build (no GPU
needed).  DESIGN 3.19 claims: it is there once per data type; it uses no scratch -- the reduced move of a block is nine integers that are picked with
selects, never an indexed array; it holds exactly one tile of 32 x 33 elements in LDS: 8448 / 4224 / 16896 bytes, at most 32 * 33 * 16; registers allow
at least four waves per SIMD (at most 128).  Nothing else named tensor_ ships, and the other families keep their counts."""
import pytest

from tests.test_kernel_resources import demangle, kernels_of_library
from tests.test_kernel_resources_block_scale import OTHERS

ALL = ("double", "float", "dbcsr_amd::z64")
NAMES = ("tensor_permute_blocks",)
TILE_BYTES = {"double": 32 * 33 * 8, "float": 32 * 33 * 4, "dbcsr_amd::z64": 32 * 33 * 16}
MINE = "dbcsr_amd::tensor_"


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    ks = kernels_of_library(tmp_path_factory.mktemp("tensor_kernels"))
    pretty = demangle(sorted(ks))
    return {pretty[n]: k for n, k in ks.items()}


@pytest.mark.parametrize("t", ALL)
@pytest.mark.parametrize("name", NAMES)
def test_tensor_kernel_ships_once_without_scratch(kernels, name, t):
    mine = [k for n, k in kernels.items() if n.startswith("void dbcsr_amd::%s<%s>(" % (name, t))]
    assert len(mine) == 1, sorted(n for n in kernels if "tensor_" in n)
    k = mine[0]
    print(name, t, {f: k[f] for f in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
    assert k["private_segment_fixed_size"] == 0, k
    assert k["group_segment_fixed_size"] == TILE_BYTES[t] <= 32 * 33 * 16, k
    assert k["vgpr_count"] <= 128, k


def test_nothing_else_named_tensor_ships(kernels):
    assert len([n for n in kernels if "tensor_" in n]) == len(NAMES) * len(ALL)
    assert len([n for n in kernels if MINE in n]) == len(NAMES) * len(ALL)


def test_the_names_keep_clear_of_the_other_resource_tests(kernels):
    """the new kernel carries no word that the earlier resource tests count kernels by"""
    mine = [n for n in kernels if MINE in n]
    for word in ("dense_", "algebra", "blocklist_", "elementwise_", "submatrix_", "block_scale", "block_inverse", "block_diag_", "dbcsr_amd::csr_"):
        assert not [n for n in mine if word in n], word


def test_the_other_families_keep_their_counts(kernels):
    for family, count in OTHERS.items():
        assert len([n for n in kernels if family in n]) == count, family
