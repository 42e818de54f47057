"""The kernels of the block lists (dbcsr_amd/csrc/mm_blocklist.h), read from the code object of the shipping build (no GPU needed).  DESIGN 3.17 claims:
blocklist_put and blocklist_get are there once per data type, blocklist_mark, blocklist_named_nze, blocklist_locate, blocklist_slot and blocklist_order
once; none uses scratch or LDS (the segments are ordered by ranking in registers, through global memory).  The register bars are what the cross-compiled
code object shows, rounded up to the next allocation step of eight:

    kernel            double    float     z64             kernel                 registers
    blocklist_put     34 -> 40  38 -> 40  34 -> 40        blocklist_mark         10 -> 16
    blocklist_get     22 -> 24  22 -> 24  16 -> 16        blocklist_named_nze    12 -> 16
                                                          blocklist_locate       10 -> 16
                                                          blocklist_slot          6 -> 8
                                                          blocklist_order        18 -> 24

The reserve reuses the union add's kernels and the copy onto a pattern by launching them: their counts, pinned elsewhere, stay."""
import pytest

from tests.test_kernel_resources import demangle, kernels_of_library

D, F, Z = "double", "float", "dbcsr_amd::z64"
TYPED = {("blocklist_put", D): 40, ("blocklist_put", F): 40, ("blocklist_put", Z): 40,
         ("blocklist_get", D): 24, ("blocklist_get", F): 24, ("blocklist_get", Z): 16}
UNTYPED = {"blocklist_mark": 16, "blocklist_named_nze": 16, "blocklist_locate": 16, "blocklist_slot": 8, "blocklist_order": 24}
OTHERS = {"algebra_union": 1, "algebra_emit": 1, "algebra_add_blocks": 3, "algebra_add_flat": 3, "algebra_compare": 1, "elementwise_copy_onto": 3,
          "elementwise_": 13, "bitmap_from_index": 1, "block_sizes_rows": 1}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    ks = kernels_of_library(tmp_path_factory.mktemp("blocklist_kernels"))
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
    assert len(mine) == 1, sorted(n for n in kernels if "blocklist_" in n)
    check(mine[0], TYPED[(name, t)])


@pytest.mark.parametrize("name", sorted(UNTYPED))
def test_untyped_kernel_is_there_once_without_scratch_or_lds(kernels, name):
    mine = [k for n, k in kernels.items() if n.startswith("dbcsr_amd::%s(" % name)]
    assert len(mine) == 1, sorted(n for n in kernels if "blocklist_" in n)
    check(mine[0], UNTYPED[name])


def test_nothing_else_of_it_ships(kernels):
    assert len([n for n in kernels if "blocklist_" in n]) == len(TYPED) + len(UNTYPED)


def test_the_kernels_the_reserve_launches_keep_their_counts(kernels):
    for family, count in OTHERS.items():
        assert len([n for n in kernels if family in n]) == count, family
