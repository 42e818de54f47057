"""The kernels of the norms and vectors (dbcsr_amd/csrc/mm_algebra.h over the block walk of mm_block_walk.h: row / column sums, max |x|, the diagonal as a vector, scale by vector), read from the
code object of the shipping build (no GPU needed): every one is there under its name, for every data type it serves, and uses no scratch.  They stream
memory: what matters is that none of them spills (the row sums keep 2 V - 1 accumulators per lane and choose among them by the block's alignment), and
that none keeps so many registers that fewer than four waves fit a SIMD (<= 128)."""
import pytest

from tests.test_kernel_resources import demangle, kernels_of_library

ALL = ("double", "float", "dbcsr_amd::z64")
PLAIN = ["algebra_vec_combine", "algebra_col_list", "algebra_max_final"]
TYPED = ["algebra_row_sums", "algebra_col_sums", "algebra_maxabs", "diag_get", "diag_set", "algebra_scale_by_vector"]


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    ks = kernels_of_library(tmp_path_factory.mktemp("norm_kernels"))
    pretty = demangle(sorted(ks))
    return {pretty[n]: k for n, k in ks.items()}


def typed_prefix(name, t):
    """(the column sums carry a variant number: 0 ships, the others exist in the lab build only)"""
    return "void dbcsr_amd::%s<%s%s>(" % (name, t, ", 0" if name == "algebra_col_sums" else "")


def wanted():
    return ["dbcsr_amd::%s(" % n for n in PLAIN] + [typed_prefix(n, t) for n in TYPED for t in ALL]


@pytest.mark.parametrize("prefix", wanted())
def test_norm_kernel_is_there_without_scratch(kernels, prefix):
    mine = [k for n, k in kernels.items() if n.startswith(prefix)]
    assert len(mine) == 1, sorted(n for n in kernels if "algebra" in n or "diag_" in n)
    k = mine[0]
    assert k["private_segment_fixed_size"] == 0
    assert k["vgpr_count"] <= 128, k


def test_only_the_shipping_form_of_the_column_sums_ships(kernels):
    assert len([n for n in kernels if "algebra_col_sums<" in n]) == len(ALL)


def test_lds_slices_leave_room_for_many_workgroups(kernels):
    """the row sums' accumulators (at most 7 x 64 doubles per wave) and the column sums' staging piece (1024 doubles per wave): <= 32 KB per workgroup"""
    for name in ("algebra_row_sums", "algebra_col_sums"):
        for t in ALL:
            k = [k for n, k in kernels.items() if n.startswith(typed_prefix(name, t))][0]
            assert 0 < k["group_segment_fixed_size"] <= 32768, k
