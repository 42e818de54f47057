"""The kernels of the matrix algebra between multiplies (dbcsr_amd/csrc/mm_algebra.h over the block walk of mm_block_walk.h: add, add_on_diag, trace, dot, Frobenius norm), read from the code
object of the shipping build (no GPU needed): every one is there under its name, for every data type it serves, and uses no scratch.  They stream
memory: what matters is that none of them spills, and that none keeps so many registers that fewer than four waves fit a SIMD (<= 128)."""
import pytest

from tests.test_kernel_resources import demangle, kernels_of_library

PLAIN = ["algebra_compare", "algebra_union", "algebra_emit", "diag_missing", "diag_emit"]
TYPED = {
    "algebra_add_blocks": ("double", "float", "dbcsr_amd::z64"),
    "algebra_add_flat": ("double", "float", "dbcsr_amd::z64"),
    "diag_fill": ("double", "float", "dbcsr_amd::z64"),
    "diag_shift": ("double", "float", "dbcsr_amd::z64"),
    "algebra_trace": ("double", "float", "dbcsr_amd::z64"),
    "algebra_norm2": ("double", "float", "dbcsr_amd::z64"),
    "algebra_dot": ("double", "float"),   # (the complex dot is not offered)
}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    ks = kernels_of_library(tmp_path_factory.mktemp("ops_kernels"))
    pretty = demangle(sorted(ks))
    return {pretty[n]: k for n, k in ks.items()}


def wanted():
    out = ["dbcsr_amd::%s(" % n for n in PLAIN]
    for name, types in TYPED.items():
        out += ["void dbcsr_amd::%s<%s>(" % (name, t) for t in types]
    return out


@pytest.mark.parametrize("prefix", wanted())
def test_algebra_kernel_is_there_without_scratch(kernels, prefix):
    mine = [k for n, k in kernels.items() if n.startswith(prefix)]
    assert len(mine) == 1, sorted(n for n in kernels if "algebra" in n or "diag_" in n)
    k = mine[0]
    assert k["private_segment_fixed_size"] == 0
    assert k["vgpr_count"] <= 128, k


def test_no_complex_dot_kernel(kernels):
    assert not [n for n in kernels if "algebra_dot<dbcsr_amd::z64>" in n]
