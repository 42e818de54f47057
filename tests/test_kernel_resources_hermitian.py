"""The kernel that ships for the twin / desymmetrize fill of complex_8 matrices (dbcsr_amd_bcsr_twin_apply with 16-byte elements), read from the code
object of the shipping build (no GPU needed): twin_fill_z64 -- the form that won the measurement of profiles/hermitian_twin.txt -- is there under its
stable name, uses no scratch, and its LDS (one 32 x 33 element image per wave, four waves per workgroup) fits the CU and keeps every image 16-byte
aligned."""
from tests.test_kernel_resources import demangle, kernels_of_library


def test_complex_twin_fill_kernel(tmp_path):
    ks = kernels_of_library(tmp_path)
    pretty = demangle(sorted(ks))
    mine = [k for n, k in ks.items() if pretty[n].startswith("dbcsr_amd::twin_fill_z64(")]
    assert len(mine) == 1, sorted(v for v in pretty.values() if "twin" in v or "desym" in v)
    k = mine[0]
    assert k["private_segment_fixed_size"] == 0
    lds = k["group_segment_fixed_size"]   # of a workgroup of four waves
    assert 0 < lds <= 160 * 1024 and lds % 16 == 0 and (lds // 4) % 16 == 0
    assert lds == 4 * 32 * 33 * 16
