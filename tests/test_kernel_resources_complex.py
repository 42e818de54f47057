"""Register, scratch and LDS budget of the complex_8 block kernels mm_numeric_z64<MA,NC> (dbcsr_amd/csrc/mm_numeric_z64.h), read from the
code objects inside the shipping build (no GPU needed): one kernel per (MA, NC) in 1 ... 4 -- never a switch inside one kernel --, none
with scratch, each within two waves per SIMD, and the static LDS plus the dynamic slice the kernel choice asks for at four waves per
workgroup within the CU's 160 KB."""
import re

from tests.test_kernel_resources import demangle, kernels_of_library
from tests.test_numeric_choice_complex import choose

LDS_PER_CU = 160 * 1024


def test_sixteen_complex_kernels_without_scratch_within_two_waves_per_simd(tmp_path):
    ks = kernels_of_library(tmp_path)
    pretty = demangle(sorted(ks))
    z = {pretty[n]: k for n, k in ks.items() if "mm_numeric_z64<" in pretty[n]}
    shapes = sorted(tuple(int(v) for v in re.search(r"mm_numeric_z64<(\d+), ?(\d+)>", n).groups()) for n in z)
    assert shapes == [(a, c) for a in range(1, 5) for c in range(1, 5)], shapes
    assert len(z) == 16
    spilled = {n: k["private_segment_fixed_size"] for n, k in z.items() if k["private_segment_fixed_size"] > 0}
    assert not spilled, "complex kernels using scratch memory: %s" % spilled
    # 512 registers per SIMD lane: two waves per SIMD is what the 64 accumulator registers of <4,4> plus staging must leave room for
    too_big = {n: k["vgpr_count"] for n, k in z.items() if k["vgpr_count"] > 256}
    assert not too_big, too_big
    # LDS: the kernels hold no static LDS to speak of; the dynamic slice comes from the choice (largest block (8 MA, 8 NC), four waves per workgroup)
    for n, k in z.items():
        ma, nc = (int(v) for v in re.search(r"mm_numeric_z64<(\d+), ?(\d+)>", n).groups())
        c = choose(dict(cplx=1, max_m=8 * ma, max_n=8 * nc, max_k=8, min_m=8 * ma, min_n=8 * nc, min_k=8, nbr=64, nbc=64, c_nblks=4096,
                        nproducts=4096 * 64, order_len=512), wg_waves=4)
        assert c["name"] == "mm_numeric_z64<%d,%d>" % (ma, nc) and c["ww"] == 4
        total = k.get("group_segment_fixed_size", 0) + c["lds_bytes"]
        assert total <= LDS_PER_CU, (n, k.get("group_segment_fixed_size", 0), c["lds_bytes"])
        assert c["lds_bytes"] % 16 == 0 and k.get("group_segment_fixed_size", 0) % 16 == 0   # the dynamic base stays 16-byte aligned
