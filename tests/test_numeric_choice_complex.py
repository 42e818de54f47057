"""The kernel choice for complex_8 data (dbcsr_amd/csrc/mm_choose.h: SizeFacts::cplx, Family::z64), exercised without a GPU through a shim of
a few lines around the header, as tests/test_numeric_choice.py does for the real families: a complex multiply takes the instance
mm_numeric_z64<MA,NC> of its largest C block, sets up neither work records nor norms, and real multiplies keep the family numbers and names
they had before the complex family was appended."""
import ctypes
import functools
import os
import shutil
import subprocess
import tempfile

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dbcsr_amd", "csrc")

FACTS = ["max_m", "max_k", "max_n", "min_m", "min_k", "min_n", "hot_m", "hot_n", "hot_k", "hot_cnt_m", "hot_cnt_k", "hot_cnt_n", "nbr", "nbc", "c_nblks",
         "nproducts", "order_len", "retain", "filter_active", "fp64", "skip_empty", "cplx"]
OUT = ["family", "ww", "work", "norms", "leaves_norms", "grid", "flags", "lds_bytes"]
FAMILY_F64_MID, FAMILY_F64_HOT, FAMILY_Z64 = 2, 4, 20   # enum class Family: the complex family is appended after the last lab family, nothing renumbered

SHIM = """
#include "mm_choose.h"
using namespace dbcsr_amd;
extern "C" void numeric_choice_z(const long long* f, int wg_waves, char* name, long long* out) {
  SizeFacts F; Switches S; LabSwitches L;
  int i = 0;
%s
  S.wg_waves = wg_waves;
  const NumericChoice c = choose_numeric(F, S, L);
  snprintf(name, 96, "%%s", c.name);
  const long long o[] = {(long long)c.family, c.ww, c.work, c.norms, c.leaves_norms, c.grid, c.flags, (long long)c.lds_bytes};
  for (unsigned k = 0; k < sizeof o / sizeof o[0]; ++k) out[k] = o[k];
}
""" % "\n".join("  F.%s = f[i++];" % n for n in FACTS)


@functools.lru_cache(maxsize=None)
def _shim():
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++ to compile the shim around mm_choose.h")
    d = tempfile.mkdtemp(prefix="numeric_choice_z")
    src = os.path.join(d, "shim.cpp")
    with open(src, "w") as fh:
        fh.write(SHIM)
    so = os.path.join(d, "shim.so")
    subprocess.run([gxx, "-std=c++17", "-O1", "-shared", "-fPIC", "-I", CSRC, src, "-o", so], check=True)
    return ctypes.CDLL(so)


def choose(facts, wg_waves=0):
    """the NumericChoice for these size facts (missing ones: 0; fp64 defaults to 1) as a dict with its name"""
    f = dict.fromkeys(FACTS, 0)
    f["fp64"] = 1
    f.update(facts)
    name = ctypes.create_string_buffer(96)
    out = (ctypes.c_longlong * len(OUT))()
    _shim().numeric_choice_z((ctypes.c_longlong * len(FACTS))(*[int(f[n]) for n in FACTS]), int(wg_waves), name, out)
    return dict(zip(OUT, out), name=name.value.decode())


def uniform(m, n, k, nb=20, **kw):
    """a multiply of nb x nb x nb blocks of m x n x k, half of C's blocks present, ten products per block"""
    c_nblks = nb * nb // 2
    f = dict(max_m=m, min_m=m, max_n=n, min_n=n, max_k=k, min_k=k, hot_m=m, hot_n=n, hot_k=k, hot_cnt_m=nb, hot_cnt_n=nb, hot_cnt_k=nb, nbr=nb, nbc=nb,
             c_nblks=c_nblks, nproducts=10 * c_nblks, order_len=(c_nblks + 7) // 8 + 8)
    f.update(kw)
    return f


@pytest.mark.parametrize("mn,inst", [((5, 5), (1, 1)), ((8, 9), (1, 2)), ((23, 23), (3, 3)), ((32, 17), (4, 3)), ((33, 40), (4, 4)), ((80, 12), (4, 2))])
def test_complex_multiply_takes_the_instance_of_its_largest_block(mn, inst):
    f = uniform(mn[0], mn[1], 13, cplx=1, fp64=0)
    c = choose(f)
    assert c["family"] == FAMILY_Z64 and c["name"] == "mm_numeric_z64<%d,%d>" % inst
    assert (c["work"], c["norms"], c["leaves_norms"]) == (0, 0, 0)
    # one wave per launch position, ww waves per workgroup, each with the slab slice of the instance
    ma, nc = inst
    slice_bytes = 8 * (8 * ma + 1) * 16 + 8 * nc * 9 * 16
    assert c["ww"] == 1 and c["grid"] == 8 * f["order_len"] and c["lds_bytes"] == slice_bytes and c["flags"] == 0
    c4 = choose(dict(f, retain=1, skip_empty=1, filter_active=1), wg_waves=4)
    assert c4["family"] == FAMILY_Z64 and c4["ww"] == 4 and c4["grid"] == 2 * f["order_len"] and c4["lds_bytes"] == 4 * slice_bytes and c4["flags"] == 1
    assert (c4["work"], c4["norms"], c4["leaves_norms"]) == (0, 0, 0)
    # without a launch order: one wave per C block
    c0 = choose(dict(f, order_len=0), wg_waves=4)
    assert c0["grid"] == (f["c_nblks"] + 3) // 4
    # mixed sizes: the largest block decides, whatever dominates
    mixed = dict(f, min_m=1, min_n=2, hot_m=0, hot_n=0, hot_k=0)
    assert choose(mixed)["name"] == c["name"]


def test_real_multiplies_keep_their_families():
    """config 2 of the benchmark (23^3 blocks) and a slab-kernel case: family number and name as before the complex family existed"""
    config2 = uniform(23, 23, 23, nb=1424, c_nblks=2027776, nproducts=14 * 2027776, order_len=2027776 // 8 + 64)
    c = choose(config2)
    assert (c["family"], c["name"], c["work"]) == (FAMILY_F64_HOT, "mm_numeric_f64_hot<23,23,23>", 1)
    c = choose(uniform(40, 40, 40))
    assert (c["family"], c["name"], c["work"]) == (FAMILY_F64_MID, "mm_numeric_f64_mid<10,10>", 1)
    # cplx = 0 is the default of SizeFacts: a caller that never sets it is a real multiply
    assert "cplx" in FACTS and choose(dict(uniform(23, 23, 23), cplx=0))["name"] == "mm_numeric_f64_hot<23,23,23>"
