"""The rules that pick the numeric kernel of a multiply (dbcsr_amd/csrc/mm_choose.h: choose_classes, choose_numeric), exercised without a GPU.

mm_choose.h is plain C++: a shim of a few lines around it is compiled with the system g++ and called through ctypes.  The size facts of a case are
what the symbolic phase computes on the device (block_size_stats, mm_numeric_f64.h), restated here in Python from the case's block-size mix
(oracle/dbcsr_oracle.c: orc_make_block_sizes).  Every row of the tables restates a last_kernel() assertion that a `-m gpu` test makes with the
same case and switches, or a rule documented in mm_choose.h; the GPU tests keep asserting the same strings on the engine itself.
"""
import ctypes
import os
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dbcsr_amd", "csrc")

FACTS = ["max_m", "max_k", "max_n", "min_m", "min_k", "min_n", "hot_m", "hot_n", "hot_k", "hot_cnt_m", "hot_cnt_k", "hot_cnt_n", "units_m", "units_cnt_m",
         "units_n", "units_cnt_n", "nbr", "nbc", "c_nblks", "nproducts", "order_len", "retain", "canonical_c", "filter_active", "fp64", "skip_empty"]
SWITCHES = ["use_lds", "use_pipe", "pipe_g", "use_hot", "use_tiny", "use_small", "small_group", "use_mid", "use_big", "use_work", "use_classes", "wg_waves",
            "f32_direct"]
LAB = ["dbg", "dma_stages", "hot_persistent", "hot_variant", "lds_pad", "class_g", "class_streams", "row_group", "f32_group", "f64_group", "use_tile", "use_band"]
OUT = ["cls_mode", "ww", "work", "norms", "leaves_norms", "grid", "flags", "lds_a", "lds_wave", "maxt", "mid_rb", "mid_cb", "mid_class_mode", "lds_bytes"]

SHIM = """
#include "mm_choose.h"
using namespace dbcsr_amd;
extern "C" int numeric_choice(const long long* f, const int* s, const int* l, const int* hist, char* name, long long* out) {
  SizeFacts F; Switches S; LabSwitches L;
  int i = 0;
%s
  i = 0;
%s
#ifdef DBCSR_AMD_EXPERIMENTS
  i = 0;
%s
#endif
  choose_classes(&F, S, hist);
  const NumericChoice c = choose_numeric(F, S, L);
  snprintf(name, 96, "%%s", c.name);
  const long long o[] = {F.cls_mode, c.ww, c.work, c.norms, c.leaves_norms, c.grid, c.flags, c.lds_a, c.lds_wave, c.maxt, c.mid_rb, c.mid_cb, c.mid_class_mode,
                         (long long)c.lds_bytes};
  for (unsigned k = 0; k < sizeof o / sizeof o[0]; ++k) out[k] = o[k];
  return (int)c.family;
}
""" % ("\n".join("  F.%s = f[i++];" % n for n in FACTS), "\n".join("  S.%s = s[i++];" % n for n in SWITCHES), "\n".join("  L.%s = l[i++];" % n for n in LAB))


@pytest.fixture(scope="module")
def shims(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++ to compile the shim around mm_choose.h")
    d = tmp_path_factory.mktemp("numeric_choice")
    src = d / "shim.cpp"
    src.write_text(SHIM)
    libs = {}
    for lab, flag in ((False, []), (True, ["-DDBCSR_AMD_EXPERIMENTS"])):
        so = d / ("shim_lab.so" if lab else "shim.so")
        subprocess.run([gxx, "-std=c++17", "-O1", "-shared", "-fPIC", "-I", CSRC] + flag + [str(src), "-o", str(so)], check=True)
        libs[lab] = ctypes.CDLL(str(so))
    return libs


# ---- what the symbolic phase learns from the block sizes -------------------------------------------------------------------------------------
def block_sizes(total, mix):
    out, cur, sel, rep = [], 0, 0, 1
    while cur < total:
        bs = min(mix[2 * sel + 1], total - cur)
        out.append(bs)
        cur += bs
        rep += 1
        if rep > mix[2 * sel]:
            rep, sel = 1, (sel + 1) % (len(mix) // 2)
    return out


def size_stats(v):
    """max, min, most frequent size in 1 ... 32 (ties: the smallest) and its count, most frequent size in units of 4 (ties: the largest) and its
    count, histogram of 1 ... 32"""
    hist = [0] * 33
    units = [0] * 13
    for s in v:
        hist[s if 1 <= s <= 32 else 0] += 1
        if 1 <= s <= 48:
            units[(s + 3) // 4] += 1
    mode = max(range(1, 33), key=lambda s: (hist[s], -s))
    umode = max(range(1, 13), key=lambda u: (units[u], u))
    return max(v), min(v), (mode if hist[mode] else 0), hist[mode], (umode if units[umode] else 0), units[umode], hist


def facts_of(case, products_per_block=10.0, c_nblks=None, fp64=True, retain=False, filter_active=False, skip_empty=False):
    M, N, K, mix_m, mix_n, mix_k = case[0], case[1], case[2], case[6], case[7], case[8]
    m, n, k = size_stats(block_sizes(M, mix_m)), size_stats(block_sizes(N, mix_n)), size_stats(block_sizes(K, mix_k))
    nbr, nbc, nbk = len(block_sizes(M, mix_m)), len(block_sizes(N, mix_n)), len(block_sizes(K, mix_k))
    dominant = 10 * m[3] >= 9 * nbr and 10 * k[3] >= 9 * nbk and 10 * n[3] >= 9 * nbc
    c_nblks = max(1, nbr * nbc // 2) if c_nblks is None else c_nblks
    f = dict(max_m=m[0], max_k=k[0], max_n=n[0], min_m=m[1], min_k=k[1], min_n=n[1], hot_m=m[2] if dominant else 0, hot_n=n[2] if dominant else 0,
             hot_k=k[2] if dominant else 0, hot_cnt_m=m[3], hot_cnt_k=k[3], hot_cnt_n=n[3], units_m=m[4], units_cnt_m=m[5], units_n=n[4], units_cnt_n=n[5],
             nbr=nbr, nbc=nbc, c_nblks=c_nblks, nproducts=int(products_per_block * c_nblks), order_len=(c_nblks + 7) // 8 + 8, retain=int(retain),
             canonical_c=0, filter_active=int(filter_active), fp64=int(fp64), skip_empty=int(skip_empty))
    return f, m[6] + n[6] + k[6]


def switches_of(env):
    """mm_engine_env.h, the switches the choice reads"""
    s = dict(use_lds=1, use_pipe=-1, pipe_g=8, use_hot=1, use_tiny=1, use_small=2, small_group=0, use_mid=1, use_big=1, use_work=1, use_classes=1,
             wg_waves=0, f32_direct=1)
    lab = dict(dbg=0, dma_stages=0, hot_persistent=0, hot_variant=0, lds_pad=0, class_g=1, class_streams=1, row_group=0, f32_group=0, f64_group=0,
               use_tile=0, use_band=0)
    kern = env.get("DBCSR_AMD_MM_KERNEL")
    if kern is not None:
        s["use_lds"] = int(kern != "direct")
        s["use_pipe"] = 1 if kern == "pipe" else (0 if kern == "lds1" else -1)
        if kern[:3] == "dma" and kern[3:] in ("2", "3", "4"):
            lab["dma_stages"] = int(kern[3:])
    for name, key in (("PIPE_G", "pipe_g"), ("CLASSES", "use_classes"), ("WORK", "use_work"), ("HOT", "use_hot"), ("TINY", "use_tiny"), ("SMALL", "use_small"),
                      ("SMALL_G", "small_group"), ("F32_DIRECT", "f32_direct"), ("BIG", "use_big"), ("MID", "use_mid"), ("WG_WAVES", "wg_waves")):
        if "DBCSR_AMD_MM_" + name in env:
            s[key] = int(env["DBCSR_AMD_MM_" + name])
    for name, key in (("HOT_VARIANT", "hot_variant"), ("HOT_PERSISTENT", "hot_persistent"), ("CLASS_G", "class_g"), ("CLASS_STREAMS", "class_streams"),
                      ("F64_GROUP", "f64_group"), ("TILE", "use_tile"), ("BAND", "use_band"), ("DBG", "dbg"), ("LDS_PAD", "lds_pad")):
        if "DBCSR_AMD_MM_" + name in env:
            lab[key] = int(env["DBCSR_AMD_MM_" + name])
    if "DBCSR_AMD_MM_F32_GROUP" in env:
        r = int(env["DBCSR_AMD_MM_F32_GROUP"])
        lab["f32_group"] = r if 2 <= r <= 4 else (-1 if r < 0 else 0)
    return s, lab, any(lab[k] != v for k, v in (("dma_stages", 0), ("hot_variant", 0), ("hot_persistent", 0), ("class_g", 1), ("class_streams", 1),
                                                 ("f32_group", 0), ("f64_group", 0), ("use_tile", 0), ("use_band", 0), ("dbg", 0), ("lds_pad", 0))) or bool(env.get("LAB"))


def choose(shims, env, case, **kw):
    f, hist = facts_of(case, **kw)
    s, lab, is_lab = switches_of(env)
    name = ctypes.create_string_buffer(96)
    out = (ctypes.c_longlong * len(OUT))()
    shims[is_lab].numeric_choice((ctypes.c_longlong * len(FACTS))(*[f[n] for n in FACTS]), (ctypes.c_int * len(SWITCHES))(*[s[n] for n in SWITCHES]),
                                 (ctypes.c_int * len(LAB))(*[lab[n] for n in LAB]), (ctypes.c_int * 99)(*hist), name, out)
    return name.value.decode(), dict(zip(OUT, out))


# ---- tests/test_gpu_kernel_variants.py: VARIANTS (the rows that do not depend on a run-time event) and the fp32 table --------------------------
MIXED = (300, 280, 260, 0.5, 0.5, 0.6, [1, 13, 1, 23, 1, 32, 1, 7], [1, 23, 1, 5, 1, 32], [1, 13, 1, 32, 1, 9])
H2O = (23 * 20 + 16, 23 * 18 + 16, 23 * 22 + 16, 0.6, 0.6, 0.7, [1, 23], [1, 23], [1, 23])
TINY = (240, 240, 240, 0.7, 0.7, 0.7, [1, 4], [1, 4, 1, 3], [1, 4, 1, 2])
TINY_K = (230, 250, 420, 0.6, 0.7, 0.7, [1, 4, 1, 2], [1, 3, 1, 1, 1, 4], [1, 7, 1, 4, 1, 13])
CONFIG3 = (68 * 9 + 24, 68 * 8 + 24, 68 * 10 + 24, 0.8, 0.8, 0.8, [1, 13, 1, 23, 1, 32], [1, 13, 1, 23, 1, 32], [1, 13, 1, 23, 1, 32])
CONFIG3_37 = (68 * 66 + 24, 68 * 66 + 24, 68 * 66 + 24, 0.864, 0.864, 0.864, [1, 13, 1, 23, 1, 32], [1, 13, 1, 23, 1, 32], [1, 13, 1, 23, 1, 32])
POW2 = (16 * 20 + 9, 32 * 10 + 5, 16 * 18 + 3, 0.6, 0.6, 0.6, [1, 16, 1, 32], [1, 32, 1, 16, 1, 8], [1, 16, 1, 32, 1, 24])
BIG = (300, 270, 280, 0.5, 0.5, 0.5, [1, 45, 1, 13], [1, 67, 1, 5], [1, 40, 1, 23])
F32 = (32 * 12, 32 * 11, 32 * 13, 0.6, 0.6, 0.6, [1, 32], [1, 32], [1, 32])
F32_TAILS = (32 * 24 + 20, 32 * 22 + 7, 32 * 26 + 12, 0.6, 0.6, 0.6, [1, 32], [1, 32], [1, 32])
F32_16 = (16 * 30 + 5, 16 * 28 + 9, 16 * 33 + 4, 0.6, 0.6, 0.6, [1, 16], [1, 16], [1, 16])
F32_24 = (24 * 20 + 13, 24 * 18, 24 * 22 + 8, 0.6, 0.6, 0.6, [1, 24], [1, 24], [1, 24])
F32_MIXED = (300, 280, 260, 0.5, 0.5, 0.6, [1, 13, 1, 32, 1, 7], [1, 23, 1, 32], [1, 13, 1, 32, 1, 9])
PPB = {id(CONFIG3_37): 3.7}   # products per C block where the case's comment states them (the pipe rule reads them)

VARIANTS = [
    ({}, H2O, "mm_numeric_f64_hot<23,23,23>"),
    ({"DBCSR_AMD_MM_HOT_VARIANT": "1"}, H2O, "mm_numeric_f64_hot<23,23,23>"),
    ({"DBCSR_AMD_MM_HOT_VARIANT": "6"}, H2O, "mm_numeric_f64_hot<23,23,23>"),
    ({"DBCSR_AMD_MM_HOT_PERSISTENT": "1"}, H2O, "mm_numeric_f64_hot_persistent<23,23,23>"),
    ({"DBCSR_AMD_MM_HOT": "0", "DBCSR_AMD_MM_KERNEL": "lds1"}, H2O, "mm_numeric_f64_lds<3>"),
    ({"DBCSR_AMD_MM_KERNEL": "pipe"}, H2O, "mm_numeric_f64_pipe<3>"),
    ({"DBCSR_AMD_MM_KERNEL": "dma2"}, H2O, "mm_numeric_f64_dma<23,23,23,2>"),
    ({"DBCSR_AMD_MM_KERNEL": "dma3"}, H2O, "mm_numeric_f64_dma<23,23,23,3>"),
    ({"DBCSR_AMD_MM_KERNEL": "direct"}, H2O, "mm_numeric_f64"),
    ({"DBCSR_AMD_MM_KERNEL": "lds1"}, MIXED, "mm_numeric_f64_lds<4>"),
    ({"DBCSR_AMD_MM_KERNEL": "pipe"}, MIXED, "mm_numeric_f64_pipe<4>"),
    ({"DBCSR_AMD_MM_KERNEL": "pipe", "DBCSR_AMD_MM_PIPE_G": "3"}, MIXED, "mm_numeric_f64_pipe<4>"),
    ({"DBCSR_AMD_MM_KERNEL": "direct"}, MIXED, "mm_numeric_f64"),
    ({}, TINY, "mm_numeric_f64_tiny"),
    ({}, TINY_K, "mm_numeric_f64_tiny"),
    ({"DBCSR_AMD_MM_TINY": "0", "DBCSR_AMD_MM_KERNEL": "lds1"}, TINY, "mm_numeric_f64_lds<1>"),
    ({"DBCSR_AMD_MM_TINY": "0", "DBCSR_AMD_MM_KERNEL": "pipe"}, TINY, "mm_numeric_f64_pipe<1>"),
    ({}, BIG, "mm_numeric_f64"),
    ({"DBCSR_AMD_MM_CLASSES": "2"}, MIXED, "mm_numeric_f64_class["),
    ({"DBCSR_AMD_MM_CLASSES": "2"}, H2O, "mm_numeric_f64_class["),
    ({"DBCSR_AMD_MM_CLASSES": "2"}, CONFIG3, "mm_numeric_f64_class["),
    ({"DBCSR_AMD_MM_CLASSES": "2"}, POW2, "mm_numeric_f64_class["),
    ({"DBCSR_AMD_MM_CLASSES": "2", "DBCSR_AMD_MM_MID": "0"}, CONFIG3_37, "mm_numeric_f64_class["),
    ({"DBCSR_AMD_MM_CLASSES": "0"}, CONFIG3_37, "mm_numeric_f64_pipe<4>"),
    ({"DBCSR_AMD_MM_CLASSES": "2", "DBCSR_AMD_MM_CLASS_G": "8"}, MIXED, "mm_numeric_f64_class["),
    ({"DBCSR_AMD_MM_WG_WAVES": "4"}, H2O, "mm_numeric_f64_hot<23,23,23>"),
    ({"DBCSR_AMD_MM_WG_WAVES": "1", "DBCSR_AMD_MM_KERNEL": "lds1", "DBCSR_AMD_MM_HOT": "0"}, MIXED, "mm_numeric_f64_lds"),
    ({"DBCSR_AMD_MM_WORK": "0"}, H2O, "mm_numeric_f64_hot<23,23,23>"),
    ({"DBCSR_AMD_MM_CLASS_STREAMS": "3", "DBCSR_AMD_MM_CLASSES": "2"}, CONFIG3_37, "mm_numeric_f64_class["),
]
F32_VARIANTS = [
    ({}, F32, "mm_numeric_f32_direct<32,32,32>"),
    ({}, F32_TAILS, "mm_numeric_f32_direct<32,32,32>"),
    ({}, F32_16, "mm_numeric_f32_direct<16,16,16>"),
    ({}, F32_24, "mm_numeric_f32_direct<24,24,24>"),
    ({}, H2O, "mm_numeric_f32_hot<23,23,23>"),
    ({"DBCSR_AMD_MM_F32_DIRECT": "0"}, F32, "mm_numeric_f32_hot<32,32,32>"),
    ({"DBCSR_AMD_MM_F32_DIRECT": "0"}, F32_TAILS, "mm_numeric_f32_hot<32,32,32>"),
    ({"DBCSR_AMD_MM_HOT": "0"}, F32, "mm_numeric_f32_lds"),
    ({"DBCSR_AMD_MM_KERNEL": "direct"}, F32, "mm_numeric_f32"),
    ({"DBCSR_AMD_MM_KERNEL": "direct"}, F32_MIXED, "mm_numeric_f32"),
    ({"DBCSR_AMD_MM_CLASSES": "2"}, F32_MIXED, "mm_numeric_f32_lds[per class"),
    ({"DBCSR_AMD_MM_WG_WAVES": "4"}, F32_TAILS, "mm_numeric_f32_direct<32,32,32>"),
    ({"DBCSR_AMD_MM_WG_WAVES": "2"}, F32_16, "mm_numeric_f32_direct<16,16,16>"),
    ({"DBCSR_AMD_MM_WG_WAVES": "2"}, F32_MIXED, "mm_numeric_f32_lds"),
    ({"DBCSR_AMD_MM_WG_WAVES": "4", "DBCSR_AMD_MM_CLASSES": "2"}, F32_MIXED, "mm_numeric_f32_lds[per class"),
    # tests/test_gpu_f32_group.py:115-181: the group kernel stands back when the inner dimension has a tail block or the switch is 0; -1 takes it
    # for at least 16 products per C block and 1024 C blocks
    ({"DBCSR_AMD_MM_F32_GROUP": "4"}, (32 * 12, 32 * 11, 32 * 13 + 12, 0.5, 0.5, 0.5, [1, 32], [1, 32], [1, 32]), "mm_numeric_f32_direct<32,32,32>"),
    ({"DBCSR_AMD_MM_F32_GROUP": "4"}, F32, "mm_numeric_f32_group<32,32,32;4>"),
    ({"DBCSR_AMD_MM_F32_GROUP": "0", "LAB": "1"}, F32, "mm_numeric_f32_direct<32,32,32>"),
]




# tests/test_gpu_multiply.py: test_exact_size_kernels_every_cube_with_tails -- every cube of 9 ... 32 with a ragged tail block in every dimension (twelve blocks
# of the size and the tail: the size dominates); the fp32 half takes the direct form where k is a multiple of 8, else the form that stages both operands
def exact_cube_with_tails(size):
    dim = 12 * size + max(1, size // 3)
    return (dim, dim, dim, 0.6, 0.6, 0.7, [1, size], [1, size], [1, size])


F32_EXACT_CUBES = [({}, exact_cube_with_tails(s), "mm_numeric_f32_%s<%d,%d,%d>" % ("direct" if s in (16, 24, 32) else "hot", s, s, s)) for s in range(9, 33)]


@pytest.mark.parametrize("env,case,expect", VARIANTS)
def test_fp64_kernel_variants(shims, env, case, expect):
    name, _ = choose(shims, env, case, products_per_block=PPB.get(id(case), 10.0))
    assert name.replace(" ", "").startswith(expect.replace(" ", "")), (name, expect)


@pytest.mark.parametrize("env,case,expect", F32_VARIANTS)
def test_fp32_kernel_variants(shims, env, case, expect):
    name, _ = choose(shims, env, case, fp64=False)
    assert name.startswith(expect), (name, expect)


@pytest.mark.parametrize("env,case,expect", F32_EXACT_CUBES, ids=[str(s) for s in range(9, 33)])
def test_fp32_exact_size_kernel_of_every_cube(shims, env, case, expect):
    assert choose(shims, env, case, fp64=False)[0] == expect
    size = case[6][1]
    assert choose(shims, env, case)[0] == "mm_numeric_f64_hot<%d,%d,%d>" % (size, size, size)   # (the fp64 half of the same test)


def test_fp32_group_automatic_choice(shims):
    """tests/test_gpu_f32_group.py: DBCSR_AMD_MM_F32_GROUP=-1 takes R = 4 from 16 products per C block and 1024 C blocks on (the product of this case is dense: 36 x 34 C blocks)"""
    case = (32 * 36, 32 * 34, 32 * 120, 0.6, 0.6, 0.5, [1, 32], [1, 32], [1, 32])
    assert choose(shims, {}, case, fp64=False, c_nblks=36 * 34, products_per_block=19)[0] == "mm_numeric_f32_direct<32,32,32>"
    assert choose(shims, {"DBCSR_AMD_MM_F32_GROUP": "-1"}, case, fp64=False, c_nblks=36 * 34, products_per_block=19)[0] == "mm_numeric_f32_group<32,32,32;4>"
    assert choose(shims, {"DBCSR_AMD_MM_F32_GROUP": "-1"}, case, fp64=False, c_nblks=36 * 34, products_per_block=3)[0] == "mm_numeric_f32_direct<32,32,32>"


# ---- tests/test_gpu_big_blocks.py: CASES, and the two switches of test_blocks_above_80_keep_the_plain_kernel ---------------------------------------
BIG_CASES = {
    "72cube": ((72 * 5, 72 * 4, 72 * 6, 0.4, 0.4, 0.5, [1, 72], [1, 72], [1, 72]), "mm_numeric_f64_big<5,5>"),
    "80cube_tails": ((80 * 3 + 33, 80 * 3 + 7, 80 * 4 + 50, 0.3, 0.3, 0.5, [1, 80], [1, 80], [1, 80]), "mm_numeric_f64_big<5,5>"),
    "64cube": ((64 * 5, 64 * 5, 64 * 5, 0.4, 0.4, 0.5, [1, 64], [1, 64], [1, 64]), "mm_numeric_f64_big<4,4>"),
    "40cube": ((40 * 8, 40 * 7, 40 * 9, 0.5, 0.5, 0.5, [1, 40], [1, 40], [1, 40]), "mm_numeric_f64_mid<10,10>"),
    "33cube": ((33 * 8, 33 * 9, 33 * 7, 0.5, 0.5, 0.5, [1, 33], [1, 33], [1, 33]), "mm_numeric_f64_mid<9,9>"),
    "55cube": ((55 * 6, 55 * 5, 55 * 7, 0.5, 0.5, 0.5, [1, 55], [1, 55], [1, 55]), "mm_numeric_f64_big<4,4>"),
    "45x67x78": ((45 * 7, 67 * 5, 78 * 5, 0.4, 0.4, 0.5, [1, 45], [1, 67], [1, 78]), "mm_numeric_f64_big<3,5>"),
    "78x45x67": ((78 * 4, 45 * 7, 67 * 5, 0.4, 0.4, 0.5, [1, 78], [1, 45], [1, 67]), "mm_numeric_f64_big<5,3>"),
    "23x23_k78": ((23 * 12, 23 * 11, 78 * 5, 0.4, 0.4, 0.5, [1, 23], [1, 23], [1, 78]), "mm_numeric_f64_big<2,2>"),
    "80x16_k37": ((80 * 4, 16 * 12, 37 * 9, 0.4, 0.4, 0.5, [1, 80], [1, 16], [1, 37]), "mm_numeric_f64_big<5,2>"),
    "13x72_k33": ((13 * 14, 72 * 4, 33 * 9, 0.4, 0.4, 0.5, [1, 13], [1, 72], [1, 33]), "mm_numeric_f64_big<2,5>"),
    "mixed_sizes": ((400, 390, 410, 0.5, 0.5, 0.6, [1, 45, 1, 13, 1, 72, 1, 5], [1, 67, 1, 5, 1, 33], [1, 40, 1, 23, 1, 3, 1, 61]), "mm_numeric_f64_big<5,5>"),
    "k_remainders": ((48 * 5, 56 * 5, 420, 0.4, 0.4, 0.5, [1, 48], [1, 56], [1, 17, 1, 18, 1, 19, 1, 33, 1, 34, 1, 35, 1, 49, 1, 1, 1, 64]), "mm_numeric_f64_big<3,4>"),
    "one_block": ((72, 80, 33, 0.0, 0.0, 0.0, [1, 72], [1, 80], [1, 33]), "mm_numeric_f64_big<5,5>"),
    "34cube": ((34 * 8, 34 * 9, 34 * 7, 0.5, 0.5, 0.5, [1, 34], [1, 34], [1, 34]), "mm_numeric_f64_mid<9,9>"),
    "35x36x37": ((35 * 8, 36 * 8, 37 * 7, 0.5, 0.5, 0.5, [1, 35], [1, 36], [1, 37]), "mm_numeric_f64_mid<9,9>"),
    "37x33x36": ((37 * 8, 33 * 9, 36 * 7, 0.5, 0.5, 0.5, [1, 37], [1, 33], [1, 36]), "mm_numeric_f64_mid<10,9>"),
    "36x39_k80": ((36 * 8, 39 * 8, 80 * 4, 0.5, 0.5, 0.5, [1, 36], [1, 39], [1, 80]), "mm_numeric_f64_mid<9,10>"),
    "36cube_tails": ((36 * 6 + 20, 36 * 6 + 7, 36 * 6 + 30, 0.4, 0.4, 0.5, [1, 36], [1, 36], [1, 36]), "mm_numeric_f64_mid<9,9>"),
    "mix_33_to_40": ((36 * 8, 36 * 8, 300, 0.5, 0.5, 0.5, [1, 33, 1, 40, 1, 37, 1, 36], [1, 40, 1, 34, 1, 38], [1, 40, 1, 5, 1, 33, 1, 17]), "mm_numeric_f64_mid<10,10>"),
    "mostly_34_some_small": ((34 * 12 + 13, 34 * 12 + 40, 34 * 8, 0.5, 0.5, 0.5, [12, 34, 1, 13], [12, 34, 1, 40], [1, 34]), "mm_numeric_f64_mid<"),
    "mix_30_36": ((33 * 8, 33 * 8, 33 * 7, 0.5, 0.5, 0.5, [1, 30, 1, 36], [1, 36, 1, 30], [1, 30, 1, 36]), "mm_numeric_f64_big<3,3>"),
    "mix_33_36": ((35 * 8, 35 * 8, 35 * 7, 0.5, 0.5, 0.5, [1, 33, 1, 36], [1, 36, 1, 33], [1, 33, 1, 36]), "mm_numeric_f64_mid<9,9>"),
    "mix_23_40": ((32 * 8, 32 * 8, 32 * 7, 0.5, 0.5, 0.5, [1, 23, 1, 40], [1, 40, 1, 23], [1, 23, 1, 40]), "mm_numeric_f64_mid<10,10>"),
    "44cube": ((44 * 7, 44 * 6, 44 * 8, 0.5, 0.5, 0.5, [1, 44], [1, 44], [1, 44]), "mm_numeric_f64_mid<11,11>"),
    "48cube_tails": ((48 * 6 + 20, 48 * 6 + 45, 48 * 6 + 30, 0.4, 0.4, 0.5, [1, 48], [1, 48], [1, 48]), "mm_numeric_f64_mid<12,12>"),
    "41x47_k33": ((41 * 7, 47 * 6, 33 * 9, 0.5, 0.5, 0.5, [1, 41], [1, 47], [1, 33]), "mm_numeric_f64_big<3,3>"),
    "44x48_k33": ((44 * 7, 48 * 6, 33 * 9, 0.5, 0.5, 0.5, [1, 44], [1, 48], [1, 33]), "mm_numeric_f64_mid<11,12>"),
    "36x45_k80": ((36 * 8, 45 * 7, 80 * 4, 0.5, 0.5, 0.5, [1, 36], [1, 45], [1, 80]), "mm_numeric_f64_mid<9,12>"),
    "mix_30_to_48": ((400, 410, 300, 0.5, 0.5, 0.5, [1, 33, 1, 48, 1, 41, 1, 30], [1, 44, 1, 34, 1, 48], [1, 40, 1, 5, 1, 33, 1, 17]), "mm_numeric_f64_mid<12,12>"),
    "41x49x20": ((41 * 7, 49 * 6, 20 * 12, 0.5, 0.5, 0.5, [1, 41], [1, 49], [1, 20]), "mm_numeric_f64_big<3,4>"),
    "53x64x41": ((53 * 6, 64 * 5, 41 * 7, 0.5, 0.5, 0.5, [1, 53], [1, 64], [1, 41]), "mm_numeric_f64_big<4,4>"),
    "65x73x16": ((65 * 5, 73 * 4, 16 * 15, 0.4, 0.4, 0.5, [1, 65], [1, 73], [1, 16]), "mm_numeric_f64_big<5,5>"),
    "69x77x31": ((69 * 4, 77 * 4, 31 * 9, 0.4, 0.4, 0.5, [1, 69], [1, 77], [1, 31]), "mm_numeric_f64_big<5,5>"),
    "33x80x5": ((33 * 9, 80 * 4, 5 * 40, 0.4, 0.4, 0.5, [1, 33], [1, 80], [1, 5]), "mm_numeric_f64_big<3,5>"),
}


@pytest.mark.parametrize("name", sorted(BIG_CASES))
def test_big_and_slab_kernels(shims, name):
    case, expect = BIG_CASES[name]
    for kw in ({}, {"retain": True}, {"retain": True, "skip_empty": True}):
        got, _ = choose(shims, {}, case, **kw)
        assert got == expect or (expect.endswith("<") and got.startswith(expect)), (got, expect)


def test_blocks_above_80_and_the_switches_back(shims):
    assert choose(shims, {}, (100 * 3, 90 * 3, 85 * 3, 0.3, 0.3, 0.5, [1, 100], [1, 90], [1, 85]))[0] == "mm_numeric_f64"
    assert choose(shims, {"DBCSR_AMD_MM_BIG": "0"}, BIG_CASES["72cube"][0])[0] == "mm_numeric_f64"
    # DBCSR_AMD_MM_MID=0: blocks of 33 ... 40 through the workgroup kernel (mm_choose.h: Switches::use_mid)
    assert choose(shims, {"DBCSR_AMD_MM_MID": "0"}, BIG_CASES["40cube"][0])[0] == "mm_numeric_f64_big<3,3>"


# ---- tests/test_gpu_small_blocks.py ---------------------------------------------------------------------------------------------------------------
SMALL_CASES = {
    "5cube": (5 * 40, 5 * 38, 5 * 42, 0.6, 0.6, 0.7, [1, 5], [1, 5], [1, 5]),
    "7cube_tails": (7 * 30 + 3, 7 * 31 + 5, 7 * 29 + 2, 0.6, 0.6, 0.7, [1, 7], [1, 7], [1, 7]),
    "8cube_tails": (8 * 30 + 5, 8 * 31 + 1, 8 * 29 + 7, 0.5, 0.5, 0.7, [1, 8], [1, 8], [1, 8]),
    "5x8x6": (5 * 40, 8 * 30, 6 * 35, 0.6, 0.6, 0.7, [1, 5], [1, 8], [1, 6]),
    "7x7_k3": (7 * 30, 7 * 32, 3 * 70, 0.6, 0.6, 0.7, [1, 7], [1, 7], [1, 3]),
    "3x8_k8": (3 * 60, 8 * 30, 8 * 30, 0.6, 0.6, 0.7, [1, 3], [1, 8], [1, 8]),          # C blocks within 4 rows, not within 4 x 4
    "8x2_k5": (8 * 30, 2 * 90, 5 * 44, 0.6, 0.6, 0.7, [1, 8], [1, 2], [1, 5]),
    "mix_1_to_8": (230, 240, 250, 0.6, 0.6, 0.7, [1, 5, 1, 8, 1, 1, 1, 3, 2, 7], [1, 6, 1, 2, 1, 8, 1, 4], [1, 8, 1, 5, 1, 1, 1, 7, 1, 4]),
    "mix_5_8": (5 * 20 + 8 * 20, 5 * 21 + 8 * 19, 5 * 18 + 8 * 22, 0.6, 0.6, 0.7, [1, 5, 1, 8], [1, 8, 1, 5], [1, 5, 1, 8]),
    "very_long_lists": (5 * 6, 7 * 6, 8 * 400, 0.3, 0.3, 0.5, [1, 5], [1, 7], [1, 8]),
    "one_block": (8, 7, 6, 0.0, 0.0, 0.0, [1, 8], [1, 7], [1, 6]),
}


@pytest.mark.parametrize("name", sorted(SMALL_CASES))
def test_small_block_kernel(shims, name):
    case = SMALL_CASES[name]
    assert choose(shims, {}, case)[0] == "mm_numeric_f64_small<2>"
    for depth in ("3", "4", "6", "8"):
        assert choose(shims, {"DBCSR_AMD_MM_SMALL": depth}, case)[0] == "mm_numeric_f64_small<%s>" % depth
    assert choose(shims, {"DBCSR_AMD_MM_SMALL": "6", "DBCSR_AMD_MM_WORK": "0"}, case)[0] == "mm_numeric_f64_small<6>"
    assert choose(shims, {}, case, retain=True, skip_empty=True)[0] == "mm_numeric_f64_small<2>"
    assert choose(shims, {}, case, filter_active=True)[0] == "mm_numeric_f64_small<2>"
    off, _ = choose(shims, {"DBCSR_AMD_MM_SMALL": "0"}, case)
    assert off.startswith("mm_numeric_f64_") and "small" not in off


def test_blocks_within_4x4_keep_the_packed_kernel_and_9_keeps_the_exact_size_kernel(shims):
    for case, expect in (((4 * 40, 4 * 40, 8 * 20, 0.6, 0.6, 0.7, [1, 4], [1, 4], [1, 8]), "mm_numeric_f64_tiny"),
                         ((9 * 20, 8 * 20, 8 * 20, 0.6, 0.6, 0.7, [1, 9], [1, 8], [1, 8]), "mm_numeric_f64_"),
                         ((8 * 20, 8 * 20, 9 * 20, 0.6, 0.6, 0.7, [1, 8], [1, 8], [1, 9]), "mm_numeric_f64_")):
        got, _ = choose(shims, {}, case)
        assert got.startswith(expect) and "small" not in got, got


# ---- rules documented in mm_choose.h -----------------------------------------------------------------------------------------------------------------
def cube(s, nb=20):
    return (s * nb, s * nb, s * nb, 0.5, 0.5, 0.5, [1, s], [1, s], [1, s])


@pytest.mark.parametrize("case,expect", [
    (cube(4), "mm_numeric_f64_tiny"), (cube(5), "mm_numeric_f64_small<2>"), (cube(8), "mm_numeric_f64_small<2>"), (cube(13), "mm_numeric_f64_hot<13,13,13>"),
    (cube(23), "mm_numeric_f64_hot<23,23,23>"), (cube(32), "mm_numeric_f64_hot<32,32,32>"), (cube(33), "mm_numeric_f64_mid<9,9>"),
    (cube(40), "mm_numeric_f64_mid<10,10>"), (cube(64), "mm_numeric_f64_big<4,4>"), (cube(80), "mm_numeric_f64_big<5,5>"), (cube(100), "mm_numeric_f64"),
    ((32 * 20, 9 * 20, 9 * 20, 0.5, 0.5, 0.5, [1, 32], [1, 9], [1, 9]), "mm_numeric_f64_lds<4>"),   # a dominant triplet that is no cube, too few C blocks for classes
])
def test_documented_rules(shims, case, expect):
    assert choose(shims, {}, case)[0] == expect


def test_switches_named_in_the_rules(shims):
    assert choose(shims, {"DBCSR_AMD_MM_HOT": "0"}, cube(23))[0] == "mm_numeric_f64_lds<3>"
    assert choose(shims, {"DBCSR_AMD_MM_TINY": "0"}, cube(4))[0] == "mm_numeric_f64_small<2>"
    assert choose(shims, {"DBCSR_AMD_MM_TINY": "0", "DBCSR_AMD_MM_SMALL": "0"}, cube(4))[0] == "mm_numeric_f64_lds<1>"
    assert choose(shims, {"DBCSR_AMD_MM_KERNEL": "direct"}, cube(40))[0] == "mm_numeric_f64"
    # short product lists of mixed sizes: the pipelined kernel between 1.5 and 6 products per C block
    for ppb, expect in ((1.2, "mm_numeric_f64_lds<4>"), (3.7, "mm_numeric_f64_pipe<4>"), (14.4, "mm_numeric_f64_lds<4>")):
        assert choose(shims, {}, MIXED, products_per_block=ppb)[0] == expect
    # (m, n) classes by themselves: from 200000 C blocks on, unless one cube of 9 ... 32 dominates
    assert choose(shims, {}, CONFIG3_37, c_nblks=200000)[0] == "mm_numeric_f64_class["
    assert choose(shims, {}, CONFIG3_37, c_nblks=199999, products_per_block=3.7)[0] == "mm_numeric_f64_pipe<4>"
    assert choose(shims, {}, H2O, c_nblks=200000)[0] == "mm_numeric_f64_hot<23,23,23>"
    assert choose(shims, {}, (5 * 900, 13 * 900, 23 * 100, 0.5, 0.5, 0.5, [1, 5], [1, 13], [1, 23]), c_nblks=400000)[0] == "mm_numeric_f64_class["


def test_waves_per_workgroup(shims):
    """one wave per workgroup while C blocks have at most 32 products on average, else four; DBCSR_AMD_MM_WG_WAVES overrides"""
    assert choose(shims, {}, H2O, products_per_block=32)[1]["ww"] == 1
    assert choose(shims, {}, H2O, products_per_block=32.1)[1]["ww"] == 4
    for w in (1, 2, 4):
        assert choose(shims, {"DBCSR_AMD_MM_WG_WAVES": str(w)}, H2O, products_per_block=100)[1]["ww"] == w


def test_work_records_and_norms(shims):
    """work records for the exact-size, slab and small-block kernels; the norm area when a filtered multiply runs a kernel family that leaves norms"""
    _, o = choose(shims, {}, H2O, filter_active=True)
    assert o["work"] and o["norms"] and o["leaves_norms"]
    _, o = choose(shims, {}, H2O, filter_active=True, retain=True)
    assert o["work"] and not o["norms"]
    _, o = choose(shims, {}, cube(40), filter_active=True)
    assert o["work"] and o["norms"] and o["leaves_norms"] and (o["mid_rb"], o["mid_cb"]) == (10, 10)
    _, o = choose(shims, {}, cube(5), filter_active=True)
    assert o["work"] and not o["norms"]
    _, o = choose(shims, {"DBCSR_AMD_MM_WORK": "0"}, cube(5))
    assert not o["work"]
    _, o = choose(shims, {}, cube(64), filter_active=True)
    assert not o["work"] and not o["norms"]
    _, o = choose(shims, {"DBCSR_AMD_MM_CLASSES": "2"}, CONFIG3, filter_active=True)
    assert o["cls_mode"] and o["work"] and o["norms"] and o["leaves_norms"]
    # kept as it is (mm_choose.h): a dominant cube without an exact-size instance sets both up, then runs the generic LDS kernel, which uses neither
    name, o = choose(shims, {"DBCSR_AMD_MM_SMALL": "0"}, cube(5), filter_active=True)
    assert name == "mm_numeric_f64_lds<1>" and o["work"] and o["norms"] and not o["leaves_norms"]
    # ... and a mixed-size multiply in class mode through DBCSR_AMD_MM_KERNEL=direct: the class arm of `norms` sets the norm area up, the plain kernel leaves none
    name, o = choose(shims, {"DBCSR_AMD_MM_KERNEL": "direct", "DBCSR_AMD_MM_CLASSES": "2"}, MIXED, filter_active=True)
    assert name == "mm_numeric_f64" and o["cls_mode"] and not o["work"] and o["norms"] and not o["leaves_norms"]


# ---- tests/test_gpu_class_mode.py: products of about 470 x 450 C blocks, all of them present (>= 200000: classes by themselves) ------------------------
CLASS_CASES = {
    "2x9x3": ((2 * 470, 9 * 450, 3 * 100, 0.7, 0.7, 0.5, [1, 2], [1, 9], [1, 3]), "mm_numeric_f64_class["),
    "13x5x23": ((13 * 470, 5 * 450, 23 * 40, 0.6, 0.6, 0.5, [1, 13], [1, 5], [1, 23]), "mm_numeric_f64_class["),
    "9x32x9_tails": ((9 * 470 + 4, 32 * 450 + 7, 9 * 60 + 5, 0.6, 0.6, 0.5, [1, 9], [1, 32], [1, 9]), "mm_numeric_f64_class["),
    "alternating_5_13": ((18 * 240, 18 * 235, 18 * 25, 0.6, 0.6, 0.5, [1, 5, 1, 13], [1, 5, 1, 13], [1, 5, 1, 13]), "mm_numeric_f64_class["),
    "period_4": ((28 * 120, 28 * 118, 28 * 14, 0.6, 0.6, 0.5, [1, 5, 1, 9, 1, 5, 1, 9], [1, 9, 1, 5], [1, 5, 2, 9, 1, 5]), "mm_numeric_f64_class["),
    "alternating_3_13_rows_only": ((16 * 250, 7 * 480, 11 * 40, 0.6, 0.6, 0.5, [1, 3, 1, 13], [1, 7], [1, 11]), "mm_numeric_f64_class["),
    "cube_13": ((13 * 470, 13 * 450, 13 * 60, 0.6, 0.6, 0.5, [1, 13], [1, 13], [1, 13]), "mm_numeric_f64_hot<13,13,13>"),
    "cube_6": ((6 * 470, 6 * 450, 6 * 100, 0.7, 0.7, 0.5, [1, 6], [1, 6], [1, 6]), "mm_numeric_f64_small<2>"),
}


@pytest.mark.parametrize("name", sorted(CLASS_CASES))
def test_class_mode_by_itself(shims, name):
    case, expect = CLASS_CASES[name]
    nblk = len(block_sizes(case[0], case[6])) * len(block_sizes(case[1], case[7]))
    assert nblk >= 200000
    got, o = choose(shims, {}, case, c_nblks=nblk)
    assert got == expect, (got, expect)
    # (a cube of 9 ... 32 keeps its ahead-of-time kernel, class mode off; blocks of at most 8 ARE in class mode -- their launch order is the classes' --
    # and the small-block kernel still takes them: it is asked before the classes)
    assert o["cls_mode"] == (name != "cube_13")


FILTER_CASES = {
    "hot23_tails": ((23 * 20 + 16, 23 * 18 + 9, 23 * 22 + 5, 0.6, 0.6, 0.6, [1, 23], [1, 23], [1, 23]), {}, "mm_numeric_f64_hot<23,23,23>"),
    "classes_13_23_32": ((68 * 6, 68 * 5 + 13, 68 * 6 + 23, 0.6, 0.6, 0.6, [1, 13, 1, 23, 1, 32], [1, 32, 1, 13, 1, 23], [1, 23, 1, 32, 1, 13]),
                         {"DBCSR_AMD_MM_CLASSES": "2"}, "mm_numeric_f64_class["),
    "mid36_tail": ((36 * 9 + 20, 36 * 8 + 7, 36 * 9 + 30, 0.6, 0.6, 0.6, [1, 36], [1, 36], [1, 36]), {}, "mm_numeric_f64_mid<9,9>"),
    "mid_33_36": ((69 * 5, 69 * 5 + 33, 69 * 4, 0.6, 0.6, 0.6, [1, 33, 1, 36], [1, 36, 1, 33], [1, 33, 1, 36]), {}, "mm_numeric_f64_mid<9,9>"),
    "mid_30_40": ((70 * 5, 70 * 5 + 30, 70 * 4, 0.6, 0.6, 0.6, [1, 30, 1, 40], [1, 40, 1, 30], [1, 30, 1, 40]), {}, "mm_numeric_f64_mid<10,10>"),
}


@pytest.mark.parametrize("name", sorted(FILTER_CASES))
def test_filtered_multiply_with_the_kernels_norms(shims, name):
    """every one of these families leaves the block norms to the final filter of a filtered multiply (and reads launch-order work records)"""
    case, env, expect = FILTER_CASES[name]
    got, o = choose(shims, env, case, filter_active=True)
    assert got == expect and o["work"] and o["norms"] and o["leaves_norms"], (got, o)
    got, o = choose(shims, env, case)
    assert got == expect and o["work"] and not o["norms"] and not o["leaves_norms"]


def test_slab_kernel_classes_switch(shims):
    """tests/test_gpu_kernel_variants.py: DBCSR_AMD_MM_MID=0 / 3 with classes differ in which classes may take the slab kernel (mid_f64_serves' mode)"""
    for env, mode in (({}, 1), ({"DBCSR_AMD_MM_MID": "0"}, 0), ({"DBCSR_AMD_MM_MID": "3"}, 3), ({"DBCSR_AMD_MM_BIG": "0"}, 0), ({"DBCSR_AMD_MM_CLASS_G": "8"}, 0)):
        got, o = choose(shims, dict(env, DBCSR_AMD_MM_CLASSES="2"), CONFIG3_37)
        assert got == "mm_numeric_f64_class[" and o["mid_class_mode"] == mode, (env, o)


def test_flag_words_grids_and_lds(shims):
    """the flag word, grid and dynamic LDS size are kernel arguments the choice owns"""
    f, _ = facts_of(H2O)
    npos = 8 * f["order_len"]
    for kw, skip in (({}, 0), ({"retain": True, "skip_empty": True}, 1)):
        _, o = choose(shims, {}, H2O, **kw)                                        # exact-size kernel: dbg | 32 when blocks without products stay untouched
        assert o["flags"] == 32 * skip and o["grid"] == npos // o["ww"] and o["lds_bytes"] == o["ww"] * o["lds_wave"] * 8
        _, o = choose(shims, {"DBCSR_AMD_MM_KERNEL": "pipe"}, H2O, **kw)           # pipe: skip_empty itself, eight blocks per wave, four waves
        assert o["flags"] == skip and o["grid"] == (npos + 31) // 32 and o["lds_bytes"] == 4 * o["lds_wave"] * 8
        _, o = choose(shims, {"DBCSR_AMD_MM_F64_GROUP": "4"}, H2O, **kw)           # group: the launch for the other sizes leaves the dominant size alone
        assert o["flags"] == 64 + 32 * skip
        _, o = choose(shims, {"DBCSR_AMD_MM_BIG": "2"}, BIG_CASES["72cube"][0], **kw)
        assert o["flags"] == skip + 4 and o["grid"] == npos_of(BIG_CASES["72cube"][0])
        _, o = choose(shims, {}, cube(40), **kw)
        assert o["flags"] == skip and o["grid"] == npos_of(cube(40))
        _, o = choose(shims, {}, cube(4), **kw)
        assert o["flags"] == skip and o["grid"] == (npos_of(cube(4)) + 15) // 16
    for env in ({"DBCSR_AMD_MM_TILE": "2"}, {"DBCSR_AMD_MM_BAND": "2"}):
        name, o = choose(shims, env, H2O)
        assert o["flags"] == 64 and name.startswith("mm_numeric_f64_" + ("tile" if "DBCSR_AMD_MM_TILE" in env else "band"))
        assert choose(shims, env, H2O, retain=True, skip_empty=True)[0] == "mm_numeric_f64_hot<23,23,23>"   # (no in-place accumulation through them)
    _, o = choose(shims, {"DBCSR_AMD_MM_DBG": "3", "DBCSR_AMD_MM_LDS_PAD": "4096"}, H2O, retain=True, skip_empty=True)
    assert o["flags"] == (3 | 32) and o["lds_bytes"] == o["ww"] * o["lds_wave"] * 8 + 4096
    # 23^3: 9.5 KB per wave (mm_choose.h); a cube of a multiple of 16 stages with the padded pitch
    _, o = choose(shims, {}, H2O)
    assert (o["lds_a"], o["lds_wave"], o["maxt"]) == (552, 552 + 640, 3)
    _, o = choose(shims, {}, cube(32))
    assert o["lds_a"] == 34 * 32 and o["lds_wave"] == 34 * 32 + 8 * 144 + 2


def npos_of(case):
    return 8 * facts_of(case)[0]["order_len"]
