"""The kernels compiled at run time (dbcsr_amd/csrc/mm_jit.hip) reach hiprtc as TEXT: every header of csrc/ that mm_exact.h or
smm_exact.h reaches by #include must be in the Makefile's jit_sources.inc list and in hname[] of mm_jit.hip.  A forgotten header
shows up only on the GPU, as a hiprtc failure and then a silent fall-back to the generic class kernel -- so the lists are checked
here, and the two translation units are compiled (device code only, no GPU needed) with the preamble mm_jit.hip writes."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dbcsr_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
ENTRY_HEADERS = ("mm_exact.h", "smm_exact.h")


def reachable_headers():
    """the files of csrc/ that the two entry headers include, directly or not (the entry headers among them)"""
    seen, todo = [], list(ENTRY_HEADERS)
    while todo:
        name = todo.pop()
        if name in seen:
            continue
        seen.append(name)
        for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(os.path.join(CSRC, name)).read(), re.M):
            if os.path.exists(os.path.join(CSRC, inc)):
                todo.append(os.path.normpath(inc))
    return sorted(seen)


def makefile_jit_list():
    text = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ")
    variables = dict(re.findall(r"^(\w+)\s*:?=\s*(.*)$", text, re.M))
    m = re.search(r"^jit_sources\.inc:.*\n\t(.*gen_jit_sources\.py\s+\$@\s+(.*))$", text, re.M)
    assert m, "the jit_sources.inc rule of the Makefile was not found"
    words = re.sub(r"\$\((\w+)\)", lambda v: variables[v.group(1)], m.group(2)).split()
    return [os.path.basename(w) for w in words]


def test_reachable_headers_are_in_the_makefile_list():
    listed = makefile_jit_list()
    missing = [h for h in reachable_headers() if h not in listed]
    assert not missing, "headers reachable from %s but not in the jit_sources.inc rule: %s" % (ENTRY_HEADERS, missing)


def test_reachable_headers_are_in_hname():
    text = open(os.path.join(CSRC, "mm_jit.hip")).read()
    m = re.search(r"hname\[\]\s*=\s*\{([^}]*)\}", text)
    assert m, "hname[] of mm_jit.hip was not found"
    names = re.findall(r'"([^"]+)"', m.group(1))
    missing = [h for h in reachable_headers() if h not in names]
    assert not missing, "headers reachable from %s but not in hname[]: %s" % (ENTRY_HEADERS, missing)
    srcs = re.search(r"hsrc\[\]\s*=\s*\{([^}]*)\}", text)
    assert srcs and [s.strip() for s in srcs.group(1).split(",")] == ["kJitSrc_" + n.replace(".h", "") for n in names], "hsrc[] and hname[] disagree"


CLASS_TU = ("#define DBCSR_AMD_JIT_M %d\n#define DBCSR_AMD_JIT_N %d\n#define DBCSR_AMD_JIT_K0 %d\n#define DBCSR_AMD_JIT_K1 %d\n"
            "#define DBCSR_AMD_JIT_K2 %d\n#define DBCSR_AMD_JIT_MINW %d\n#define DBCSR_AMD_JIT_G %d\n#include \"mm_exact.h\"\n")
STACK_TU = ("#define DBCSR_AMD_JIT_SM %d\n#define DBCSR_AMD_JIT_SN %d\n#define DBCSR_AMD_JIT_SK %d\n#define DBCSR_AMD_JIT_SBT %d\n"
            "#define DBCSR_AMD_JIT_MINW %d\n#include \"smm_exact.h\"\n")


@pytest.mark.parametrize("name,text,entry", [
    ("class_23_23_g1", CLASS_TU % (23, 23, 23, 13, 0, 3, 1), "mm_numeric_f64_class"),
    ("class_23_23_g8", CLASS_TU % (23, 23, 23, 13, 0, 2, 8), "mm_numeric_f64_class"),
    ("stack_23_23_23", STACK_TU % (23, 23, 23, 0, 3), "smm_stack_f64_exact"),
    ("stack_23_23_13_bt", STACK_TU % (23, 23, 13, 1, 3), "smm_stack_f64_exact"),
])
def test_translation_units_compile_for_gfx950(tmp_path, name, text, entry):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    src = tmp_path / (name + ".hip")
    src.write_text(text)
    co = tmp_path / (name + ".co")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "--cuda-device-only", "--no-gpu-bundle-output", "-O3", "-std=c++17", "-munsafe-fp-atomics", "-Wall", "-Werror",
                        "-Wno-unused-function", "-I", CSRC, "-c", str(src), "-o", str(co)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    assert entry.encode() in co.read_bytes(), "the code object does not hold %s" % entry
