"""Every compiled instance of the multiply kernel families that are instantiated from lists -- the 43 slab kernels mm_numeric_f64_mid<RB,CB>, the 16
workgroup kernels mm_numeric_f64_big<TM,TN>, the 16 complex kernels mm_numeric_z64<MA,NC> -- and the run-time compiled class kernels of the 24 SHAPES
of tests/test_gpu_class_mode.py, each run once on a small multiply against the CPU oracle with the kernel's name asserted.  The rows come from
tests/kernel_instances.py; tests/test_kernel_instances_cpu.py shows without a GPU that they reach every instance and what the reference says about them.

Per real case, on a fresh engine: the general multiply (alpha = 0.7, beta = 1.3, C_in holding some product blocks and lacking others), beta = 0,
retain_sparsity followed by a product accumulated IN PLACE (MultiplyEngine.accumulate: C blocks without products stay untouched), and for the slab
kernels a filtered multiply whose threshold no block of the reference sits on.  Index bit-exact, flop equal, values 1e-10 element-wise relative.
dbcsr_multiply itself never works in place (its product gets a data area of its own), so the canary check -- C's data area inside an allocation full
of canaries, pointer unmoved, every canary intact -- is made on the in-place accumulation, where the kernels write into the caller's memory."""
import re

import numpy as np
import pytest
import torch

from dbcsr_amd.multiply import MultiplyEngine, dbcsr_multiply
from oracle import oracle as O
from tests import kernel_instances as KI
from tests import test_gpu_class_mode
from tests.elementwise_ref import same_bits
from tests.gpu_util import dev_to_bcsr, rel_err, to_dev
from tests.test_gpu_block_inverse import CANARY, GUARD, placed
from tests.test_gpu_complex_multiply import check_case, complex_case

pytestmark = pytest.mark.gpu

ENV = ("DBCSR_AMD_MM_KERNEL", "DBCSR_AMD_MM_HOT", "DBCSR_AMD_MM_TINY", "DBCSR_AMD_MM_SYMBOLIC", "DBCSR_AMD_MM_CLASSES", "DBCSR_AMD_MM_WG_WAVES",
       "DBCSR_AMD_MM_BIG", "DBCSR_AMD_MM_MID", "DBCSR_AMD_MM_KCHUNKS", "DBCSR_AMD_MM_SMALL", "DBCSR_AMD_MM_WORK", "DBCSR_AMD_MM_EXPECT_FILTER")
TABLES = {"mid": KI.mid_cases(), "mid_class": KI.mid_class_cases(), "big": KI.big_cases(), "class": KI.class_cases()}
Z64 = KI.z64_cases()
REAL = [(t, n) for t in ("mid", "mid_class", "big") for n in sorted(TABLES[t])]
SLAB = [(t, n) for t, n in REAL if t != "big"]
IDS = lambda v: v if isinstance(v, str) else None
_operands = {}


def operands(table, name):
    """(A, B, C_in) of a case, made once and shared (nothing writes to them)"""
    if (table, name) not in _operands:
        _operands[table, name] = O.perf_case(*TABLES[table][name][0])
    return _operands[table, name]


def engine(monkeypatch, table):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    if table in ("mid_class", "class"):
        monkeypatch.setenv("DBCSR_AMD_MM_CLASSES", "2")
    return MultiplyEngine()


def assert_kernel(eng, table, name):
    """the instance by its exact name; a class-mode shape: exactly one class took the slab kernel, and of the classes the name reports only the shape's
    own is one the slab kernel serves -- so that class held C blocks and ran <rb, cb>"""
    got, shape = eng.last_kernel(), TABLES[table][name][1]
    if table == "mid":
        assert got == "mm_numeric_f64_mid<%d,%d>" % shape, got
    elif table == "big":
        assert got == "mm_numeric_f64_big<%d,%d>" % shape, got
    else:
        m = re.fullmatch(r"mm_numeric_f64_class\[(\d+) jit \+ (?:(\d+) slab \+ )?(\d+) generic launches; m \{(\d+),(\d+),(\d+)\} n \{(\d+),(\d+),(\d+)\} k \{.*\}\]", got)
        assert m, got
        v = [int(x or 0) for x in m.groups()]
        served = [(a, b) for a in v[3:6] for b in v[6:9] if a and b and KI.mid_serves(a, b, 1)]
        assert v[1] == 1 and len(served) == 1 and ((served[0][0] + 3) // 4, (served[0][1] + 3) // 4) == shape, got


def check(out, ref, tol=1e-10):
    assert np.array_equal(out.row_p, ref.row_p) and np.array_equal(out.col_i, ref.col_i) and np.array_equal(out.blk_p, ref.blk_p)
    assert rel_err(out.data, ref.data) <= tol


def multiply_and_check(monkeypatch, table, name, alpha, beta, eps=None):
    eng = engine(monkeypatch, table)
    A, B, Cm = operands(table, name)
    ref, info = O.multiply("N", "N", alpha, A, B, beta, Cm, filter_eps=eps or 0.0)
    dA, dB, dC = to_dev(A), to_dev(B), to_dev(Cm)
    flop = [0]
    dbcsr_multiply("N", "N", alpha, dA, dB, beta, dC, filter_eps=eps, flop=flop, engine=eng)
    torch.cuda.synchronize()
    assert_kernel(eng, table, name)
    assert flop[0] == info["flop"]
    check(dev_to_bcsr(dC), ref)
    return ref


@pytest.mark.parametrize("table,name", REAL, ids=IDS)
def test_general_multiply(monkeypatch, table, name):
    multiply_and_check(monkeypatch, table, name, 0.7, 1.3)


@pytest.mark.parametrize("table,name", REAL, ids=IDS)
def test_beta_zero(monkeypatch, table, name):
    multiply_and_check(monkeypatch, table, name, 0.7, 0.0)


@pytest.mark.parametrize("table,name", REAL, ids=IDS)
def test_retain_sparsity_then_accumulate_in_place(monkeypatch, table, name):
    eng = engine(monkeypatch, table)
    A, B, Cm = operands(table, name)
    ref, _ = O.multiply("N", "N", 1.0, A, B, 1.0, Cm, retain_sparsity=True)
    dA, dB, dC = to_dev(A), to_dev(B), to_dev(Cm)
    dbcsr_multiply("N", "N", 1.0, dA, dB, 1.0, dC, retain_sparsity=True, engine=eng)
    torch.cuda.synchronize()
    assert_kernel(eng, table, name)
    check(dev_to_bcsr(dC), ref)
    # the second product in place, C's data area between canaries (16-byte aligned: GUARD elements of 8 bytes into the allocation)
    ref2, info2 = O.multiply("N", "N", -0.5, A, B, 1.0, ref, retain_sparsity=True)
    dP, big = placed(dC, 0)
    ptr, before = dP.data.data_ptr(), dP.data.cpu().numpy()
    assert ptr % 16 == 0 and ptr == big.data_ptr() + 8 * GUARD
    counts = eng.accumulate(-0.5, dA, dB, dP)
    torch.cuda.synchronize()
    assert_kernel(eng, table, name)
    assert counts.flop == info2["flop"] and dP.data.data_ptr() == ptr
    check(dev_to_bcsr(dP), ref2)
    n, whole = dP.data.numel(), big.cpu().numpy()
    assert same_bits(whole[:GUARD], np.full(GUARD, CANARY)) and same_bits(whole[GUARD + n:], np.full(whole.size - GUARD - n, CANARY))
    # blocks without a product in the call keep their bits
    lengths = KI.block_pattern(A).astype(np.int64) @ KI.block_pattern(B).astype(np.int64)
    rows, after, untouched = ref.rows(), dP.data.cpu().numpy(), 0
    for b in np.flatnonzero(lengths[rows, ref.col_i] == 0):
        sl = slice(int(ref.blk_p[b]), int(ref.blk_p[b]) + int(ref.row_sizes[rows[b]]) * int(ref.col_sizes[ref.col_i[b]]))
        assert same_bits(after[sl], before[sl])
        untouched += 1
    assert untouched > 0


@pytest.mark.parametrize("table,name", SLAB, ids=IDS)
def test_filtered_multiply_with_the_kernels_norms(monkeypatch, table, name):
    """the slab kernel computes a block's norm from its accumulators through the same per-instance visit<> that drains them and drops the block itself:
    the pattern must be the reference's (no block sits on the threshold: tests/test_kernel_instances_cpu.py)"""
    A, B, Cm = operands(table, name)
    full, _ = O.multiply("N", "N", KI.FILTER_ALPHA, A, B, KI.FILTER_BETA, Cm)
    ref = multiply_and_check(monkeypatch, table, name, KI.FILTER_ALPHA, KI.FILTER_BETA, eps=KI.filter_eps(full))
    assert 0.25 * full.nblks <= ref.nblks <= 0.75 * full.nblks


@pytest.fixture(scope="module")
def z64_engine():
    return MultiplyEngine()


@pytest.mark.parametrize("name", sorted(Z64))
def test_complex_instance(monkeypatch, z64_engine, name):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    (M, N, K, sp, bs_m, bs_n, bs_k), inst = Z64[name]
    A, B, Cm = complex_case(M, N, K, sp, bs_m, bs_n, bs_k, seed=100 * inst[0] + 10 * inst[1] + bs_k[1])
    check_case(z64_engine, "N", "N", -1.25 + 0.5j, A, B, 0.5 - 2j, Cm)
    assert z64_engine.last_kernel() == "mm_numeric_z64<%d,%d>" % inst


def test_the_class_shapes_are_the_at_scale_tests_list():
    assert KI.class_shapes() == [tuple(s) for s in test_gpu_class_mode.SHAPES]


@pytest.mark.parametrize("name", list(TABLES["class"]))
def test_class_kernels_small(monkeypatch, name):
    """the 24 shapes of the at-scale walk (tests/test_gpu_class_mode.py) at a size that runs by default: the time of a case is hiprtc's, see DESIGN.md 4e"""
    eng = engine(monkeypatch, "class")
    A, B, Cm = operands("class", name)
    ref, info = O.multiply("N", "N", 0.7, A, B, 1.3, Cm)
    dA, dB, dC = to_dev(A), to_dev(B), to_dev(Cm)
    flop = [0]
    dbcsr_multiply("N", "N", 0.7, dA, dB, 1.3, dC, flop=flop, engine=eng)
    torch.cuda.synchronize()
    got = re.match(r"mm_numeric_f64_class\[(\d+) jit \+ ", eng.last_kernel())
    assert got and int(got.group(1)) >= 1, eng.last_kernel()
    assert flop[0] == info["flop"]
    check(dev_to_bcsr(dC), ref)
