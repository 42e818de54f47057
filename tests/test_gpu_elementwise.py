"""Element-wise operations on two patterns on the device (dbcsr_amd/operations.py: dbcsr_hadamard_product, dbcsr_copy, dbcsr_function_of_elements; the
section of that name in include/dbcsr_amd_mm.h; kernels of dbcsr_amd/csrc/mm_elementwise.h) for float64, float32 and complex128.

Reference: numpy on dicts of blocks (tests/elementwise_ref.py, checked against dense numpy in tests/test_elementwise_cpu.py).  The INDEX of a product is
the reference's: sorted block columns per row, blk_p the running sum of the block sizes.  Bars:
  hadamard   float64 / float32: bit for bit a * b in the type.  complex128: |got - ref| <= 4 u |a| |b| per element, u = 2^-53 (elementwise_ref.hadamard_bar
             has the derivation).  An assumed value of exactly 1 copies A's block bit for bit.
  copy       bit for bit, the sign of the zeros included; every element the index does not name keeps its bits.
  functions  per element C u |ref| + 2 u |f'(y)| (|a1 x| + |a0|) against the formula in np.longdouble rounded once to the type, y = a1 x + a0; the second
             term is the rounding of y itself.  float32: C = 1, u = 2^-24 (the value is formed in double: one rounding to float32 is half a unit).
             float64: C = C64 below, u = 2^-53 -- twice the largest excess over the second term that any case of test_function_of_elements showed on
             an MI355X, rounded up (profiles/elementwise.txt lists the maxima per function).
Matrices: the oracle's generator with the mixes [1, 13, 1, 5] x [1, 23, 1, 4] at 230 x 260 (two counters, sparsity 0.5 each), the tiny-block matrix
([1, 1, 1, 3], 76 block columns, fill 0.9: rows of more than 64 blocks, blocks at odd offsets), hand-made patterns on 5 x 5 blocks, and operands whose
blk_p leaves gaps filled with a canary."""
import ctypes as C

import numpy as np
import pytest
import torch

from dbcsr_amd import lib as L
from dbcsr_amd import operations as OPS
from dbcsr_amd.matrix import DbcsrMatrix, StreamHandle
from dbcsr_amd.multiply import MultiplyEngine, _z, dbcsr_multiply
from dbcsr_amd.operations import dbcsr_add, dbcsr_copy, dbcsr_frobenius_norm, dbcsr_function_of_elements, dbcsr_hadamard_product
from oracle import oracle as O
from tests import elementwise_ref as R
from tests import far_arena as FA
from tests.gpu_util import dev_to_bcsr, to_dev

pytestmark = pytest.mark.gpu

DTYPES, IDS, F64, F32, Z64 = R.DTYPES, R.IDS, R.F64, R.F32, R.Z64
C64 = 8   # the float64 constant of the functions' bar: see the module's text and profiles/elementwise.txt
FUNCS = {name: getattr(OPS, "dbcsr_func_" + name) for name in R.FUNC_NAMES}


@pytest.fixture(scope="module")
def eng():
    return MultiplyEngine()


class NoLibrary:
    """in the place of an engine: whatever is asked of it fails, so a refusal that is reached with it came before any call of the library"""

    def __getattr__(self, name):
        raise AssertionError("the library was about to be called (%s)" % name)


def dev(M):
    """the host matrix on the device; a matrix whose blk_p leaves gaps names fewer elements than its data area has"""
    d = to_dev(M)
    d.nze = int(R.sizes_of(M).sum())
    return d


def empty_like(M):
    return dev(R.subset(M, lambda r, c: False))


def same_index(got, ref):
    assert np.array_equal(got.row_p, ref.row_p), "row_p"
    assert np.array_equal(got.col_i, ref.col_i), "col_i"
    assert np.array_equal(got.blk_p, ref.blk_p), "blk_p"


def index_of(d):
    return (d.index_stamp(), d.row_p, d.col_i, d.blk_p, d.data)


def index_kept(d, before):
    return d.index_stamp() == before[0] and d.row_p is before[1] and d.col_i is before[2] and d.blk_p is before[3] and d.data is before[4]


def assumed(dtype):
    """the assumed values of B's missing blocks: none, exactly 1, and one that multiplies"""
    return [None, 1, 0.5 - 2j if np.dtype(dtype).kind == "c" else -0.5]


def assert_product(got, A, B, assume):
    dtype = A.data.dtype
    ref, scale = R.reference_hadamard(A, B, assume)
    same_index(got, ref)
    assert got.data.dtype == ref.data.dtype and got.data.size == ref.data.size
    if np.dtype(dtype).kind != "c":
        assert R.same_bits(got.data, ref.data), "real data: a * b in the type, bit for bit"
        return
    err, bar = np.abs(got.data - ref.data), R.hadamard_bar(dtype, scale)
    worst = int(np.argmax(err - bar)) if err.size else 0
    assert np.all(err <= bar), "worst element: error %.3e against a bar of %.3e" % (float(err[worst]), float(bar[worst]))
    if assume == 1:
        bg, ba, bb = R.blocks_of(got), R.blocks_of(A), R.blocks_of(B)
        assert all(R.same_bits(bg[k], ba[k]) for k in ba if k not in bb), "an assumed 1 copies A's block bit for bit"


def check_hadamard(eng, A, B, assume=None, where="new", dA=None, dB=None, expect_same=False):
    """one product with C a third matrix ("new"), A ("a") or B ("b"); returns the device matrices and the host result"""
    dA = dev(A) if dA is None else dA
    dB = dev(B) if dB is None else dB
    dC = {"new": empty_like(A), "a": dA, "b": dB}[where] if isinstance(where, str) else where
    before = index_of(dC)
    same = dbcsr_hadamard_product(dA, dB, dC, b_assume_value=assume, engine=eng)
    torch.cuda.synchronize()
    assert same is expect_same
    if not expect_same:
        assert dC.row_p is not before[1] and dC.col_i is not before[2] and dC.blk_p is not before[3], "two patterns: C has new index tensors"
    got = dev_to_bcsr(dC)
    assert dC.packed
    assert_product(got, A, B, assume)
    return dA, dB, dC, got


# ---- 1. hadamard: two patterns --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("which", ["mixed", "tiny"])
def test_hadamard_of_independent_patterns(eng, dtype, which):
    A, B = (R.typed(M, dtype, 1 + i) for i, M in enumerate((R.mixed_pair if which == "mixed" else R.tiny_pair)()))
    for v in assumed(dtype):
        _, _, _, got = check_hadamard(eng, A, B, v)
        assert got.nblks == (A.nblks if v is not None else len(set(R.blocks_of(A)) & set(R.blocks_of(B))))
    check_hadamard(eng, B, A)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", sorted(R.EDGE_PATTERNS))
def test_hadamard_edge_patterns(eng, dtype, name):
    A, B = R.edge_pair(name, dtype)
    for v in assumed(dtype):
        _, _, dC, got = check_hadamard(eng, A, B, v, expect_same=(name == "both_empty"))
        if v is None and name in ("a_empty", "b_empty", "both_empty", "disjoint"):
            assert got.nblks == 0 and not got.row_p.any() and dC.data.numel() == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_hadamard_aliasing_on_two_patterns(eng, dtype):
    A, B = (R.typed(M, dtype, 3 + i) for i, M in enumerate(R.mixed_pair()))
    for v in (None, assumed(dtype)[2]):
        ref = check_hadamard(eng, A, B, v)[3]
        for where in ("a", "b"):
            got = check_hadamard(eng, A, B, v, where=where)[3]
            same_index(got, ref)
            assert R.same_bits(got.data, ref.data), "C is %s: the result of a separate C" % where


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_hadamard_of_operands_with_holes(eng, dtype):
    A, B = (R.typed(M, dtype, 5 + i) for i, M in enumerate(R.mixed_pair()))
    hA, hB = R.with_holes(A), R.with_holes(B)
    assert (hA.blk_p % 2).any() and not R.named_mask(hA).all()
    for X, Y in ((hA, B), (A, hB), (hA, hB)):
        for v in (None, assumed(dtype)[2]):
            dX, dY, _, _ = check_hadamard(eng, X, Y, v)
            assert R.same_bits(dX.data.cpu().numpy(), X.data) and R.same_bits(dY.data.cpu().numpy(), Y.data), "the operands are only read"


@pytest.mark.parametrize("dtype,symmetry", [(F64, "S"), (F32, "S"), (Z64, "H")], ids=["fp64_S", "fp32_S", "z64_H"])
def test_hadamard_on_stored_triangles(eng, dtype, symmetry):
    sizes = O.make_block_sizes(120, [1, 13, 1, 5])
    A, B = (R.typed(R.subset(O.make_random_matrix(sizes, sizes, 0.4, O.RANDMAT_SEED_INIT + 65 + i), lambda r, c: c >= r), dtype, 7 + i)
            for i in range(2))
    dA, dB, dC = dev(A), dev(B), empty_like(A)
    for d in (dA, dB, dC):
        d.symmetry = symmetry
    check_hadamard(eng, A, B, dA=dA, dB=dB, where=dC)
    assert dC.symmetry == symmetry


# ---- 2. hadamard: the same pattern ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("which", ["mixed", "tiny"])
def test_hadamard_same_pattern_in_place(eng, dtype, which):
    A = R.typed((R.mixed_pair if which == "mixed" else R.tiny_pair)()[0], dtype, 9)
    B = R.with_data(A, R.typed(A, dtype, 10).data[::-1].copy() if np.dtype(dtype).kind == "c" else (A.data[::-1] * 1.5).astype(dtype))
    for where in ("a", "b"):   # C is an operand: its index tensors and its stamp stay
        dA, dB = dev(A), dev(B)
        dC = dA if where == "a" else dB
        before = index_of(dC)
        check_hadamard(eng, A, B, where=where, dA=dA, dB=dB, expect_same=True)
        assert index_kept(dC, before)
    dC = dev(R.with_data(A, np.full(A.data.size, 3.0, dtype)))   # a third matrix that already has that index
    before = index_of(dC)
    dA, dB, _, _ = check_hadamard(eng, A, B, where=dC, expect_same=True)
    assert index_kept(dC, before)
    assert R.same_bits(dA.data.cpu().numpy(), A.data) and R.same_bits(dB.data.cpu().numpy(), B.data)
    dC = empty_like(A)   # a third matrix with another index: it adopts a new one
    before = index_of(dC)
    check_hadamard(eng, A, B, assumed(dtype)[2], where=dC, expect_same=True)
    assert dC.col_i is not before[2] and dC.nblks == A.nblks


def test_hadamard_of_different_patterns_is_not_in_place(eng):
    A, B = (R.typed(M, F64, 1 + i) for i, M in enumerate(R.mixed_pair()))
    dA = dev(A)
    before = index_of(dA)
    check_hadamard(eng, A, B, where="a", dA=dA, expect_same=False)
    assert dA.index_stamp() != before[0] and dA.data is not before[4]


# ---- 3. the plan survives -----------------------------------------------------------------------------------------------------------------------------------
def test_a_saved_plan_survives_the_elementwise_operations(monkeypatch):
    monkeypatch.delenv("DBCSR_AMD_MM_PLAN", raising=False)
    eng = MultiplyEngine()
    sizes = O.make_block_sizes(160, [1, 13, 1, 5])
    A, B, Y = (R.typed(O.make_random_matrix(sizes, sizes, 0.5, O.RANDMAT_SEED_INIT + 70 + i), F64, i) for i in range(3))
    dA, dB = dev(A), dev(B)
    dC = empty_like(A)
    dbcsr_multiply("N", "N", 1.0, dA, dB, 0.0, dC, engine=eng)
    dbcsr_multiply("N", "N", 1.0, dA, dB, 0.0, dC, engine=eng)
    assert eng.plan_stats() == (1, 1)
    X1, X2 = (R.typed(M, F64, 1 + i) for i, M in enumerate(R.mixed_pair()))
    check_hadamard(eng, X1, X2)                                   # two patterns: the union add in this place costs the plan
    stamp = dA.index_stamp()
    dbcsr_copy(dA, dev(Y), keep_sparsity=True, engine=eng)        # onto A from a matrix of another pattern
    dbcsr_function_of_elements(dB, OPS.dbcsr_func_tanh, 0.25, -0.5, engine=eng)
    assert dA.index_stamp() == stamp
    dbcsr_multiply("N", "N", 1.0, dA, dB, 0.0, dC, engine=eng)
    assert eng.plan_stats() == (2, 1), "a multiply after hadamard / copy / function must reuse its plan"
    torch.cuda.synchronize()
    hA, hB = dev_to_bcsr(dA), dev_to_bcsr(dB)
    assert R.same_bits(hA.data, R.reference_copy_onto(Y, A))
    ref = R.dense(hA) @ R.dense(hB)
    scale = np.abs(R.dense(hA)) @ np.abs(R.dense(hB))
    assert np.all(np.abs(R.dense(dev_to_bcsr(dC)) - ref) <= 1e-10 * np.maximum(scale, 1e-300))


# ---- 4. copy onto a pattern -----------------------------------------------------------------------------------------------------------------------------------
def check_copy_onto(eng, A, B, stream=None):
    dA, dB = dev(A), dev(B)
    before = index_of(dB)
    if stream is not None:
        torch.cuda.synchronize()
    dbcsr_copy(dB, dA, keep_sparsity=True, engine=eng, stream=stream)
    (stream.synchronize if stream is not None else torch.cuda.synchronize)()
    assert index_kept(dB, before), "B keeps its index tensors, its data tensor and its stamp"
    got = dB.data.cpu().numpy()
    ref = R.reference_copy_onto(A, B)
    assert R.same_bits(got, ref), "A's block bit for bit, +0.0 where A has none, every other element as it was"
    assert R.same_bits(dA.data.cpu().numpy(), A.data)
    ba, mask = R.blocks_of(A), R.named_mask(B)
    lacking = [v for k, v in R.blocks_of(R.with_data(B, got)).items() if k not in ba]
    if lacking:
        z = np.concatenate(lacking)
        assert not z.any() and not np.signbit(z.real).any() and not np.signbit(z.imag).any(), "+0.0"
    assert np.all(got[~mask] == R.CANARY) if (~mask).any() else True
    return got


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("which", ["mixed", "tiny"])
def test_copy_onto_a_pattern(eng, dtype, which):
    A, B = (R.typed(M, dtype, 11 + i) for i, M in enumerate((R.mixed_pair if which == "mixed" else R.tiny_pair)()))
    check_copy_onto(eng, A, B)
    check_copy_onto(eng, R.with_holes(A), R.with_holes(B))      # the canaries in B's holes are kept
    other = R.with_data(A, np.full(A.data.size, -3.5, dtype))
    check_copy_onto(eng, A, other)                              # the same pattern
    part = R.with_holes(R.subset(other, lambda r, c: (r + c) % 3 != 0))
    assert 0 < part.nblks < A.nblks
    check_copy_onto(eng, A, part)                               # A's pattern a superset of B's: A restricted
    got = check_copy_onto(eng, R.subset(A, lambda r, c: False), B)   # A empty: B is all zeros
    assert B.nblks and not got.any()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", sorted(R.EDGE_PATTERNS))
def test_copy_onto_edge_patterns(eng, dtype, name):
    A, B = R.edge_pair(name, dtype)
    check_copy_onto(eng, A, B)
    check_copy_onto(eng, B, R.with_holes(A))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_copy_without_keep_sparsity(eng, dtype):
    A, B = (R.typed(M, dtype, 14 + i) for i, M in enumerate(R.mixed_pair()))
    dA, dB = dev(R.with_holes(A)), dev(B)
    dA.symmetry = "H" if np.dtype(dtype).kind == "c" else "S"   # (a label here: it is copied too)
    dbcsr_copy(dB, dA, engine=eng)
    torch.cuda.synchronize()
    for x, y in zip(dB.to_host(), dA.to_host()):
        assert R.same_bits(x, y)
    assert dB.nze == dA.nze and dB.symmetry == dA.symmetry and dB.data is not dA.data and dB.col_i is not dA.col_i


# ---- 5. functions of elements ---------------------------------------------------------------------------------------------------------------------------------
def run_function(eng, X, name, a0, a1, dX=None):
    dX = dev(X) if dX is None else dX
    before = index_of(dX)
    dbcsr_function_of_elements(dX, FUNCS[name], a0, a1, a2=0.0 if name == "sin" else None, engine=eng)   # (an a2 of 0 is no a2)
    torch.cuda.synchronize()
    assert index_kept(dX, before)
    return dX


def function_excess(X, name, a0, a1, got):
    """the largest (|got - ref| - second term of the bar) / (u |ref|) over the elements the index names, after the checks on the inputs"""
    mask = R.named_mask(X)
    x = X.data[mask]
    y = np.abs(R.y_of(x, a0, a1))
    lo, hi = R.y_range(name)
    assert y.min() >= lo and y.max() <= hi, "the inputs of %s must keep |y| in [%g, %g]" % (name, lo, hi)
    assert R.same_bits(got[~mask], X.data[~mask]), "holes keep their bits"
    excess, ref = R.function_errors(name, x, a0, a1, got[mask])
    assert np.all(np.isfinite(ref)) and np.all(np.isfinite(got[mask]))
    return float(excess.max())


@pytest.mark.parametrize("dtype", [F64, F32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("a0,a1", R.PARAMS)
@pytest.mark.parametrize("name", R.FUNC_NAMES)
def test_function_of_elements(eng, name, a0, a1, dtype):
    X = R.with_holes(R.function_input(R.mixed_pair()[0], name, a0, a1, dtype))
    dX = run_function(eng, X, name, a0, a1)
    worst = function_excess(X, name, a0, a1, dX.data.cpu().numpy())
    print("function %s a0 %g a1 %g %s: largest (|got - ref| - 2 u |f'| (|a1 x| + |a0|)) / (u |ref|) = %.3f" % (name, a0, a1, np.dtype(dtype).name, worst))
    assert worst <= (1 if dtype == F32 else C64)


def test_function_of_elements_on_tiny_blocks(eng):
    X = R.function_input(R.tiny_pair()[0], "sin", 0.25, -0.5, F32)   # blocks at odd offsets: heads and tails of the 16-byte walk
    dX = run_function(eng, X, "sin", 0.25, -0.5)
    assert function_excess(X, "sin", 0.25, -0.5, dX.data.cpu().numpy()) <= 1


def test_function_of_elements_refuses_what_it_does_not_offer():
    A = R.mixed_pair()[0]
    dA, dZ = dev(A), dev(R.typed(A, Z64))
    for func in (5, 6, 14, 99, -1, 1.0, "tanh", None):
        with pytest.raises(NotImplementedError):
            dbcsr_function_of_elements(dA, func, engine=NoLibrary())
    with pytest.raises(NotImplementedError):
        dbcsr_function_of_elements(dA, OPS.dbcsr_func_tanh, a2=1.0, engine=NoLibrary())
    with pytest.raises(NotImplementedError):
        dbcsr_function_of_elements(dZ, OPS.dbcsr_func_tanh, engine=NoLibrary())
    assert R.same_bits(dA.data.cpu().numpy(), A.data)


# ---- 6. the two-call protocol and the C entries' answers ----------------------------------------------------------------------------------------------------
def raw_count(eng, dA, dB, assume=False):
    row_p = torch.empty(dA.nblkrows + 1, dtype=torch.int32, device="cuda")
    nb, nz, same = C.c_int64(), C.c_int64(), C.c_int32()
    a, b = dA.desc(), dB.desc()
    rc = eng.L.dbcsr_amd_bcsr_hadamard_count(eng.h, C.byref(a), C.byref(b), 1 if assume else 0, row_p.data_ptr(), C.byref(nb), C.byref(nz), C.byref(same),
                                             StreamHandle().ptr)
    return rc, row_p, nb.value, nz.value, same.value


def raw_apply(eng, dA, dB, row_p, nb, nz, value=None):
    out = DbcsrMatrix(dA.row_blk_size, dA.col_blk_size, row_p, torch.empty(nb, dtype=torch.int32, device="cuda"),
                      torch.empty(nb, dtype=torch.int64, device="cuda"), torch.empty(nz, dtype=dA.dtype, device="cuda"))
    a, b, d = dA.desc(), dB.desc(), out.desc(out=True)
    rc = eng.L.dbcsr_amd_bcsr_hadamard_apply(eng.h, dA.dtype_code, C.byref(a), C.byref(b), None if value is None else _z(value), C.byref(d), StreamHandle().ptr)
    torch.cuda.synchronize()
    return rc, out


def test_one_apply_per_count_and_nothing_between_disturbs_it():
    eng = MultiplyEngine()
    A, B = (R.typed(M, F64, 1 + i) for i, M in enumerate(R.mixed_pair()))
    X, Y = (R.typed(M, F64, 3 + i) for i, M in enumerate(R.tiny_pair()))
    dA, dB = dev(A), dev(B)
    row_p = torch.zeros(dA.nblkrows + 1, dtype=torch.int32, device="cuda")
    assert raw_apply(eng, dA, dB, row_p, 0, 0)[0] == -1, "an apply without a count"
    rc, row_p, nb, nz, same = raw_count(eng, dA, dB)
    assert (rc, same) == (0, 0)
    # a norm and a union add of other matrices between the two halves
    dX, dY = dev(X), dev(Y)
    dbcsr_frobenius_norm(dX, engine=eng)
    assert dbcsr_add(dX, dY, 1.0, 1.0, engine=eng) is False
    rc, out = raw_apply(eng, dA, dB, row_p, nb, nz)
    assert rc == 0
    assert_product(dev_to_bcsr(out), A, B, None)
    assert raw_apply(eng, dA, dB, row_p, nb, nz)[0] == -1, "a second apply after one count"
    # operands whose block counts differ from the counted ones, and an assumed value the count was not told of
    rc, row_p, nb, nz, _ = raw_count(eng, dA, dB)
    assert raw_apply(eng, dA, dev(R.subset(B, lambda r, c: (r + c) % 2 == 0)), row_p, nb, nz)[0] == -1
    rc, row_p, nb, nz, _ = raw_count(eng, dA, dB)
    assert raw_apply(eng, dA, dB, row_p, nb, nz, value=2.0)[0] == -1
    # a destination on an operand's data area, two patterns
    rc, row_p, nb, nz, _ = raw_count(eng, dA, dB)
    a, b, d = dA.desc(), dB.desc(), dA.desc()
    assert eng.L.dbcsr_amd_bcsr_hadamard_apply(eng.h, dA.dtype_code, C.byref(a), C.byref(b), None, C.byref(d), StreamHandle().ptr) == -1
    torch.cuda.synchronize()
    assert R.same_bits(dA.data.cpu().numpy(), A.data)


def test_a_pending_add_is_not_disturbed_by_a_whole_hadamard_product():
    eng = MultiplyEngine()
    A, B = (R.typed(M, F64, 1 + i) for i, M in enumerate(R.mixed_pair()))
    X, Y = (R.typed(M, F64, 3 + i) for i, M in enumerate(R.tiny_pair()))
    dA, dB = dev(A), dev(B)
    a, b = dA.desc(), dB.desc()
    row_p = torch.empty(dA.nblkrows + 1, dtype=torch.int32, device="cuda")
    nb, nz, same = C.c_int64(), C.c_int64(), C.c_int32()
    st = StreamHandle()
    assert eng.L.dbcsr_amd_bcsr_add_count(eng.h, C.byref(a), C.byref(b), 0, row_p.data_ptr(), C.byref(nb), C.byref(nz), C.byref(same), st.ptr) == 0
    assert same.value == 0
    check_hadamard(eng, X, Y)
    check_hadamard(eng, X, Y, 0.75)
    out = DbcsrMatrix(dA.row_blk_size, dA.col_blk_size, row_p, torch.empty(nb.value, dtype=torch.int32, device="cuda"),
                      torch.empty(nb.value, dtype=torch.int64, device="cuda"), torch.empty(nz.value, dtype=dA.dtype, device="cuda"))
    d = out.desc(out=True)
    assert eng.L.dbcsr_amd_bcsr_add_apply(eng.h, dA.dtype_code, _z(1.0), C.byref(a), _z(1.0), C.byref(b), C.byref(d), st.ptr) == 0
    torch.cuda.synchronize()
    got = dev_to_bcsr(out)
    ba, bb = R.blocks_of(A), R.blocks_of(B)
    ref = R.from_blocks(A.row_sizes, A.col_sizes, {k: (ba[k] + bb[k] if k in ba and k in bb else ba.get(k, bb.get(k))) for k in set(ba) | set(bb)}, F64)
    same_index(got, ref)
    assert R.same_bits(got.data, ref.data)


def test_c_entries_refuse_bad_arguments(eng):
    A, B = (R.typed(M, F64, 1 + i) for i, M in enumerate(R.mixed_pair()))
    T = R.typed(R.tiny_pair()[0], F64)
    dA, dB, dT = dev(A), dev(B), dev(T)
    a, b, t = dA.desc(), dB.desc(), dT.desc()
    Lb, h, st = eng.L, eng.h, StreamHandle().ptr
    row_p = torch.empty(dA.nblkrows + 1, dtype=torch.int32, device="cuda")
    nb, nz, same = C.c_int64(), C.c_int64(), C.c_int32()
    args = (row_p.data_ptr(), C.byref(nb), C.byref(nz), C.byref(same), st)
    assert Lb.dbcsr_amd_bcsr_hadamard_count(None, C.byref(a), C.byref(b), 0, *args) == -1
    assert Lb.dbcsr_amd_bcsr_hadamard_count(h, None, C.byref(b), 0, *args) == -1
    assert Lb.dbcsr_amd_bcsr_hadamard_count(h, C.byref(a), C.byref(b), 0, None, *args[1:]) == -1
    assert Lb.dbcsr_amd_bcsr_hadamard_count(h, C.byref(a), C.byref(t), 0, *args) == -1
    assert Lb.dbcsr_amd_bcsr_hadamard_apply(h, L.dbcsr_type_complex_4, C.byref(a), C.byref(b), None, C.byref(a), st) == -10
    assert Lb.dbcsr_amd_bcsr_hadamard_apply(h, L.dbcsr_type_real_8, C.byref(a), None, None, C.byref(a), st) == -1
    assert Lb.dbcsr_amd_bcsr_copy_onto(h, L.dbcsr_type_real_8, None, C.byref(b), st) == -1
    assert Lb.dbcsr_amd_bcsr_copy_onto(h, L.dbcsr_type_real_8, C.byref(t), C.byref(b), st) == -1
    assert Lb.dbcsr_amd_bcsr_copy_onto(h, 99, C.byref(a), C.byref(b), st) == -10
    assert Lb.dbcsr_amd_bcsr_function_of_elements(h, L.dbcsr_type_real_8, None, 1, 0.0, 1.0, st) == -1
    for func in (5, 6, 14, 15, -1):
        assert Lb.dbcsr_amd_bcsr_function_of_elements(h, L.dbcsr_type_real_8, C.byref(a), func, 0.0, 1.0, st) == -1
    assert Lb.dbcsr_amd_bcsr_function_of_elements(h, L.dbcsr_type_complex_8, C.byref(a), 1, 0.0, 1.0, st) == -10
    assert Lb.dbcsr_amd_bcsr_function_of_elements(h, 99, C.byref(a), 1, 0.0, 1.0, st) == -10
    torch.cuda.synchronize()
    assert R.same_bits(dA.data.cpu().numpy(), A.data) and R.same_bits(dB.data.cpu().numpy(), B.data)


def test_operations_refuse_mismatches_before_any_call():
    A, B = R.mixed_pair()
    no = NoLibrary()

    def other(what):
        """a matrix that does not go with A: another data type, other block sizes, another symmetry"""
        d = dev({"dtype": R.typed(A, F32), "sizes": R.tiny_pair()[0], "symmetry": B}[what])
        d.symmetry = "S" if what == "symmetry" else "N"
        return d

    def sym(M, s):
        d = dev(M)
        d.symmetry = s
        return d

    for what, error in (("dtype", TypeError), ("sizes", ValueError), ("symmetry", ValueError)):
        with pytest.raises(error):
            dbcsr_hadamard_product(dev(A), other(what), dev(A), engine=no)
        with pytest.raises(error):
            dbcsr_hadamard_product(dev(A), dev(B), other(what), engine=no)
        with pytest.raises(error):
            dbcsr_copy(other(what), dev(A), keep_sparsity=True, engine=no)
    for s in ("A", "K"):
        with pytest.raises(ValueError):
            dbcsr_hadamard_product(sym(A, s), sym(B, s), sym(A, s), engine=no)
    with pytest.raises(TypeError):
        dbcsr_hadamard_product(dev(A), dev(B), dev(A), b_assume_value=1j, engine=no)
    dA, dB = dev(A), dev(B)
    with pytest.raises(ValueError):
        dbcsr_copy(dA, dA, keep_sparsity=True, engine=no)
    view = DbcsrMatrix(dA.row_blk_size, dA.col_blk_size, dB.row_p, dB.col_i, dB.blk_p, dA.data[8:])   # another matrix in A's data area
    with pytest.raises(ValueError):
        dbcsr_copy(view, dA, keep_sparsity=True, engine=no)
    with pytest.raises(TypeError):
        dbcsr_copy(other("dtype"), dA, engine=no)
    with pytest.raises(ValueError):
        dbcsr_copy(other("sizes"), dA, engine=no)


# ---- 7. a side stream -----------------------------------------------------------------------------------------------------------------------------------------
def test_on_a_side_stream(eng):
    A, B = (R.typed(M, Z64, 1 + i) for i, M in enumerate(R.mixed_pair()))
    s = torch.cuda.Stream()
    dA, dB, dC = dev(A), dev(B), empty_like(A)
    torch.cuda.synchronize()
    assert dbcsr_hadamard_product(dA, dB, dC, engine=eng, stream=s) is False
    s.synchronize()
    assert_product(dev_to_bcsr(dC), A, B, None)
    check_copy_onto(eng, A, R.with_holes(B), stream=s)


# ---- 8. block offsets at and above 2^32 elements ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def arena():
    torch.cuda.reset_peak_memory_stats()
    a = FA.arena()
    yield a
    if a is not None:
        a.release()
        del a
    torch.cuda.empty_cache()


def far_pair(arena, A, B, dtype):
    """A and B with their blocks spread over the arena's zones (plan "blocks": the high bytes vary from block to block), or a skip by the arena's rule"""
    if arena is None:
        pytest.skip("the device has less than %d bytes free: no far arena" % (FA.ARENA_SMALL + FA.MARGIN))
    if np.dtype(dtype).kind == "c" and arena.nbytes < FA.ARENA_LARGE:
        pytest.skip("complex128 offsets above 2^32 need the arena of %d bytes: %d bytes missing" % (FA.ARENA_LARGE, FA.ARENA_LARGE - arena.nbytes))
    far = FA.Far(arena.view(dtype))
    dA = far.on_device(A, FA.place(A, dtype, "blocks", 0, arena.nbytes))
    dB = far.on_device(B, FA.place(B, dtype, "blocks", 1, arena.nbytes)) if B is not None else None
    far.seal()
    assert far.max_high_byte() >= 1, "offsets cross 2^32 elements"
    return far, dA, dB


@pytest.mark.parametrize("dtype", [F64, Z64], ids=["fp64", "z64"])
def test_hadamard_of_far_operands(eng, arena, dtype):
    A, B = (R.typed(M, dtype, 1 + i) for i, M in enumerate(R.mixed_pair()))
    far, dA, dB = far_pair(arena, A, B, dtype)
    dC = empty_like(A)
    assert dbcsr_hadamard_product(dA, dB, dC, b_assume_value=assumed(dtype)[2], engine=eng) is False
    torch.cuda.synchronize()
    assert_product(dev_to_bcsr(dC), A, B, assumed(dtype)[2])
    assert far.guards_kept()


@pytest.mark.parametrize("dtype", [F64, Z64], ids=["fp64", "z64"])
def test_copy_onto_a_far_pattern(eng, arena, dtype):
    """source and destination both live in the arena, which dbcsr_copy takes for one data area (it is one tensor): the C entry is called as dbcsr_copy
    calls it"""
    A, B = (R.typed(M, dtype, 1 + i) for i, M in enumerate(R.mixed_pair()))
    far, dA, dB = far_pair(arena, A, B, dtype)
    with pytest.raises(ValueError):
        dbcsr_copy(dB, dA, keep_sparsity=True, engine=eng)
    stamp = dB.index_stamp()
    a, b = dA.desc(), dB.desc()
    assert eng.L.dbcsr_amd_bcsr_copy_onto(eng.h, dA.dtype_code, C.byref(a), C.byref(b), StreamHandle().ptr) == 0
    torch.cuda.synchronize()
    assert dB.index_stamp() == stamp
    assert R.same_bits(FA.blocks_to_host(dB).data, R.reference_copy_onto(A, B))
    assert R.same_bits(FA.blocks_to_host(dA).data, A.data) and far.guards_kept()


def test_function_of_far_elements(eng, arena):
    """(the functions take real data only: float64)"""
    name, (a0, a1) = "tanh", R.PARAMS[1]
    X = R.function_input(R.mixed_pair()[0], name, a0, a1, F64)
    far, dX, _ = far_pair(arena, X, None, F64)
    run_function(eng, X, name, a0, a1, dX=dX)
    got = FA.blocks_to_host(dX).data
    excess, _ = R.function_errors(name, X.data, a0, a1, got)
    assert excess.max() <= C64 and far.guards_kept()
