"""complex_8 block-sparse multiply on the device (kernel family mm_numeric_z64<MA,NC>, the _z entries of include/dbcsr_amd_mm.h,
dbcsr_multiply with complex128 matrices).

Reference for VALUES: dense numpy in complex128 -- A, B and C_in scattered to dense, R = beta*C_in + alpha*op(A)*op(B) (restricted to the
window for limits).  Reference for the BLOCK INDEX: the oracle's real multiply of the real parts (without a filter the pattern does not
depend on the values).  Value bar, element-wise:

    |got - R| <= 1e-12 * (|alpha| * (|op(A)| * |op(B)|) + |beta| * |C_in|)

with the absolute-value product computed the same dense way.  Derivation, not measurement: with at most ~300 summed terms per element both
the kernel and the numpy reference stay below (2n + 10) * u * sqrt(2) ~ 1e-13 of that bound, so the bar leaves 4x over the sum of both.  (A
strict relative error per element is the wrong measure: Re = sum ArBr - sum AiBi cancels.)  Imaginary parts of the inputs:
np.random.default_rng(seed).uniform(-1, 1) laid over the oracle's real matrices of the same pattern."""
import ctypes as C

import numpy as np
import pytest
import torch

from dbcsr_amd import lib as L
from dbcsr_amd.matrix import DbcsrMatrix, StreamHandle, _dtype_code
from dbcsr_amd.multiply import MultiplyEngine, dbcsr_multiply
from oracle import oracle as O
from tests.gpu_util import dev_to_bcsr, to_dev
from tests.test_oracle_limits import CASES, limit_case_matrices

pytestmark = pytest.mark.gpu

BAR = 1e-12


@pytest.fixture(scope="module")
def eng():
    return MultiplyEngine()


# ---- helpers ------------------------------------------------------------------------------------------------------------------------------
def with_imag(M, seed, real=True):
    """the oracle's real matrix with uniform(-1, 1) imaginary parts laid over it (real=False: purely imaginary, i * M)"""
    im = np.random.default_rng(seed).uniform(-1.0, 1.0, M.data.size)
    data = (M.data + 1j * im) if real else 1j * M.data
    return O.Bcsr(M.row_sizes, M.col_sizes, M.row_p, M.col_i, M.blk_p, data.astype(np.complex128))


def part(M, data):
    return O.Bcsr(M.row_sizes, M.col_sizes, M.row_p, M.col_i, M.blk_p, np.ascontiguousarray(data, np.float64))


def dense(M):
    return part(M, M.data.real).to_dense() + 1j * part(M, M.data.imag).to_dense()


def op(D, t):
    return D if t == "N" else (D.T if t == "T" else D.conj().T)


def reference(ta, tb, alpha, A, B, beta, Cm):
    """(R, bound): the dense result and the element-wise error scale of the bar"""
    Ad, Bd, Cd = op(dense(A), ta), op(dense(B), tb), dense(Cm)
    return beta * Cd + alpha * (Ad @ Bd), abs(alpha) * (np.abs(Ad) @ np.abs(Bd)) + abs(beta) * np.abs(Cd)


def block_mask(M):
    """True on the elements M's blocks cover"""
    return part(M, np.ones(M.data.size)).to_dense() != 0.0


def same_index(got, ref):
    assert np.array_equal(got.row_p, ref.row_p) and np.array_equal(got.col_i, ref.col_i) and np.array_equal(got.blk_p, ref.blk_p)


def within_bar(got, R, bound, where=None):
    """every stored element of got within the bar of R"""
    G, mask = dense(got), block_mask(got)
    if where is not None:
        mask = mask & where
    err, lim = np.abs(G - R)[mask], BAR * bound[mask]
    assert np.all(err <= lim), "worst element: error %.3e against a bar of %.3e" % (float(err[np.argmax(err - lim)]), float(lim[np.argmax(err - lim)]))


def index_reference(ta, tb, A, B, Cm, beta, retain):
    """the oracle's multiply of the real parts: block index and flop ('C' is 'T' there; only beta == 0 matters to the pattern)"""
    real = lambda t: "T" if t == "C" else t
    return O.multiply(real(ta), real(tb), 1.0, part(A, A.data.real), part(B, B.data.real), 0.0 if beta == 0 else 1.0, part(Cm, Cm.data.real),
                      retain_sparsity=retain)


def run_multiply(eng, ta, tb, alpha, A, B, beta, Cm, retain=False, **kw):
    dC = to_dev(Cm)
    flop = [0]
    dbcsr_multiply(ta, tb, alpha, to_dev(A), to_dev(B), beta, dC, retain_sparsity=retain, flop=flop, engine=eng, **kw)
    torch.cuda.synchronize()
    assert eng.last_kernel().startswith("mm_numeric_z64<"), eng.last_kernel()
    return dev_to_bcsr(dC), flop[0]


def check_case(eng, ta, tb, alpha, A, B, beta, Cm, retain=False):
    got, flop = run_multiply(eng, ta, tb, alpha, A, B, beta, Cm, retain)
    ref, info = index_reference(ta, tb, A, B, Cm, beta, retain)
    same_index(got, ref)
    assert flop == info["flop"]
    R, bound = reference(ta, tb, alpha, A, B, beta, Cm)
    within_bar(got, R, bound)
    return got


def complex_case(M, N, K, sp, bs_m, bs_n, bs_k, ta="N", tb="N", seed=1):
    real = lambda t: "T" if t == "C" else t
    A, B, Cm = O.perf_case(M, N, K, sp[0], sp[1], sp[2], bs_m, bs_n, bs_k, real(ta), real(tb))
    return with_imag(A, seed), with_imag(B, seed + 1), with_imag(Cm, seed + 2)


# ---- 1. transposes -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trans", ["NN", "TN", "NT", "CN", "NC", "CC", "TC"])
@pytest.mark.parametrize("alpha,beta,retain", [(1, 1, False), (-0.5 + 2j, 2 - 1j, False), (2j, 0, True)])
def test_transposes_and_conjugation(eng, trans, alpha, beta, retain):
    A, B, Cm = complex_case(230, 260, 200, (0.5, 0.6, 0.7), [1, 13, 1, 5], [1, 23, 1, 4], [1, 7, 1, 32], trans[0], trans[1])
    check_case(eng, trans[0], trans[1], alpha, A, B, beta, Cm, retain)
    if "C" in trans:   # 'C' and 'T' differ on these inputs by far more than the bar: a missing conjugation cannot pass
        R, bound = reference(trans[0], trans[1], alpha, A, B, beta, Cm)
        Rt, _ = reference(trans[0].replace("C", "T"), trans[1].replace("C", "T"), alpha, A, B, beta, Cm)
        assert np.max(np.abs(R - Rt) - 1e3 * BAR * bound) > 0.1


# ---- 2. / 3. block sizes: slab tails, tile edges, blocks above 32, a mix; the kernel name --------------------------------------------------------
@pytest.mark.parametrize("s", [1, 3, 4, 5, 8, 9, 16, 17, 23, 24, 32])
def test_uniform_blocks(eng, s):
    for k in (1, 7, 8, 9, 23):
        A, B, Cm = complex_case(6 * s + (s + 1) // 2, 5 * s, 7 * k + k // 2, (0.3, 0.3, 0.5), [1, s], [1, s], [1, k], seed=10 * s + k)
        check_case(eng, "N", "N", 0.75 - 0.5j, A, B, 1.5 + 0.25j, Cm)
        t = (s + 7) // 8
        assert eng.last_kernel() == "mm_numeric_z64<%d,%d>" % (t, t)


@pytest.mark.parametrize("mnk,inst", [((32, 9, 9), (4, 2)), ((5, 13, 23), (1, 2)), ((33, 33, 33), (4, 4)), ((40, 40, 40), (4, 4)), ((45, 67, 78), (4, 4))])
def test_rectangular_and_large_blocks(eng, mnk, inst):
    m, n, k = mnk
    A, B, Cm = complex_case(5 * m + m // 3, 4 * n + n // 2, 4 * k + 3, (0.3, 0.3, 0.5), [1, m], [1, n], [1, k], seed=m + n + k)
    check_case(eng, "N", "N", -1.25 + 0.5j, A, B, 0.5 - 2j, Cm)
    assert eng.last_kernel() == "mm_numeric_z64<%d,%d>" % inst


def test_mixed_sizes_in_one_matrix(eng):
    mix = [1, 13, 1, 23, 1, 32, 1, 40]
    A, B, Cm = complex_case(270, 250, 290, (0.4, 0.4, 0.6), mix, mix, mix, seed=77)
    check_case(eng, "N", "N", 1 + 1j, A, B, -1j, Cm)
    assert eng.last_kernel() == "mm_numeric_z64<4,4>"


def test_real_multiply_after_a_complex_one_on_the_same_engine(eng):
    A, B, Cm = O.perf_case(230, 260, 200, 0.5, 0.6, 0.7, [1, 13, 1, 5], [1, 23, 1, 4], [1, 7, 1, 32])
    check_case(eng, "N", "N", 1j, with_imag(A, 1), with_imag(B, 2), 1, with_imag(Cm, 3))
    ref, info = O.multiply("N", "N", -0.5, A, B, 2.0, Cm)
    dC, flop = to_dev(Cm), [0]
    dbcsr_multiply("N", "N", -0.5, to_dev(A), to_dev(B), 2.0, dC, flop=flop, engine=eng)
    torch.cuda.synchronize()
    assert eng.last_kernel().startswith("mm_numeric_f64"), eng.last_kernel()   # engine state does not leak between types
    got = dev_to_bcsr(dC)
    same_index(got, ref)
    assert flop[0] == info["flop"] and np.all(np.abs(got.data - ref.data) <= 1e-10 * np.maximum(np.abs(ref.data), 1.0))


# ---- 4. limits ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in CASES if c[0] in ("LIMITS_MIX_3", "LIMITS_ROW_3", "CUT_NEW")], ids=lambda c: c[0])
@pytest.mark.parametrize("beta_im", [0.0, 0.75])
def test_limits(eng, case, beta_im):
    Ar, Br, Cr = limit_case_matrices(case)
    _, _, _, retain, alpha, beta, _, _, _, lim = case
    alpha, beta = complex(alpha, -0.5), complex(beta, beta_im)
    A, B, Cm = with_imag(Ar, 21), with_imag(Br, 22), with_imag(Cr, 23)
    names = ("first_row", "last_row", "first_column", "last_column", "first_k", "last_k")
    got, flop = run_multiply(eng, "N", "N", alpha, A, B, beta, Cm, retain, **dict(zip(names, lim)))
    ref, info = O.multiply_limits("N", "N", 1.0, Ar, Br, 0.0 if beta == 0 else 1.0, Cr, lim, retain_sparsity=retain)
    same_index(got, ref)
    assert flop == info["flop"]
    Ad, Bd, Cd = dense(A), dense(B), dense(Cm)
    r, c, k = slice(lim[0] - 1, lim[1]), slice(lim[2] - 1, lim[3]), slice(lim[4] - 1, lim[5])
    R, bound, inside = Cd.copy(), np.abs(Cd), np.zeros(Cd.shape, bool)
    R[r, c] = beta * Cd[r, c] + alpha * (Ad[r, k] @ Bd[k, c])
    bound[r, c] = abs(beta) * np.abs(Cd[r, c]) + abs(alpha) * (np.abs(Ad[r, k]) @ np.abs(Bd[k, c]))
    inside[r, c] = True
    within_bar(got, R, bound, where=inside)
    # outside the window C is bit-identical to C_in
    G, stored = dense(got), block_mask(got)
    out = stored & ~inside
    assert out.any()
    assert np.array_equal(G[out].real.view(np.uint64), Cd[out].real.view(np.uint64)) and np.array_equal(G[out].imag.view(np.uint64), Cd[out].imag.view(np.uint64))


# ---- 5. filter --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [2.0, 40.0])
def test_filter_follows_the_real_rule(eng, eps):
    """Norms are sum re^2 + im^2: a complex matrix without imaginary parts is filtered exactly as the oracle filters the real one, and so is i * A
    (the product is then purely imaginary).  Values against the oracle's at the bar of the real filtered multiplies, 1e-10 relative."""
    A, B, Cm = O.perf_case(300, 260, 280, 0.5, 0.5, 0.5, [1, 5, 1, 13], [1, 7, 1, 9], [1, 4, 1, 23])
    ref, _ = O.multiply("N", "N", 1.0, A, B, 1.0, Cm, filter_eps=eps)
    z = lambda M: O.Bcsr(M.row_sizes, M.col_sizes, M.row_p, M.col_i, M.blk_p, M.data.astype(np.complex128))
    got, _ = run_multiply(eng, "N", "N", 1.0, z(A), z(B), 1.0, z(Cm), filter_eps=eps)
    same_index(got, ref)
    assert np.all(np.abs(got.data.real - ref.data) <= 1e-10 * np.maximum(np.abs(ref.data), 1.0)) and np.all(got.data.imag == 0.0)
    got, _ = run_multiply(eng, "N", "N", 1.0, with_imag(A, 0, real=False), z(B), 1.0, with_imag(Cm, 0, real=False), filter_eps=eps)
    same_index(got, ref)
    assert np.all(np.abs(got.data.imag - ref.data) <= 1e-10 * np.maximum(np.abs(ref.data), 1.0)) and np.all(got.data.real == 0.0)


# ---- 6. in-place accumulation -----------------------------------------------------------------------------------------------------------------------
def test_in_place_accumulation_over_two_halves_of_k(eng):
    A, B, Cm = complex_case(230, 260, 200, (0.5, 0.6, 0.7), [1, 13, 1, 5], [1, 23, 1, 4], [1, 7, 1, 32], seed=5)
    alpha, beta = 0.5 - 1.5j, 2 + 1j
    dA, dB, dC = to_dev(A), to_dev(B), to_dev(Cm)
    row_p, counts = eng.symbolic(dA, dB, dC)
    out = eng.init_c(beta, dC, row_p, counts, torch.complex128)
    torch.cuda.synchronize()
    koff = np.concatenate([[0], np.cumsum(A.col_sizes)])
    kb = A.nbc // 2
    pattern = lambda M: part(M, np.ones(M.data.size)).to_dense()
    blocks_of = lambda M: np.add.reduceat(np.add.reduceat(pattern(M), np.concatenate([[0], np.cumsum(M.row_sizes)])[:-1], 0),
                                          np.concatenate([[0], np.cumsum(M.col_sizes)])[:-1], 1) > 0
    PA, PB = blocks_of(A), blocks_of(B)
    untouched_seen = 0
    for k0, k1 in ((0, kb), (kb, A.nbc)):
        before = dev_to_bcsr(out)
        Ah = eng.cropped(dA, None, (int(koff[k0]), int(koff[k1]) - 1))
        Bh = eng.cropped(dB, (int(koff[k0]), int(koff[k1]) - 1), None)
        eng.accumulate(alpha, Ah, Bh, out)
        torch.cuda.synchronize()
        assert eng.last_kernel().startswith("mm_numeric_z64<")
        after = dev_to_bcsr(out)
        same_index(after, before)
        # blocks without a product in this pass keep their bits
        has = (PA[:, k0:k1].astype(np.int64) @ PB[k0:k1, :].astype(np.int64)) > 0
        rows = after.rows()
        for b in range(after.nblks):
            if not has[rows[b], after.col_i[b]]:
                ne = int(after.row_sizes[rows[b]]) * int(after.col_sizes[after.col_i[b]])
                sl = slice(int(after.blk_p[b]), int(after.blk_p[b]) + ne)
                assert np.array_equal(after.data[sl].view(np.uint64), before.data[sl].view(np.uint64))
                untouched_seen += 1
    assert untouched_seen > 0
    got = dev_to_bcsr(out)
    ref, _ = index_reference("N", "N", A, B, Cm, beta, False)
    same_index(got, ref)
    R, bound = reference("N", "N", alpha, A, B, beta, Cm)
    within_bar(got, R, bound)


# ---- 7. plan reuse ------------------------------------------------------------------------------------------------------------------------------------
def test_plan_reuse_and_reproducibility():
    e = MultiplyEngine()
    A, B, Cm = complex_case(23 * 9 + 16, 23 * 8 + 16, 23 * 10 + 16, (0.5, 0.5, 0.6), [1, 23], [1, 23], [1, 23], seed=9)
    dA, dB, dC = to_dev(A), to_dev(B), to_dev(Cm)

    def run(alpha, beta):
        out, _ = e.multiply_local(alpha, dA, dB, beta, dC)
        torch.cuda.synchronize()
        return dev_to_bcsr(out)

    first = run(1 - 1j, 0.5j)
    again = run(1 - 1j, 0.5j)
    assert e.plan_stats()[0] >= 1
    assert np.array_equal(first.data.view(np.uint64), again.data.view(np.uint64))   # the same multiply twice: identical bits
    dA.data.mul_(0.5 - 0.25j)   # other values in the same arrays, another alpha: the plan stands
    A2 = O.Bcsr(A.row_sizes, A.col_sizes, A.row_p, A.col_i, A.blk_p, A.data * (0.5 - 0.25j))
    reused = e.plan_stats()[0]
    got = run(-2 + 0.5j, 1.0)
    assert e.plan_stats()[0] == reused + 1
    same_index(got, first)
    R, bound = reference("N", "N", -2 + 0.5j, A2, B, 1.0, Cm)
    within_bar(got, R, bound)


# ---- 8. the native one-call entry ---------------------------------------------------------------------------------------------------------------------
def fetch(lib, ptr, count, dtype):
    out = np.empty(count, dtype)
    if count:
        assert lib.c_dbcsr_acc_memcpy_d2h(C.c_void_p(ptr), out.ctypes.data_as(C.c_void_p), C.c_size_t(out.nbytes), None) == 0
        assert lib.c_dbcsr_acc_device_synchronize() == 0
    return out


@pytest.mark.parametrize("trans", ["NN", "CT"])
def test_native_multiply_z(trans):
    E = MultiplyEngine()
    lib = E.L
    A, B, Cm = complex_case(230, 260, 200, (0.5, 0.6, 0.7), [1, 13, 1, 5], [1, 23, 1, 4], [1, 7, 1, 32], trans[0], trans[1], seed=3)
    alpha, beta = -0.5 + 2j, 2 - 1j
    dA, dB, dC = to_dev(A), to_dev(B), to_dev(Cm)
    a, b, c = dA.desc(), dB.desc(), dC.desc()
    out, flop = L.BcsrDesc(), C.c_int64(0)
    z = lambda x: (C.c_double * 2)(complex(x).real, complex(x).imag)
    rc = lib.dbcsr_amd_multiply_z(E.h, trans[0].encode(), trans[1].encode(), z(alpha), C.byref(a), C.byref(b), z(beta), C.byref(c), None, 0, 0.0,
                                  C.byref(out), C.byref(flop), None)
    assert rc == 0
    torch.cuda.synchronize()
    row_p = fetch(lib, out.row_p, out.nblkrows + 1, np.int32)
    nblks = int(out.nblks)
    assert row_p[-1] == nblks
    col_i, blk_p = fetch(lib, out.col_i, nblks, np.int32), fetch(lib, out.blk_p, nblks, np.int64)
    rows = np.repeat(np.arange(out.nblkrows), np.diff(row_p))
    nze = int((Cm.row_sizes[rows].astype(np.int64) * Cm.col_sizes[col_i]).sum())
    data = fetch(lib, out.data, nze, np.complex128)
    assert lib.dbcsr_amd_bcsr_release(C.byref(out)) == 0
    got = O.Bcsr(Cm.row_sizes, Cm.col_sizes, row_p, col_i, blk_p, data)
    ref, info = index_reference(trans[0], trans[1], A, B, Cm, beta, False)
    same_index(got, ref)
    assert flop.value == info["flop"]
    R, bound = reference(trans[0], trans[1], alpha, A, B, beta, Cm)
    within_bar(got, R, bound)


# ---- 9. conjugate transpose and fill -------------------------------------------------------------------------------------------------------------------
def test_conjugate_transpose_against_numpy(eng):
    A, _, _ = complex_case(230, 260, 200, (0.5, 0.6, 0.7), [1, 13, 1, 5], [1, 23, 1, 4], [1, 7, 1, 32], seed=4)
    dA = to_dev(A)
    for conj in (True, False):
        T = eng.transposed(dA, conjugate=conj)
        torch.cuda.synchronize()
        got = dev_to_bcsr(T)
        same_index(got, O.transposed(part(A, A.data.real)))
        assert np.array_equal(dense(got), dense(A).conj().T if conj else dense(A).T)


def test_fill_random_is_the_real_stream_in_pairs(eng):
    """zlarnv(idist = 1): the block's 2 m n doubles are the dlarnv stream of the block's seed -- the values of the real matrix with the same pattern,
    doubled row block sizes and 2 * blk_p"""
    A, _, _ = O.perf_case(230, 260, 200, 0.5, 0.6, 0.7, [1, 13, 1, 5], [1, 23, 1, 4], [1, 7, 1, 32])
    Z = to_dev(O.Bcsr(A.row_sizes, A.col_sizes, A.row_p, A.col_i, A.blk_p, np.zeros(A.data.size, np.complex128)))
    Rm = to_dev(O.Bcsr(2 * A.row_sizes, A.col_sizes, A.row_p, A.col_i, 2 * A.blk_p, np.zeros(2 * A.data.size, np.float64)))
    eng.fill_random(Z, 7)
    eng.fill_random(Rm, 7)
    torch.cuda.synchronize()
    z, r = Z.data.cpu().numpy().view(np.float64), Rm.data.cpu().numpy()
    assert z.size == r.size and np.array_equal(z, r) and np.all((z > 0.0) & (z < 1.0))


# ---- 10. refusals ----------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(eng):
    A, B, Cm = complex_case(60, 60, 60, (0.3, 0.3, 0.3), [1, 5], [1, 5], [1, 5])
    with pytest.raises(TypeError, match="complex_8"):
        _dtype_code(torch.complex64)
    c64 = lambda M: O.Bcsr(M.row_sizes, M.col_sizes, M.row_p, M.col_i, M.blk_p, M.data.astype(np.complex64))
    with pytest.raises(TypeError):
        dbcsr_multiply("N", "N", 1.0, to_dev(c64(A)), to_dev(c64(B)), 1.0, to_dev(c64(Cm)), engine=eng)
    with pytest.raises(TypeError):   # mixed real / complex operands
        dbcsr_multiply("N", "N", 1.0, to_dev(part(A, A.data.real)), to_dev(B), 1.0, to_dev(Cm), engine=eng)
    with pytest.raises(TypeError):   # complex scalars with real matrices
        dbcsr_multiply("N", "N", 1j, to_dev(part(A, A.data.real)), to_dev(part(B, B.data.real)), 1.0, to_dev(part(Cm, Cm.data.real)), engine=eng)
    for which in range(3):
        ms = [to_dev(A), to_dev(B), to_dev(Cm)]
        ms[which].symmetry = "S"
        with pytest.raises(NotImplementedError):
            dbcsr_multiply("N", "N", 1.0, ms[0], ms[1], 1.0, ms[2], engine=eng)
    from dbcsr_amd.cannon import CannonMultiply
    with pytest.raises(TypeError):
        CannonMultiply(60, 60, 60, (0.3, 0.3, 0.3), (1, 5), dtype=torch.complex128)
    dA = to_dev(A)
    out2, d = (C.c_double * 2)(), dA.desc()
    assert eng.L.dbcsr_amd_bcsr_checksum(eng.h, L.dbcsr_type_complex_8, C.byref(d), out2, StreamHandle().ptr) == -10
    st = StreamHandle()
    s = torch.ones(3, dtype=torch.int32, device="cuda")
    zb = torch.zeros(64, dtype=torch.complex128, device="cuda")
    assert eng.L.libsmm_acc_process(None, s.data_ptr(), 1, L.dbcsr_type_complex_8, zb.data_ptr(), zb.data_ptr(), zb.data_ptr(), 2, 2, 2, 80, 1, st.ptr,
                                    st.ptr) == -10
