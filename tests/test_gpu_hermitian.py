"""Hermitian ('H') and antihermitian ('K') complex_8 matrices on the device: the twin / desymmetrize kernel for 16-byte elements (twin_fill_z64), the
kind codes 0 ... 3 of the C ABI, dbcsr_multiply with 'H' / 'K' operands and product matrices, dbcsr_amd_multiply_symmetric_c_z.

Inputs: the oracle's make_random_matrix_symmetric(sizes, sparsity, counter, 'S') gives the pattern and the real parts, the imaginary parts are
np.random.default_rng(seed).uniform(-1, 1) laid over them (with_imag of tests/test_gpu_complex_multiply.py).

References.  TWIN / DESYMMETRIZE, bit for bit: the twin of a block is made of sign flips and copies, and for 'H' the real part moves as 'S' and the
imaginary part as 'A' ('K': the reverse; 'S' / 'A': the same kind on both parts) -- so the expected matrix is the oracle's desymmetrize / move_to_twin of
the two parts.  MULTIPLY VALUES: dense numpy in complex128 under the bar of tests/test_gpu_complex_multiply.py,
|got - R| <= 1e-12 * (|alpha| * (|op A| * |op B|) + |beta| * |C_in|) element-wise (derived there, not measured).  A stored block X at (r, c) of a product
matrix with symmetry becomes beta * X + alpha * P(r, c) when it stays in canonical (checkerboard) form and twin(beta * twin(X) + alpha * P(c, r)) when it
moves (P = op(A) * op(B)); the bound's product block is then the one the formula uses, P(c, r) transposed.  INDEX AND FLOP: the oracle's real multiply
of the real parts, c_symmetry = 'S' for a product with symmetry (the pattern does not depend on the kind)."""
import ctypes as C

import numpy as np
import pytest
import torch

from dbcsr_amd import lib as L
from dbcsr_amd.matrix import StreamHandle
from dbcsr_amd.multiply import MultiplyEngine, dbcsr_multiply
from oracle import oracle as O
from tests.gpu_util import dev_to_bcsr, to_dev
from tests.test_gpu_complex_multiply import BAR, dense, fetch, op, part, same_index, with_imag, within_bar

pytestmark = pytest.mark.gpu

# which of the oracle's two real kinds moves the (real, imaginary) part
PARTS = {"S": ("S", "S"), "A": ("A", "A"), "H": ("S", "A"), "K": ("A", "S")}
MIX = [1, 13, 1, 5, 1, 23, 1, 32, 1, 33, 1, 40, 1, 1]   # rectangular off-diagonal blocks, the edge sizes of the 32 x 32 LDS image, blocks above it
SMALL = [1, 13, 1, 5, 1, 23]


@pytest.fixture(scope="module")
def eng():
    return MultiplyEngine()


# ---- helpers ------------------------------------------------------------------------------------------------------------------------------
def triangle(sizes, sparsity, counter, seed):
    return with_imag(O.make_random_matrix_symmetric(sizes, sparsity, counter, "S"), seed)


def general(rs, cs, sparsity, counter, seed):
    return with_imag(O.make_random_matrix(rs, cs, sparsity, counter), seed)


def join(R, I):
    assert np.array_equal(R.row_p, I.row_p) and np.array_equal(R.col_i, I.col_i) and np.array_equal(R.blk_p, I.blk_p)
    return O.Bcsr(R.row_sizes, R.col_sizes, R.row_p, R.col_i, R.blk_p, R.data + 1j * I.data)


def expected_full(M, sym):
    re, im = PARTS[sym]
    return join(O.desymmetrize(part(M, M.data.real), re), O.desymmetrize(part(M, M.data.imag), im))


def expected_moved(M, move, sym):
    re, im = PARTS[sym]
    return join(O.move_to_twin(part(M, M.data.real), move, re), O.move_to_twin(part(M, M.data.imag), move, im))


to_canonical = lambda r, c: r != c and bool(O.checker_tr(r + 1, c + 1))
to_triangle = lambda r, c: r > c


def same_bits(got, ref):
    same_index(got, ref)
    g, r = np.ascontiguousarray(got.data, np.complex128), np.ascontiguousarray(ref.data, np.complex128)
    assert g.size == r.size and np.array_equal(g.view(np.uint64), r.view(np.uint64))


def dev(M, sym="N"):
    d = to_dev(M)
    d.symmetry = sym
    return d


def diagonal_only(sizes, seed):
    sizes = np.asarray(sizes, np.int32)
    nze = sizes.astype(np.int64) ** 2
    rng = np.random.default_rng(seed)
    return O.Bcsr(sizes, sizes, np.arange(len(sizes) + 1), np.arange(len(sizes)), np.concatenate([[0], np.cumsum(nze)[:-1]]),
                  rng.uniform(-1, 1, int(nze.sum())) + 1j * rng.uniform(-1, 1, int(nze.sum())))


def empty(sizes):
    sizes = np.asarray(sizes, np.int32)
    return O.Bcsr(sizes, sizes, np.zeros(len(sizes) + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros(0, np.complex128))


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def with_hermitian_diagonal(M):
    """the stored triangle with its diagonal blocks made hermitian: the real parts of the oracle's 'S' matrix are symmetric there already, the imaginary
    parts become antisymmetric"""
    data, rows = M.data.copy(), M.rows()
    for b in np.nonzero(rows == M.col_i)[0]:
        m = int(M.row_sizes[rows[b]])
        blk = data[M.blk_p[b]:M.blk_p[b] + m * m].reshape(m, m)
        data[M.blk_p[b]:M.blk_p[b] + m * m] = (blk.real + 0.5j * (blk.imag - blk.imag.T)).reshape(-1)
    return O.Bcsr(M.row_sizes, M.col_sizes, M.row_p, M.col_i, M.blk_p, data)


@pytest.fixture(scope="module")
def mats():
    mixed = O.make_block_sizes(2 * 147, MIX)          # 14 block rows
    rows70 = np.asarray([3, 5] * 35, np.int32)        # 70 block rows: three bitmap words per row
    return {"mixed": triangle(mixed, 0.5, 11, 1), "rows70": triangle(rows70, 0.7, 12, 2), "diagonal": diagonal_only(mixed, 3), "empty": empty(mixed)}


# ---- 1. desymmetrize ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "rows70", "diagonal", "empty"])
def test_desymmetrize_is_bit_exact(eng, mats, name):
    M = mats[name]
    if name in ("mixed", "rows70"):
        assert M.nblks > M.nbr and np.any(M.rows() != M.col_i)
    for sym in ("H", "K"):   # through the mirror
        got = eng.desymmetrized(dev(M, sym))
        torch.cuda.synchronize()
        same_bits(dev_to_bcsr(got), expected_full(M, sym))
    full = {}
    for sym in ("S", "A", "H", "K"):   # kinds 0 ... 3 through dbcsr_amd_bcsr_twin_apply on complex data
        got = eng.twin_moved(dev(M), 0, sym)
        torch.cuda.synchronize()
        full[sym] = dev_to_bcsr(got)
        same_bits(full[sym], expected_full(M, sym))
    if name in ("mixed", "rows70"):   # a missing conjugation cannot pass
        assert not np.array_equal(full["H"].data, full["S"].data) and not np.array_equal(full["K"].data, full["A"].data)
        assert not np.array_equal(full["H"].data, full["K"].data)


# ---- 2. canonical form and back ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "rows70"])
@pytest.mark.parametrize("sym", ["H", "K"])
def test_canonical_form_and_back(eng, mats, name, sym):
    M = mats[name]
    canon = eng.twin_moved(dev(M), 1, sym)
    torch.cuda.synchronize()
    hc = dev_to_bcsr(canon)
    same_bits(hc, expected_moved(M, to_canonical, sym))
    assert np.any(hc.rows() > hc.col_i)   # some block did move
    back = eng.twin_moved(canon, 2, sym)
    torch.cuda.synchronize()
    hb = dev_to_bcsr(back)
    same_bits(hb, expected_moved(hc, to_triangle, sym))
    same_bits(hb, M)   # mode 2 after mode 1: the input, bit for bit


# ---- 3. an unpacked source -------------------------------------------------------------------------------------------------------------------------
def test_unpacked_source(eng, mats):
    M, gap = mats["mixed"], 7
    nze = (M.row_sizes[M.rows()].astype(np.int64) * M.col_sizes[M.col_i])
    blk_p = M.blk_p + gap * (1 + np.arange(M.nblks))
    data = np.full(int(M.data.size + gap * (M.nblks + 2)), 777.0 - 555.0j, np.complex128)
    for b in range(M.nblks):
        data[blk_p[b]:blk_p[b] + nze[b]] = M.data[M.blk_p[b]:M.blk_p[b] + nze[b]]
    U = dev(O.Bcsr(M.row_sizes, M.col_sizes, M.row_p, M.col_i, blk_p, data), "H")
    U.nze = int(M.data.size)
    assert not U.packed
    got = eng.desymmetrized(U)
    packed = eng.desymmetrized(dev(M, "H"))
    torch.cuda.synchronize()
    assert got.packed
    same_bits(dev_to_bcsr(got), dev_to_bcsr(packed))
    same_bits(dev_to_bcsr(got), expected_full(M, "H"))


# ---- 4. operands -----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def operand_case():
    sizes = O.make_block_sizes(4 * 41, SMALL)   # 12 block rows
    return {"sizes": sizes, "T1": triangle(sizes, 0.5, 21, 4), "T2": triangle(sizes, 0.6, 22, 5), "G1": general(sizes, sizes, 0.5, 23, 6),
            "G2": general(sizes, sizes, 0.6, 24, 7), "C": general(sizes, sizes, 0.7, 25, 8)}


@pytest.mark.parametrize("trans", ["NN", "TN", "NC", "CC"])
@pytest.mark.parametrize("symm", ["HN", "NK", "HK", "KH"])
def test_hermitian_operands(eng, operand_case, symm, trans):
    oc = operand_case
    A, B, Cm = (oc["T1"] if symm[0] != "N" else oc["G1"]), (oc["T2"] if symm[1] != "N" else oc["G2"]), oc["C"]
    alpha, beta = -0.5 + 2j, 2 - 1j
    dC, flop = dev(Cm), [0]
    dbcsr_multiply(trans[0], trans[1], alpha, dev(A, symm[0]), dev(B, symm[1]), beta, dC, flop=flop, engine=eng)
    torch.cuda.synchronize()
    assert eng.last_kernel().startswith("mm_numeric_z64<"), eng.last_kernel()
    got = dev_to_bcsr(dC)
    fa = expected_full(A, symm[0]) if symm[0] != "N" else A   # desymmetrized BEFORE op()
    fb = expected_full(B, symm[1]) if symm[1] != "N" else B
    real = lambda t: "T" if t == "C" else t
    ref, info = O.multiply(real(trans[0]), real(trans[1]), 1.0, part(fa, fa.data.real), part(fb, fb.data.real), 1.0, part(Cm, Cm.data.real))
    same_index(got, ref)
    assert flop[0] == info["flop"]
    Ad, Bd, Cd = op(dense(fa), trans[0]), op(dense(fb), trans[1]), dense(Cm)
    within_bar(got, beta * Cd + alpha * (Ad @ Bd), abs(alpha) * (np.abs(Ad) @ np.abs(Bd)) + abs(beta) * np.abs(Cd))


# ---- 5. products with the symmetry -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def product_case():
    sizes, ksizes = O.make_block_sizes(4 * 41, SMALL), O.make_block_sizes(190, [1, 7, 1, 32])
    return {"sizes": sizes, "A": general(sizes, ksizes, 0.5, 31, 9), "B": general(sizes, ksizes, 0.5, 32, 10),
            "C": with_hermitian_diagonal(triangle(sizes, 0.6, 33, 11)), "SA": general(sizes, sizes, 0.5, 34, 12), "SB": general(sizes, sizes, 0.5, 35, 13)}


@pytest.mark.parametrize("retain", [False, True])
def test_hermitian_product_is_the_triangle_of_the_full_product(eng, product_case, retain):
    A, Cm = product_case["A"], product_case["C"]
    alpha, beta = -0.5, 2.0
    dC, flop = dev(Cm, "H"), [0]
    dbcsr_multiply("N", "C", alpha, dev(A), dev(A), beta, dC, retain_sparsity=retain, flop=flop, engine=eng)
    torch.cuda.synchronize()
    assert eng.last_kernel().startswith("mm_numeric_z64<"), eng.last_kernel()
    got = dev_to_bcsr(dC)
    ref, info = O.multiply("N", "T", 1.0, part(A, A.data.real), part(A, A.data.real), 1.0, part(Cm, Cm.data.real), retain_sparsity=retain, c_symmetry="S")
    same_index(got, ref)
    assert flop[0] == info["flop"] and np.all(got.rows() <= got.col_i)
    Ad, Cd = dense(A), dense(expected_full(Cm, "H"))
    assert np.array_equal(Cd, Cd.conj().T)   # (the input: C_in is hermitian, diagonal blocks included)
    within_bar(got, beta * Cd + alpha * (Ad @ Ad.conj().T), abs(alpha) * (np.abs(Ad) @ np.abs(Ad).T) + abs(beta) * np.abs(Cd))


def test_antihermitian_product_is_the_triangle_of_the_full_product(eng, product_case):
    """A B^H - B A^H, accumulated in two multiplies into an empty 'K' matrix"""
    A, B, sizes = product_case["A"], product_case["B"], product_case["sizes"]
    ra, rb = part(A, A.data.real), part(B, B.data.real)
    dC, f1, f2 = dev(empty(sizes), "K"), [0], [0]
    dbcsr_multiply("N", "C", 1.0, dev(A), dev(B), 0.0, dC, flop=f1, engine=eng)
    dbcsr_multiply("N", "C", -1.0, dev(B), dev(A), 1.0, dC, flop=f2, engine=eng)
    torch.cuda.synchronize()
    got = dev_to_bcsr(dC)
    r1, i1 = O.multiply("N", "T", 1.0, ra, rb, 0.0, part(empty(sizes), np.zeros(0)), c_symmetry="S")
    r2, i2 = O.multiply("N", "T", 1.0, rb, ra, 1.0, r1, c_symmetry="S")
    same_index(got, r2)
    assert (f1[0], f2[0]) == (i1["flop"], i2["flop"])
    Ad, Bd = dense(A), dense(B)
    R = Ad @ Bd.conj().T - Bd @ Ad.conj().T
    within_bar(got, R, np.abs(Ad) @ np.abs(Bd).T + np.abs(Bd) @ np.abs(Ad).T)


# ---- 6. a product without the symmetry, complex scalars: where each conjugate goes ----------------------------------------------------------------------
@pytest.mark.parametrize("sym", ["H", "K"])
def test_product_without_the_symmetry_follows_the_two_case_formula(eng, product_case, sym):
    A, B, Cm = product_case["SA"], product_case["SB"], product_case["C"]
    alpha, beta = -0.5 + 2j, 2 - 1j
    twin = (lambda Y: Y.conj().T) if sym == "H" else (lambda Y: -Y.conj().T)
    dC, flop = dev(Cm, sym), [0]
    dbcsr_multiply("N", "N", alpha, dev(A), dev(B), beta, dC, flop=flop, engine=eng)
    torch.cuda.synchronize()
    got = dev_to_bcsr(dC)
    ref, info = O.multiply("N", "N", 1.0, part(A, A.data.real), part(B, B.data.real), 1.0, part(Cm, Cm.data.real), c_symmetry="S")
    same_index(got, ref)
    assert flop[0] == info["flop"]
    Ad, Bd, Cd = dense(A), dense(B), dense(Cm)   # Cd: the stored triangle, zero where a block is new
    P, Pabs = Ad @ Bd, np.abs(Ad) @ np.abs(Bd)
    R, bound = np.zeros_like(Cd), np.zeros(Cd.shape)
    off, rows, moved = offsets(Cm.row_sizes), got.rows(), np.zeros(Cd.shape, bool)
    for b in range(got.nblks):
        r, c = int(rows[b]), int(got.col_i[b])
        rr, cc = slice(off[r], off[r + 1]), slice(off[c], off[c + 1])
        X = Cd[rr, cc]
        if r != c and O.checker_tr(r + 1, c + 1):   # the block lives at (c, r) during the multiply
            R[rr, cc] = twin(beta * twin(X) + alpha * P[cc, rr])
            bound[rr, cc] = abs(beta) * np.abs(X) + abs(alpha) * Pabs[cc, rr].T
            moved[rr, cc] = True
        else:
            R[rr, cc] = beta * X + alpha * P[rr, cc]
            bound[rr, cc] = abs(beta) * np.abs(X) + abs(alpha) * Pabs[rr, cc]
    assert moved.any() and (bound[~moved] > 0).any()
    within_bar(got, R, bound)
    # on the blocks that move the formula's two cases are far apart on these inputs: a conjugate in the wrong place cannot pass
    wrong = beta * Cd + alpha * P
    assert np.max((np.abs(R - wrong) - 1e3 * BAR * bound)[moved]) > 0.1


# ---- 7. filter_eps --------------------------------------------------------------------------------------------------------------------------------------
def test_filter_with_a_hermitian_product(eng):
    """The final block filter on a hermitian product.  Three of A's twelve block rows are scaled by 1e-4, so the norms of the product's blocks fall into
    classes four decades apart, the boundary between the two larger ones near 40 % of the sorted list; eps sits in the geometric middle of the widest gap between neighbouring norms in the middle half of the sorted list.  Conditions on the
    INPUT, asserted below: that gap is at least 1e-6 relative (no block at the threshold), and no block product of a kept block comes near the on-the-fly
    rule ||A(i,k)|| * ||alpha * B(k,j)|| < eps / #blocks of A's row i (a factor 2 away: the rule works in single precision) -- so the kept blocks hold all
    their products and the dense reference applies to them."""
    sizes, ksizes = O.make_block_sizes(4 * 41, SMALL), O.make_block_sizes(190, [1, 7, 1, 32])
    A0 = general(sizes, ksizes, 0.5, 41, 14)
    scale = np.where(np.isin(np.arange(len(sizes)), (2, 6, 9)), 1e-4, 1.0)
    nze = A0.row_sizes[A0.rows()].astype(np.int64) * A0.col_sizes[A0.col_i]
    A = O.Bcsr(A0.row_sizes, A0.col_sizes, A0.row_p, A0.col_i, A0.blk_p, A0.data * np.repeat(scale[A0.rows()], nze))
    alpha = -0.5
    Ad = dense(A)
    R, bound = alpha * (Ad @ Ad.conj().T), abs(alpha) * (np.abs(Ad) @ np.abs(Ad).T)
    unfiltered, _ = O.multiply("N", "T", 1.0, part(A, A.data.real), part(A, A.data.real), 0.0, part(empty(sizes), np.zeros(0)), c_symmetry="S")
    off, rows = offsets(sizes), unfiltered.rows()
    norms = np.asarray([np.linalg.norm(R[off[r]:off[r + 1], off[c]:off[c + 1]]) for r, c in zip(rows, unfiltered.col_i)])
    s = np.sort(norms)
    lo, hi = len(s) // 4, 3 * len(s) // 4
    g = lo + int(np.argmax(s[lo + 1:hi + 1] / s[lo:hi]))
    eps = float(np.sqrt(s[g] * s[g + 1]))
    assert s[g + 1] / s[g] - 1.0 >= 1e-6
    keep = norms >= eps
    assert 0 < np.count_nonzero(keep) < len(keep)
    # the on-the-fly rule leaves the kept blocks' products alone
    koff, arows = offsets(ksizes), A.rows()
    anorm = {(int(r), int(k)): np.linalg.norm(Ad[off[r]:off[r + 1], koff[k]:koff[k + 1]]) for r, k in zip(arows, A.col_i)}
    row_blocks = np.diff(A.row_p)
    for r, c in zip(rows[keep], unfiltered.col_i[keep]):
        for i, j in ((int(r), int(c)), (int(c), int(r))):   # whichever of the pair is computed
            ks = [k for k in range(len(ksizes)) if (i, k) in anorm and (j, k) in anorm]
            assert all(anorm[(i, k)] * abs(alpha) * anorm[(j, k)] >= 2.0 * eps / max(1, int(row_blocks[i])) for k in ks)
    dC = dev(empty(sizes), "H")
    dbcsr_multiply("N", "C", alpha, dev(A), dev(A), 0.0, dC, filter_eps=eps, engine=eng)
    torch.cuda.synchronize()
    got = dev_to_bcsr(dC)
    assert np.array_equal(got.rows(), rows[keep]) and np.array_equal(got.col_i, unfiltered.col_i[keep])
    within_bar(got, R, bound)


# ---- 8. the C ABI -----------------------------------------------------------------------------------------------------------------------------------------
def fetch_matrix(lib, out, like):
    row_p = fetch(lib, out.row_p, out.nblkrows + 1, np.int32)
    nblks = int(out.nblks)
    assert row_p[-1] == nblks
    col_i, blk_p = fetch(lib, out.col_i, nblks, np.int32), fetch(lib, out.blk_p, nblks, np.int64)
    rows = np.repeat(np.arange(out.nblkrows), np.diff(row_p))
    nze = int((like.row_sizes[rows].astype(np.int64) * like.col_sizes[col_i]).sum())
    data = fetch(lib, out.data, nze, np.complex128)
    assert lib.dbcsr_amd_bcsr_release(C.byref(out)) == 0
    return O.Bcsr(like.row_sizes, like.col_sizes, row_p, col_i, blk_p, data)


def test_native_desymmetrized(mats):
    E = MultiplyEngine()
    M = mats["mixed"]
    dM = to_dev(M)
    src, out = dM.desc(), L.BcsrDesc()
    assert E.L.dbcsr_amd_bcsr_desymmetrized(E.h, L.dbcsr_type_complex_8, C.byref(src), 4, C.byref(out), None) == -1
    assert E.L.dbcsr_amd_bcsr_desymmetrized(E.h, L.dbcsr_type_complex_8, C.byref(src), 2, C.byref(out), None) == 0
    same_bits(fetch_matrix(E.L, out, M), expected_full(M, "H"))
    # kind 4 is refused by the twin entry too (the destination is never touched)
    assert E.L.dbcsr_amd_bcsr_twin_apply(E.h, L.dbcsr_type_complex_8, C.byref(src), 0, 4, C.byref(src), StreamHandle().ptr) == -1


@pytest.mark.parametrize("klimits", [(0, 0), (40, 150)])
def test_native_multiply_symmetric_c_z(product_case, klimits):
    E = MultiplyEngine()
    lib = E.L
    A, Cm = product_case["A"], product_case["C"]
    alpha, beta = -0.5, 2.0
    dA, dC = to_dev(A), to_dev(Cm)
    a, c = dA.desc(), dC.desc()
    z = lambda x: (C.c_double * 2)(complex(x).real, complex(x).imag)
    out, flop = L.BcsrDesc(), C.c_int64(0)
    args = lambda kind: (E.h, b"N", b"C", z(alpha), C.byref(a), C.byref(a), z(beta), C.byref(c), kind, klimits[0], klimits[1], 0, 0.0, C.byref(out),
                         C.byref(flop), None)
    assert lib.dbcsr_amd_multiply_symmetric_c_z(*args(4)) == -1
    assert lib.dbcsr_amd_multiply_symmetric_c_z(*args(2)) == 0
    torch.cuda.synchronize()
    got = fetch_matrix(lib, out, Cm)
    ra = part(A, A.data.real)
    ksl = slice(None)
    if klimits[0]:   # the window of k: blocks that intersect it take part (with their outside parts cleared), the dense reference is cut
        ra = O.crop(ra, None, (klimits[0] - 1, klimits[1] - 1))
        ksl = slice(klimits[0] - 1, klimits[1])
    ref, info = O.multiply("N", "T", 1.0, ra, ra, 1.0, part(Cm, Cm.data.real), c_symmetry="S")
    same_index(got, ref)
    assert flop.value == info["flop"]
    Ad, Cd = dense(A)[:, ksl], dense(expected_full(Cm, "H"))
    within_bar(got, beta * Cd + alpha * (Ad @ Ad.conj().T), abs(alpha) * (np.abs(Ad) @ np.abs(Ad).T) + abs(beta) * np.abs(Cd))
    # the entries with real scalars keep answering -10 for complex data
    assert lib.dbcsr_amd_multiply_symmetric_c(E.h, b"N", b"C", L.dbcsr_type_complex_8, alpha, C.byref(a), C.byref(a), beta, C.byref(c), 2, 0, 0.0,
                                              C.byref(out), C.byref(flop), None) == -10


# ---- 9. refusals that remain --------------------------------------------------------------------------------------------------------------------------------
def test_refusals_that_remain(eng, operand_case):
    oc = operand_case
    with pytest.raises(NotImplementedError):   # complex 'S' / 'A': the C ABI can do them, the mirror does not offer them yet
        dbcsr_multiply("N", "N", 1.0, dev(oc["T1"], "S"), dev(oc["G2"]), 1.0, dev(oc["C"]), engine=eng)
    with pytest.raises(NotImplementedError):
        eng.desymmetrized(dev(oc["T1"], "A"))
    realm = lambda M: part(M, M.data.real)
    with pytest.raises(ValueError):            # real 'H'
        dbcsr_multiply("N", "N", 1.0, dev(realm(oc["T1"]), "H"), dev(realm(oc["G2"])), 1.0, dev(realm(oc["C"])), engine=eng)
    with pytest.raises(ValueError):
        eng.desymmetrized(dev(realm(oc["T1"]), "K"))
    with pytest.raises(NotImplementedError):   # row limits with a product with symmetry
        dbcsr_multiply("N", "C", 1.0, dev(oc["G1"]), dev(oc["G1"]), 1.0, dev(oc["T2"], "H"), first_row=2, last_row=50, engine=eng)
