"""The in-place block filter: dbcsr_amd_bcsr_filter_apply_index compacts C's index and leaves its data area alone
(MultiplyEngine.filtered(..., in_place=True), MultiplyEngine.filter_in_place, dbcsr_amd_mm_set_filter_in_place).  What it returns is
an UNPACKED matrix: same row_p / col_i as the copying filter, every kept block bit-identical and where the product kernel put it.

Inputs: the oracle's perf_case with the block magnitudes spread over two and a half decades (seed 5, 10 ** uniform(-2, 0.5) per
block, as tests/test_gpu_multiply.py::test_filter_eps_matches_oracle), five structures that reach different product-kernel families.
For the stand-alone filter eps is the midpoint between two neighbouring block norms of the ORACLE's unfiltered product at the 10 %,
50 % and 90 % positions, so that no norm sits on the threshold."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from dbcsr_amd import lib as L
from dbcsr_amd.matrix import DbcsrMatrix, StreamHandle
from dbcsr_amd.multiply import MultiplyEngine, dbcsr_multiply
from oracle import oracle as O
from tests.gpu_util import dev_to_bcsr, rel_err, to_dev
from tests.test_gpu_multiply import TOL

pytestmark = pytest.mark.gpu

CASES = {
    "mixed": (300, 280, 290, .5, .5, .6, [1, 13, 1, 23], [1, 23, 1, 5], [1, 13, 1, 7]),
    "23_with_tails": (283, 258, 302, .5, .5, .6, [1, 23], [1, 23], [1, 23]),
    "small": (200, 210, 190, .5, .5, .6, [1, 5, 1, 8], [1, 7], [1, 6, 1, 8]),
    "slab": (288, 252, 324, .4, .4, .5, [1, 36], [1, 36], [1, 36]),
    "long_rows": (200, 1000, 300, .5, .5, .9, [1, 5], [1, 5], [1, 5]),
}
QUANTILES = (0.1, 0.5, 0.9)


def spread(mats, seed=5):
    rng = np.random.default_rng(seed)
    for M in mats:
        rows = M.rows()
        for b in range(M.nblks):
            ne = int(M.row_sizes[rows[b]]) * int(M.col_sizes[M.col_i[b]])
            M.data[M.blk_p[b]:M.blk_p[b] + ne] *= 10.0 ** rng.uniform(-2, 0.5)
    return mats


@functools.lru_cache(maxsize=None)
def inputs(case):
    return spread(O.perf_case(*CASES[case]))


@functools.lru_cache(maxsize=None)
def oracle_product(case):
    A, B, Cm = inputs(case)
    return O.multiply("N", "N", 1.0, A, B, 1.0, Cm)[0]


def block_sizes(M):
    return M.row_sizes[M.rows()].astype(np.int64) * M.col_sizes[M.col_i]


def block_sq_norms(M):
    """sum of squares per block, float64"""
    sq = np.asarray(M.data, np.float64) ** 2
    return np.array([sq[p:p + n].sum() for p, n in zip(M.blk_p, block_sizes(M))])


def gathered(M):
    """the blocks of M in index order, one after the other: what a packed copy of M holds"""
    if M.nblks == 0:
        return M.data[:0]
    return np.concatenate([M.data[p:p + n] for p, n in zip(M.blk_p, block_sizes(M))])


def same_bits(x, y):
    return x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


def quantile_eps(case, q):
    """midpoint between the two neighbouring block norms of the oracle's unfiltered product at position q; asserts the two
    conditions that make the case mean something"""
    s = np.sort(np.sqrt(block_sq_norms(oracle_product(case))))
    i = int(round(q * len(s)))
    eps = 0.5 * (s[i - 1] + s[i])
    below = float(np.count_nonzero(s < eps)) / len(s)
    assert 0.05 <= below <= 0.95, (case, q, below)
    assert np.all(np.abs(s - eps) > 1e-6 * eps), (case, q, "a block norm sits on the threshold")
    return float(eps)


def cast(M, dtype):
    return O.Bcsr(M.row_sizes, M.col_sizes, M.row_p, M.col_i, M.blk_p, M.data.astype(dtype))


def alias(M):
    """another DbcsrMatrix over the same tensors (dbcsr_multiply re-points its matrix_c)"""
    return DbcsrMatrix(M.row_blk_size, M.col_blk_size, M.row_p, M.col_i, M.blk_p, M.data, M.name, symmetry=M.symmetry, nze=M.nze)


def check_unpacked_pair(X, Y, P=None):
    """X: in-place result, Y: copying result of the same filter.  Returns their host forms."""
    hx, hy = dev_to_bcsr(X), dev_to_bcsr(Y)
    assert np.array_equal(hx.row_p, hy.row_p) and np.array_equal(hx.col_i, hy.col_i)
    assert same_bits(gathered(hx), hy.data), "a kept block differs between the two forms"
    assert X.nze == Y.data.numel() == Y.nze
    assert np.all(np.diff(hx.blk_p) > 0), "blk_p of the in-place result is not strictly increasing"
    if P is not None:
        assert X.data is P.data and X.data.data_ptr() == P.data.data_ptr()
    return hx, hy


# ---- 1. stand-alone filter, both forms ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("q", QUANTILES + (None,), ids=["q10", "q50", "q90", "nothing"])
@pytest.mark.parametrize("case", list(CASES))
def test_standalone_filter_both_forms(case, q, dtype):
    A, B, Cm = inputs(case)
    eps = 1e-30 if q is None else quantile_eps(case, q)
    eng = MultiplyEngine()
    dA, dB, P = to_dev(cast(A, dtype)), to_dev(cast(B, dtype)), to_dev(cast(Cm, dtype))
    dbcsr_multiply("N", "N", 1.0, dA, dB, 1.0, P, engine=eng)
    torch.cuda.synchronize()
    hp = dev_to_bcsr(P)
    assert hp.nblks == oracle_product(case).nblks
    Y = eng.filtered(P, eps)
    X = eng.filtered(P, eps, in_place=True)
    torch.cuda.synchronize()
    if q is None:
        assert X is P and Y is P and P.packed
        return
    keep = ~(block_sq_norms(hp) < eps * eps)      # the expected pattern, from the downloaded product itself
    assert 0 < np.count_nonzero(keep) < hp.nblks
    hx, hy = check_unpacked_pair(X, Y, P)
    want_row_p = np.concatenate([[0], np.cumsum(np.bincount(hp.rows()[keep], minlength=hp.nbr))])
    assert np.array_equal(hx.row_p, want_row_p) and np.array_equal(hx.col_i, hp.col_i[keep])
    assert np.array_equal(hx.blk_p, hp.blk_p[keep]), "a kept block moved"
    assert same_bits(hx.data, hp.data), "the in-place filter touched the data area"
    assert same_bits(hy.data, gathered(O.Bcsr(hp.row_sizes, hp.col_sizes, want_row_p, hp.col_i[keep], hp.blk_p[keep], hp.data)))
    assert X.nze == int(block_sizes(hp)[keep].sum())
    assert not X.packed and Y.packed


# ---- 2. the whole filtered multiply against the oracle -----------------------------------------------------------------------
@pytest.mark.parametrize("announce", [True, False], ids=["announced", "unannounced"])
@pytest.mark.parametrize("eps,alpha", [(2.0, 1.0), (2.0, 0.5), (40.0, 1.0), (40.0, 0.5)])
@pytest.mark.parametrize("case", list(CASES))
def test_filtered_multiply_in_place_matches_oracle(case, eps, alpha, announce, monkeypatch):
    if announce:
        monkeypatch.delenv("DBCSR_AMD_MM_EXPECT_FILTER", raising=False)
    else:
        monkeypatch.setenv("DBCSR_AMD_MM_EXPECT_FILTER", "0")
    A, B, Cm = inputs(case)
    ref, info = O.multiply("N", "N", alpha, A, B, 1.0, Cm, filter_eps=eps)
    res = {}
    for on in (True, False):
        eng = MultiplyEngine()
        assert eng.filter_in_place is False
        eng.filter_in_place = on
        dA, dB, dC = to_dev(A), to_dev(B), to_dev(Cm)
        flop = [0]
        dbcsr_multiply("N", "N", alpha, dA, dB, 1.0, dC, filter_eps=eps, flop=flop, engine=eng)
        torch.cuda.synchronize()
        assert flop[0] == info["flop"]
        res[on] = dC
    X, Y = res[True], res[False]
    hx, hy = check_unpacked_pair(X, Y)
    assert np.array_equal(hx.row_p, ref.row_p) and np.array_equal(hx.col_i, ref.col_i)
    assert np.array_equal(hy.blk_p, ref.blk_p)
    assert rel_err(gathered(hx), ref.data) <= TOL
    assert X.packed == (hx.data.size == ref.data.size)


# ---- 3. consumers of an unpacked matrix --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def xy():
    """X: in-place, Y: copying result of one filtered multiply that drops blocks (mixed sizes, eps = 40)"""
    A, B, Cm = inputs("mixed")
    out = {}
    for on in (True, False):
        eng = MultiplyEngine()
        eng.filter_in_place = on
        dC = to_dev(Cm)
        dbcsr_multiply("N", "N", 1.0, to_dev(A), to_dev(B), 1.0, dC, filter_eps=40.0, engine=eng)
        out[on] = dC
    torch.cuda.synchronize()
    X, Y = out[True], out[False]
    assert not X.packed and Y.packed and X.nblks == Y.nblks > 0 and X.nze < X.data.numel()
    return X, Y


def same_matrix(G, H):
    g, h = dev_to_bcsr(G), dev_to_bcsr(H)
    assert np.array_equal(g.row_p, h.row_p) and np.array_equal(g.col_i, h.col_i) and np.array_equal(g.blk_p, h.blk_p)
    assert same_bits(g.data, h.data)


@pytest.mark.parametrize("role", ["A", "B", "C_in"])
def test_unpacked_matrix_as_operand(xy, role):
    X, Y = xy
    m, n, k, sa, sb, sc, bm, bn, bk = CASES["mixed"]
    if role == "A":      # X is m x n: times an n x 200 matrix
        _, B2, C2 = O.perf_case(m, 200, n, sa, sb, sc, bm, [1, 7], bn)
        run = lambda Z, E: (alias(Z), to_dev(B2), to_dev(C2), 1.0)
    elif role == "B":    # a 200 x m matrix times X
        A3, _, C3 = O.perf_case(200, n, m, sa, sb, sc, [1, 7], bn, bm)
        run = lambda Z, E: (to_dev(A3), alias(Z), to_dev(C3), 1.0)
    else:
        A, B, _ = inputs("mixed")
        run = lambda Z, E: (to_dev(A), to_dev(B), alias(Z), 2.0)
    outs = []
    for Z in (X, Y):
        E = MultiplyEngine()
        a, b, c, beta = run(Z, E)
        dbcsr_multiply("N", "N", 1.0, a, b, beta, c, engine=E)
        torch.cuda.synchronize()
        assert c.packed and c.nblks > 0
        outs.append(c)
    same_matrix(outs[0], outs[1])
    # the operand itself is as it was
    check_unpacked_pair(X, Y)


def test_unpacked_matrix_transposed_cropped_checksum(xy):
    X, Y = xy
    E = MultiplyEngine()
    tx, ty = E.transposed(X), E.transposed(Y)
    assert tx.data.numel() == X.nze and tx.packed
    same_matrix(tx, ty)
    m, n = CASES["mixed"][0], CASES["mixed"][1]
    win = ((m // 5, 3 * m // 4), (n // 6, 2 * n // 3))
    same_matrix(E.cropped(X, *win), E.cropped(Y, *win))
    assert E.checksum(X) == E.checksum(Y)
    # the unbounded crop is the packing copy: all four arrays of the copying filter's result
    packed = E.cropped(X)
    assert packed.packed
    same_matrix(packed, Y)
    sx, sy = E.scaled_window(X, 3.0, *win), E.scaled_window(Y, 3.0, *win)
    assert sx.nze == X.nze and not sx.packed
    same_matrix(E.cropped(sx), sy)


def test_symmetric_product_with_the_filter_in_place():
    A, _, _ = O.perf_case(300, 300, 290, .5, .5, .6, [1, 13, 1, 23], [1, 13, 1, 23], [1, 13, 1, 7])
    (A,) = spread([A])
    outs = {}
    for key, on, eps in (("in_place", True, 40.0), ("copy", False, 40.0), ("unfiltered", False, None)):
        E = MultiplyEngine()
        E.filter_in_place = on
        dA = to_dev(A)
        sym = DbcsrMatrix.empty_like_pattern(dA.row_blk_size, dA.row_blk_size, torch.float64, device=dA.data.device)
        sym.symmetry = "S"
        dbcsr_multiply("N", "T", 1.0, dA, dA, 0.0, sym, filter_eps=eps, engine=E)
        torch.cuda.synchronize()
        outs[key] = sym
    assert 0 < outs["copy"].nblks < outs["unfiltered"].nblks
    same_matrix(outs["in_place"], outs["copy"])
    Ce = O.Bcsr(A.row_sizes, A.row_sizes, np.zeros(A.nbr + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros(0))
    ref, _ = O.multiply("N", "T", 1.0, A, A, 0.0, Ce, filter_eps=40.0, c_symmetry="S")
    got = dev_to_bcsr(outs["in_place"])
    assert np.array_equal(got.row_p, ref.row_p) and np.array_equal(got.col_i, ref.col_i)
    assert rel_err(got.data, ref.data) <= TOL


# ---- 4. guards ---------------------------------------------------------------------------------------------------------------
def test_accumulate_into_an_unpacked_matrix_is_refused(xy):
    X, Y = xy
    A, B, _ = inputs("mixed")
    E = MultiplyEngine()
    with pytest.raises(ValueError, match="not packed"):
        E.accumulate(1.0, to_dev(A), to_dev(B), X)
    E.accumulate(1.0, to_dev(A), to_dev(B), Y.copy())   # (a packed one is taken)
    torch.cuda.synchronize()


def test_smaller_eps_than_announced_is_refused_in_both_forms(monkeypatch):
    monkeypatch.delenv("DBCSR_AMD_MM_EXPECT_FILTER", raising=False)
    case = (23 * 40 + 16, 23 * 38 + 9, 23 * 30 + 5, 0.8, 0.8, 0.97, [1, 23], [1, 23], [1, 23])   # sparse C_in: most C blocks are new
    A, B, Cm = O.perf_case(*case)
    eps = 200.0
    ref, _ = O.multiply("N", "N", 1.0, A, B, 1.0, Cm, filter_eps=eps)
    eng = MultiplyEngine()
    lib = eng.L
    dA, dB, dC = to_dev(A), to_dev(B), to_dev(Cm)
    sth = StreamHandle(None)
    a, b, cin = dA.desc(), dB.desc(), dC.desc()
    row_p = torch.empty(dC.nblkrows + 1, dtype=torch.int32, device="cuda")
    counts = L.MmCounts()
    assert lib.dbcsr_amd_mm_symbolic_filtered(eng.h, dA.dtype_code, 1.0, eps, C.byref(a), C.byref(b), C.byref(cin), 0, row_p.data_ptr(),
                                              C.byref(counts), sth.ptr) == 0
    out = DbcsrMatrix(dC.row_blk_size, dC.col_blk_size, row_p, torch.empty(counts.c_nblks, dtype=torch.int32, device="cuda"),
                      torch.empty(counts.c_nblks, dtype=torch.int64, device="cuda"),
                      torch.empty(counts.c_nze, dtype=torch.float64, device="cuda"), "C")
    cout = out.desc(out=True)
    assert lib.dbcsr_amd_mm_expect_filter(eng.h, eps) == 0
    assert lib.dbcsr_amd_mm_numeric(eng.h, dA.dtype_code, 1.0, C.byref(a), C.byref(b), 1.0, C.byref(cin), C.byref(cout), sth.ptr) == 0
    with pytest.raises(RuntimeError, match=r"filter_count failed \(-3\)"):
        eng.filtered(out, 0.5 * eps, in_place=True)
    with pytest.raises(RuntimeError, match=r"filter_count failed \(-3\)"):
        eng.filtered(out, 0.5 * eps)
    # the announced eps itself is served, and the index that comes back names no block the product kernel left unwritten
    X = eng.filtered(out, eps, in_place=True)
    torch.cuda.synchronize()
    hx = dev_to_bcsr(X)
    assert X.data is out.data and not X.packed
    assert np.array_equal(hx.row_p, ref.row_p) and np.array_equal(hx.col_i, ref.col_i)
    assert rel_err(gathered(hx), ref.data) <= TOL


def test_apply_index_argument_checks():
    A, B, Cm = inputs("small")
    eng = MultiplyEngine()
    lib = eng.L
    P = to_dev(Cm)
    dbcsr_multiply("N", "N", 1.0, to_dev(A), to_dev(B), 1.0, P, engine=eng)
    eps = quantile_eps("small", 0.5)
    sth = StreamHandle(None)
    src = P.desc()
    row_p = torch.empty(P.nblkrows + 1, dtype=torch.int32, device="cuda")
    nb, nz = C.c_int64(), C.c_int64()

    def dest(data):
        return DbcsrMatrix(P.row_blk_size, P.col_blk_size, row_p, torch.full((nb.value,), -7, dtype=torch.int32, device="cuda"),
                           torch.full((nb.value,), -7, dtype=torch.int64, device="cuda"), data, "X", nze=nz.value)

    # no count on this handle yet
    fresh = MultiplyEngine()
    nb.value = P.nblks
    d0 = dest(P.data).desc(out=True)
    assert lib.dbcsr_amd_bcsr_filter_apply_index(fresh.h, C.byref(src), C.byref(d0), sth.ptr) == -1
    assert lib.dbcsr_amd_bcsr_filter_count(eng.h, P.dtype_code, C.byref(src), eps, row_p.data_ptr(), C.byref(nb), C.byref(nz), sth.ptr) == 0
    assert 0 < nb.value < P.nblks
    # dst->data is not src->data
    other = dest(torch.empty_like(P.data))
    d1 = other.desc(out=True)
    assert lib.dbcsr_amd_bcsr_filter_apply_index(eng.h, C.byref(src), C.byref(d1), sth.ptr) == -1
    # a src whose nblks is not the counted one
    good = dest(P.data)
    d2 = good.desc(out=True)
    short = P.desc()
    short.nblks = P.nblks - 1
    assert lib.dbcsr_amd_bcsr_filter_apply_index(eng.h, C.byref(short), C.byref(d2), sth.ptr) == -1
    assert lib.dbcsr_amd_bcsr_filter_apply_index(eng.h, None, C.byref(d2), sth.ptr) == -1
    torch.cuda.synchronize()
    assert int(other.col_i.max()) == -7 and int(good.col_i.max()) == -7, "a refused call wrote its destination"
    # ... and the count is still good for the right call
    assert lib.dbcsr_amd_bcsr_filter_apply_index(eng.h, C.byref(src), C.byref(d2), sth.ptr) == 0
    torch.cuda.synchronize()
    Y = eng.filtered(P, eps)
    check_unpacked_pair(good, Y, P)


# ---- 5. the one-call C path --------------------------------------------------------------------------------------------------
def fetch(lib, ptr, count, dtype):
    out = np.empty(count, dtype)
    if count:
        assert lib.c_dbcsr_acc_memcpy_d2h(C.c_void_p(ptr), out.ctypes.data_as(C.c_void_p), C.c_size_t(out.nbytes), None) == 0
        assert lib.c_dbcsr_acc_device_synchronize() == 0
    return out


def native(E, A, B, Cm, transb="N", beta=1.0, eps=0.0, alpha=1.0, symmetric=False):
    """dbcsr_amd_multiply / dbcsr_amd_multiply_symmetric_c on E's handle; the result on the host (data: up to the last block's end)"""
    lib = E.L
    dA, dB, dC = to_dev(A), to_dev(B), to_dev(Cm)
    a, b, c = dA.desc(), dB.desc(), dC.desc()
    out = L.BcsrDesc()
    flop = C.c_int64(0)
    if symmetric:
        rc = lib.dbcsr_amd_multiply_symmetric_c(E.h, b"N", transb.encode(), L.dbcsr_type_real_8, float(alpha), C.byref(a), C.byref(b), float(beta),
                                                C.byref(c), 0, 0, float(eps), C.byref(out), C.byref(flop), None)
    else:
        rc = lib.dbcsr_amd_multiply(E.h, b"N", transb.encode(), L.dbcsr_type_real_8, float(alpha), C.byref(a), C.byref(b), float(beta), C.byref(c),
                                    None, 0, float(eps), C.byref(out), C.byref(flop), None)
    assert rc == 0
    torch.cuda.synchronize()
    nbr, nblks = out.nblkrows, int(out.nblks)
    row_p = fetch(lib, out.row_p, nbr + 1, np.int32)
    assert row_p[-1] == nblks
    col_i, blk_p = fetch(lib, out.col_i, nblks, np.int32), fetch(lib, out.blk_p, nblks, np.int64)
    rows = np.repeat(np.arange(nbr), np.diff(row_p))
    sizes = Cm.row_sizes[rows].astype(np.int64) * Cm.col_sizes[col_i]
    data = fetch(lib, out.data, int((blk_p + sizes).max()) if nblks else 0, np.float64)
    assert lib.dbcsr_amd_bcsr_release(C.byref(out)) == 0
    assert not out.row_p and not out.col_i and not out.blk_p and not out.data
    return O.Bcsr(Cm.row_sizes, Cm.col_sizes, row_p, col_i, blk_p, data), flop.value


@pytest.mark.parametrize("announce", [True, False], ids=["announced", "unannounced"])
@pytest.mark.parametrize("eps,alpha", [(2.0, 1.0), (40.0, 0.5)])
@pytest.mark.parametrize("case", ["mixed", "23_with_tails", "long_rows"])
def test_native_multiply_with_the_filter_in_place(case, eps, alpha, announce, monkeypatch):
    if announce:
        monkeypatch.delenv("DBCSR_AMD_MM_EXPECT_FILTER", raising=False)
    else:
        monkeypatch.setenv("DBCSR_AMD_MM_EXPECT_FILTER", "0")
    A, B, Cm = inputs(case)
    ref, info = O.multiply("N", "N", alpha, A, B, 1.0, Cm, filter_eps=eps)
    plain, plain_info = O.multiply("N", "N", alpha, A, B, 1.0, Cm)
    E = MultiplyEngine()
    E.set_filter_in_place(True)
    assert E.filter_in_place is True
    hx, flop = native(E, A, B, Cm, eps=eps, alpha=alpha)
    assert flop == info["flop"]
    assert np.array_equal(hx.row_p, ref.row_p) and np.array_equal(hx.col_i, ref.col_i)
    assert np.all(np.diff(hx.blk_p) > 0)
    assert rel_err(gathered(hx), ref.data) <= TOL
    if ref.nblks < plain.nblks and eps >= 40.0:
        assert hx.data.size > ref.data.size or hx.blk_p[0] > 0, "blocks were dropped and the result is packed: the copying form ran"
    # the handle after the release: an unfiltered multiply, then the copying form again -- same bits as the in-place result
    hp, flop = native(E, A, B, Cm, alpha=alpha)
    assert flop == plain_info["flop"]
    assert np.array_equal(hp.row_p, plain.row_p) and np.array_equal(hp.col_i, plain.col_i) and np.array_equal(hp.blk_p, plain.blk_p)
    assert rel_err(hp.data, plain.data) <= TOL
    E.set_filter_in_place(False)
    hy, _ = native(E, A, B, Cm, eps=eps, alpha=alpha)
    assert np.array_equal(hy.row_p, hx.row_p) and np.array_equal(hy.col_i, hx.col_i) and np.array_equal(hy.blk_p, ref.blk_p)
    assert same_bits(gathered(hx), hy.data)


def test_native_symmetric_multiply_with_the_filter_in_place():
    A, _, _ = O.perf_case(300, 300, 290, .5, .5, .6, [1, 13, 1, 23], [1, 13, 1, 23], [1, 13, 1, 7])
    (A,) = spread([A])
    Ce = O.Bcsr(A.row_sizes, A.row_sizes, np.zeros(A.nbr + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros(0))
    eps = 40.0
    ref, info = O.multiply("N", "T", 1.0, A, A, 0.0, Ce, filter_eps=eps, c_symmetry="S")
    full, _ = O.multiply("N", "T", 1.0, A, A, 0.0, Ce, c_symmetry="S")
    assert 0 < ref.nblks < full.nblks
    E = MultiplyEngine()
    E.set_filter_in_place(True)
    hx, flop = native(E, A, A, Ce, transb="T", beta=0.0, eps=eps, symmetric=True)
    E.set_filter_in_place(False)
    hy, flop_y = native(E, A, A, Ce, transb="T", beta=0.0, eps=eps, symmetric=True)
    assert flop == flop_y == info["flop"]
    for h in (hx, hy):   # (the way back to the stored triangle is a copy: packed either way)
        assert np.array_equal(h.row_p, ref.row_p) and np.array_equal(h.col_i, ref.col_i) and np.array_equal(h.blk_p, ref.blk_p)
        assert rel_err(h.data, ref.data) <= TOL
    assert same_bits(hx.data, hy.data)


# ---- 6. memory ---------------------------------------------------------------------------------------------------------------
def test_in_place_filter_allocates_no_second_data_area():
    from dbcsr_amd.randmat import perf_matrices
    E = MultiplyEngine()
    A, B, Cm = perf_matrices(6144, 6144, 6144, (0.9, 0.9, 0.9), [1, 23], [1, 23], [1, 23], dtype=torch.float64, engine=E)
    P, _ = E.multiply_local(1.0, A, B, 1.0, Cm)
    torch.cuda.synchronize()
    assert P.packed and P.data.numel() * P.data.element_size() >= 128 * 2 ** 20
    # eps: the median of P's block norms (P is packed: a block's sum of squares is a difference of the running sum)
    rows = torch.repeat_interleave(torch.arange(P.nblkrows, device=P.data.device), torch.diff(P.row_p.to(torch.int64)))
    sizes = P.row_blk_size.to(torch.int64)[rows] * P.col_blk_size.to(torch.int64)[P.col_i.to(torch.int64)]
    run = torch.cat([torch.zeros(1, dtype=torch.float64, device=P.data.device), torch.cumsum(P.data * P.data, 0)])
    eps = float(torch.sqrt(torch.median(run[P.blk_p + sizes] - run[P.blk_p])))
    del run, rows, sizes
    E.filtered(P, eps)   # (the engine's own work areas exist from here on)
    torch.cuda.synchronize()
    peak = {}
    for in_place in (True, False):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        R = E.filtered(P, eps, in_place=in_place)
        torch.cuda.synchronize()
        peak[in_place] = torch.cuda.max_memory_allocated() - before
        nze, nblks = R.nze, R.nblks
        assert 0.3 * P.nblks < nblks < 0.7 * P.nblks
        assert (R.data is P.data) == in_place
        peak["nze", in_place] = nze
        del R
    assert peak["nze", True] == peak["nze", False]
    saved = peak[False] - peak[True]
    print("filtered(): peak above the product %d B copying, %d B in place; new_nze * 8 = %d B" % (peak[False], peak[True], 8 * peak["nze", True]))
    assert saved >= 8 * peak["nze", True]
