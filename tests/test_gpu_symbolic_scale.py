"""The symbolic phase at scale on the device: every case of tests/symbolic_scale.py (4267 block rows and columns of 1 ... 3 elements, five million C blocks,
several column panels, the (m, n) classes with panels, both sides of nbr = 2048, empty block rows) on a fresh MultiplyEngine through the dbcsr_multiply
mirror, a third of them through the C entry as well.

 * last_symbolic() is the line mm_choose.h predicts for the oracle's counts (tests/test_symbolic_scale_cpu.py shows that it is the path the case is there
   for), last_kernel() the family it predicts;
 * index (row_p, col_i, blk_p), flop and the product count are the oracle's, every element is within 2 gamma (|alpha| (|A| |B|) + |beta| |C_in|) of the
   oracle's (the bar is derived in tests/symbolic_scale.py);
 * the same case under DBCSR_AMD_MM_SYMBOLIC=word / grid / rows and with DBCSR_AMD_MM_PANEL_MB unset / 1 gives the same BITS, index and data: the product
   lists are the same lists whichever kernels made them (mm_symbolic.h: count_products_rows), and the launch order changes no result (order_fill).  The
   numeric family reads none of these switches, so it never changes with the variant (asserted), and no case needs the bar instead;
 * a second multiply of the same operands reports plan=hit and the same bits (a filtered multiply, and one whose operand the mirror transposes on the same
   engine, never reuse a plan: plan=miss, the same bits);
 * the operations that share the bitmaps, row_prefix and exclusive_scan -- the stand-alone transpose, crop with limits inside a block, the copying and the
   in-place filter, dbcsr_add on a union pattern, desymmetrize, dbcsr_get_block_diag -- on matrices of 4267 block rows and 134 bitmap words, bit for bit
   against numpy on the host."""
import time

import numpy as np
import pytest
import torch

from dbcsr_amd.multiply import MultiplyEngine, dbcsr_multiply
from dbcsr_amd.operations import dbcsr_add, dbcsr_get_block_diag
from oracle import oracle as O
from tests import option_sweep as OS
from tests import symbolic_scale as S
from tests.gpu_util import dev_to_bcsr, native_multiply_any, to_dev
from tests.test_numeric_choice import choose, shims  # noqa: F401
from tests.test_symbolic_scale_cpu import class_mode, shim  # noqa: F401

pytestmark = pytest.mark.gpu

SWITCHES = ("DBCSR_AMD_MM_CLASSES", "DBCSR_AMD_MM_SYMBOLIC", "DBCSR_AMD_MM_PANEL_MB", "DBCSR_AMD_MM_WG_WAVES", "DBCSR_AMD_MM_HOT", "DBCSR_AMD_MM_KCHUNKS",
            "DBCSR_AMD_MM_PLAN", "DBCSR_AMD_LAB")
LINES = {}   # case -> last_symbolic() of its own run (the last test prints them: profiles/symbolic_scale.txt)


def engine_with(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return MultiplyEngine()   # a fresh engine: it reads the switches when it is made


def through_the_mirror(case, eng):
    A, B, Cm = S.operands(case)
    dA, dB, dC = to_dev(A), to_dev(B), to_dev(Cm)
    flop = [0]
    counts = dbcsr_multiply(case["ta"], case["tb"], case["alpha"], dA, dB, case["beta"], dC, retain_sparsity=case["retain"], filter_eps=case["eps"] or None,
                            flop=flop, engine=eng)
    torch.cuda.synchronize()
    return dev_to_bcsr(dC), flop[0], int(counts.nproducts)


def bits(M):
    return tuple(np.ascontiguousarray(x).tobytes() for x in (M.row_p, M.col_i, M.blk_p, M.data))


def variants_of(case):
    """the case's switches with each symbolic kernel set forced, and with the panel size the other way round (1 MB <-> the default)"""
    env = case["env"]
    out = [dict(env, DBCSR_AMD_MM_SYMBOLIC=mode) for mode in ("word", "grid", "rows")]
    if "DBCSR_AMD_MM_PANEL_MB" in env:
        out.append({k: v for k, v in env.items() if k != "DBCSR_AMD_MM_PANEL_MB"})
    else:
        out.append(dict(env, DBCSR_AMD_MM_PANEL_MB="1"))
    return out


@pytest.mark.parametrize("name", S.NAMES)
def test_case(name, monkeypatch, shim, shims):  # noqa: F811
    case = S.BY_NAME[name]
    t0 = time.perf_counter()
    cls = class_mode(shims, case)
    eng = engine_with(monkeypatch, case["env"])
    got, flop, nprod = through_the_mirror(case, eng)
    line, kernel = eng.last_symbolic(), eng.last_kernel()
    LINES[name] = line
    # the path
    assert line == S.line_of(S.predicted(case, shim, cls)), line
    fields = S.parse_line(line)
    assert all(fields[k] == v for k, v in case["expect"].items() if k != "claims"), (line, case["expect"])
    if case["dtype"] == S.Z64:
        assert OS.family(kernel) == "z64", kernel
    else:
        q, kw = S.choice_query(case)
        assert OS.family(kernel) == OS.family(choose(shims, case["env"], q, **kw)[0]), kernel
    # index, flop, product count: exact; values: element by element within the bar
    bad, worst = S.compare(case, got, flop, nprod)
    print("%s: %s; %s; err / bar %.3f" % (name, line, kernel, worst))
    assert bad is None, (bad, name)
    # the same operands again: the saved plan, the same bits (a filtered multiply saves no plan, and the mirror's transpose of an operand runs in the
    # engine's work areas, which ends the plan: those report plan=miss and still give the same bits)
    again, flop2, nprod2 = through_the_mirror(case, eng)
    reuses = case["eps"] == 0 and case["ta"] + case["tb"] == "NN"
    assert S.parse_line(eng.last_symbolic())["plan"] == ("hit" if reuses else "miss"), eng.last_symbolic()
    assert dict(fields, plan="") == dict(S.parse_line(eng.last_symbolic()), plan="")
    assert bits(again) == bits(got) and (flop2, nprod2) == (flop, nprod)
    # the symbolic variants: the same bits
    for env in variants_of(case):
        e = engine_with(monkeypatch, env)
        v, vflop, vprod = through_the_mirror(case, e)
        assert e.last_symbolic() == S.line_of(S.predicted(case, shim, cls, env=env)), (env, e.last_symbolic())
        assert OS.family(e.last_kernel()) == OS.family(kernel), (env, e.last_kernel(), kernel)
        assert (vflop, vprod) == (flop, nprod), env
        assert bits(v) == bits(got), "the result differs in its bits under %r (%s against %s)" % (env, e.last_symbolic(), line)
    print("%s: %.2f s" % (name, time.perf_counter() - t0))


@pytest.mark.parametrize("name", [c["name"] for c in S.CASES if c["native"]])
def test_case_through_the_c_entry(name, monkeypatch, shim, shims):  # noqa: F811
    case = S.BY_NAME[name]
    eng = engine_with(monkeypatch, case["env"])
    A, B, Cm = S.operands(case)
    got, flop = native_multiply_any(eng, case["ta"], case["tb"], case["alpha"], A, B, case["beta"], Cm, retain=case["retain"], eps=case["eps"])
    assert eng.last_symbolic() == S.line_of(S.predicted(case, shim, class_mode(shims, case))), eng.last_symbolic()
    bad, worst = S.compare(case, got, flop, None)
    print("%s (C entry): err / bar %.3f" % (name, worst))
    assert bad is None, (bad, name)


def test_panel_size_of_zero_runs_as_one_megabyte(monkeypatch, shim, shims):  # noqa: F811
    """DBCSR_AMD_MM_PANEL_MB=0 divided by zero on the host; now it is the smallest panel, 1 MB"""
    case = S.BY_NAME["panels_small-TN-f64-mb1"]
    eng = engine_with(monkeypatch, dict(case["env"], DBCSR_AMD_MM_PANEL_MB="0"))
    got, flop, nprod = through_the_mirror(case, eng)
    assert eng.last_symbolic() == S.line_of(S.predicted(case, shim, class_mode(shims, case))), eng.last_symbolic()
    assert S.compare(case, got, flop, nprod)[0] is None


# ---- the operations that share the bitmaps, row_prefix and exclusive_scan: 4267 block rows, 134 bitmap words ------------------------------------------------
def square_sizes():
    return O.make_block_sizes(6400, S.A12)


@pytest.fixture(scope="module")
def Y():
    """4267 x 4267 blocks of 1 ... 2 elements, one block in 200 stored (91 000 blocks, 21 per block row and column)"""
    sizes = square_sizes()
    M = O.make_random_matrix(sizes, sizes, 0.995, O.RANDMAT_SEED_INIT + 101)
    assert M.nbr > 4096 and (M.nbc + 31) // 32 > 64 and np.any(M.col_i == 2047) and np.any(M.col_i == 2048)
    return M


@pytest.fixture(scope="module")
def Z():
    sizes = square_sizes()
    return O.make_random_matrix(sizes, sizes, 0.995, O.RANDMAT_SEED_INIT + 102)


def block_sizes_of(M):
    return M.row_sizes[M.rows()].astype(np.int64) * M.col_sizes[M.col_i]


def elements(M, blocks=None):
    """the data positions of the given blocks (all of them), block after block"""
    size = block_sizes_of(M)
    blk_p = M.blk_p
    if blocks is not None:
        size, blk_p = size[blocks], M.blk_p[blocks]
    start = np.concatenate([[0], np.cumsum(size)])
    return np.repeat(blk_p, size) + (np.arange(int(start[-1])) - np.repeat(start[:-1], size)), start[:-1]


def same_bits(dev, ref, packed=True):
    got = dev_to_bcsr(dev)
    assert np.array_equal(got.row_p, ref.row_p) and np.array_equal(got.col_i, ref.col_i), "index"
    if packed:
        assert np.array_equal(got.blk_p, ref.blk_p), "blk_p"
        assert got.data[:ref.data.size].tobytes() == ref.data.tobytes(), "data"
    else:
        assert got.data[elements(got)[0]].tobytes() == ref.data[elements(ref)[0]].tobytes(), "data"


def test_transpose_at_scale(Y):
    eng = MultiplyEngine()
    same_bits(eng.transposed(to_dev(Y)), O.transposed(Y))


def test_crop_with_limits_inside_a_block_at_scale(Y):
    """rows 302 ... 4201 and columns 152 ... 6001 (0-based elements): every bound is the second element of a block of two, or the first"""
    eng = MultiplyEngine()
    off = np.concatenate([[0], np.cumsum(Y.row_sizes)])
    rb, cb = (3 * 100 + 2, 3 * 1400 + 1), (3 * 50 + 2, 3 * 2000 + 1)
    for lo, hi in (rb, cb):
        assert lo not in off and hi + 1 not in off   # inside a block
    assert np.searchsorted(off, cb[1]) > 2048
    same_bits(eng.cropped(to_dev(Y), rb, cb), O.crop(Y, rb, cb))


def filtered_on_the_host(M, eps):
    pos, _ = elements(M)
    n2 = np.add.reduceat(np.square(M.data[pos]), np.concatenate([[0], np.cumsum(block_sizes_of(M))[:-1]]))
    assert np.all(np.abs(n2 - eps * eps) > 1e-12), "a block norm at eps^2"
    keep = ~(n2 < eps * eps)
    cnt = np.bincount(M.rows()[keep], minlength=M.nbr)
    src, start = elements(M, keep)
    return keep, O.Bcsr(M.row_sizes, M.col_sizes, np.concatenate([[0], np.cumsum(cnt)]), M.col_i[keep], start, M.data[src])


def test_filters_at_scale(Y):
    eps = 0.6
    keep, ref = filtered_on_the_host(Y, eps)
    assert 0.2 < keep.mean() < 0.8
    eng = MultiplyEngine()
    same_bits(eng.filtered(to_dev(Y), eps), ref)
    dY = to_dev(Y)
    out = eng.filtered(dY, eps, in_place=True)
    assert out.data.data_ptr() == dY.data.data_ptr()
    got = dev_to_bcsr(out)
    assert np.array_equal(got.row_p, ref.row_p) and np.array_equal(got.col_i, ref.col_i) and np.array_equal(got.blk_p, Y.blk_p[keep])
    assert got.data.tobytes() == Y.data.tobytes()   # (the data area is left as it is)


def added_on_the_host(A, B, alpha, beta):
    ka, kb = A.rows().astype(np.int64) * A.nbc + A.col_i, B.rows().astype(np.int64) * B.nbc + B.col_i
    keys = np.union1d(ka, kb)
    rows, cols = keys // A.nbc, (keys % A.nbc).astype(np.int32)
    size = A.row_sizes[rows].astype(np.int64) * A.col_sizes[cols]
    blk_p = np.concatenate([[0], np.cumsum(size)[:-1]])
    data = np.zeros(int(size.sum()))
    for M, k, s in ((A, ka, alpha), (B, kb, beta)):
        src, _ = elements(M)
        at = np.searchsorted(keys, k)
        sz = block_sizes_of(M)
        st = np.concatenate([[0], np.cumsum(sz)])
        dst = np.repeat(blk_p[at], sz) + (np.arange(int(st[-1])) - np.repeat(st[:-1], sz))
        data[dst] += s * M.data[src]
    return O.Bcsr(A.row_sizes, A.col_sizes, np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=A.nbr))]), cols, blk_p, data)


def test_add_on_a_union_pattern_at_scale(Y, Z):
    """2 Y - Z: powers of two, so every element is rounded once however the device forms it"""
    ref = added_on_the_host(Y, Z, 2.0, -1.0)
    assert Y.nblks < ref.nblks < Y.nblks + Z.nblks   # (a union with an overlap)
    dY = to_dev(Y)
    assert dbcsr_add(dY, to_dev(Z), 2.0, -1.0, engine=MultiplyEngine()) is False
    torch.cuda.synchronize()
    same_bits(dY, ref)


def test_desymmetrize_at_scale(Y):
    """the upper triangle of Y as an 'S' matrix of 4267 block rows"""
    up = Y.rows() <= Y.col_i
    src, start = elements(Y, up)
    T = O.Bcsr(Y.row_sizes, Y.col_sizes, np.concatenate([[0], np.cumsum(np.bincount(Y.rows()[up], minlength=Y.nbr))]), Y.col_i[up], start, Y.data[src])
    dT = to_dev(T)
    dT.symmetry = "S"
    same_bits(MultiplyEngine().desymmetrized(dT), O.desymmetrize(T, "S"))


def test_block_diag_at_scale():
    """the product of square_sparse: 814 713 blocks in 4267 block rows, some two hundred of them on the diagonal"""
    X = S.reference(S.BY_NAME["square_sparse-NN-f64"]).C
    diag = X.rows() == X.col_i
    assert diag.sum() > 100 and not np.all(np.bincount(X.rows()[diag], minlength=X.nbr))   # (and block rows without one)
    src, start = elements(X, diag)
    ref = O.Bcsr(X.row_sizes, X.col_sizes, np.concatenate([[0], np.cumsum(np.bincount(X.rows()[diag], minlength=X.nbr))]), X.col_i[diag], start, X.data[src])
    D = dbcsr_get_block_diag(to_dev(X), engine=MultiplyEngine())
    torch.cuda.synchronize()
    same_bits(D, ref)


def test_report_the_lines():
    """for the record (profiles/symbolic_scale.txt): last_symbolic() of every case of this run"""
    print("\n".join("%-40s %s" % (n, LINES[n]) for n in S.NAMES if n in LINES))
