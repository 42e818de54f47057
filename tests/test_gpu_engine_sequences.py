"""One long-lived engine through mixed sequences of operations.  Every other GPU test that checks a multiply against the oracle makes a
fresh engine for its case; in deployment one engine per rank takes thousands of multiplies of different sizes, types and kernel families with filters,
crops, transposes, adds, norms and vector operations in between, and carries work areas that only grow, a saved plan, announcements, block norms and
the halves of two-call protocols from call to call.

A. a multiply does not depend on the engine's past: the walks of tests/engine_sequences.py on one engine, every case against the oracle at the bar of
   its own file AND bit for bit (index, data bytes, flop, last_kernel) against the same case on a fresh engine -- the choice of the kernel and the
   order of every sum are functions of the call.  No pool case has a legitimate dependence on history: the one memo that steers a multiply by what
   came before, kpass_memo, belongs to the one-call C entry dbcsr_amd_multiply (and the Python mirror's k passes engage at A rows above 1 MB only).
B. other users of the engine between two multiplies of the same operands.
C. the two-call protocols and the announcements, through the C entries.
D. a shipping and a lab engine alive together.
E. the algebra against itself: every public operation of operations.py and submatrix.py and the engine's filter, crop, transpose and desymmetrize in
   three walks on one engine, over ten matrices of three element types and ten sets of block sizes (the pool and the walks: tests/engine_sequences.py).

Host operands, oracle results (functools.lru_cache in tests/engine_sequences.py) and fresh-engine results (the module-scoped `fresh`) are computed once."""
import contextlib
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from dbcsr_amd import lib as L
from dbcsr_amd import operations as OPS
from dbcsr_amd import submatrix as SUB
from dbcsr_amd.cannon import gather_blocks
from dbcsr_amd.matrix import DbcsrMatrix, StreamHandle
from dbcsr_amd.multiply import MultiplyEngine, _z, dbcsr_multiply
from oracle import oracle as O
from tests import engine_sequences as ES
from tests import test_gpu_complex_multiply as CM
from tests import test_gpu_filter_in_place as FIP
from tests import test_gpu_random_sweep as SW
from tests.gpu_util import dev_to_bcsr, to_dev
from tests.test_numeric_choice import BIG

pytestmark = pytest.mark.gpu

KNOBS = ("DBCSR_AMD_MM_CLASSES", "DBCSR_AMD_MM_SYMBOLIC", "DBCSR_AMD_MM_WG_WAVES", "DBCSR_AMD_MM_HOT", "DBCSR_AMD_MM_PLAN", "DBCSR_AMD_MM_EXPECT_FILTER",
         "DBCSR_AMD_MM_KCHUNKS", "DBCSR_AMD_MM_KERNEL", "DBCSR_AMD_LAB")
CANARY = -77.25


@contextlib.contextmanager
def switches(env=()):
    """the environment an engine reads when it is made: the knobs cleared, then `env` (a tuple of (name, value) pairs)"""
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    os.environ.update(dict(env))
    try:
        yield
    finally:
        for k in KNOBS:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


@pytest.fixture(autouse=True)
def plain_environment():
    with switches():
        yield


# ---- a pool case on an engine -------------------------------------------------------------------------------------------------------------------------
def launch(eng, i):
    """pool[i] through the dbcsr_multiply mirror on eng, without a synchronisation of its own: (C on the device, flop, last_kernel)"""
    h = ES.host(i)
    p = h.par
    dA, dB, dC = to_dev(h.A), to_dev(h.B), to_dev(h.C)
    dC.symmetry = p["symm_c"]
    flop = [0]
    dbcsr_multiply(p["ta"], p["tb"], p["alpha"], dA, dB, p["beta"], dC, retain_sparsity=bool(p["retain"]), filter_eps=p["eps"] or None, flop=flop, engine=eng)
    return dC, flop[0], eng.last_kernel()


def run(eng, i):
    dC, flop, kernel = launch(eng, i)
    torch.cuda.synchronize()
    return dev_to_bcsr(dC), flop, kernel


def against_oracle(i, out, flop):
    h = ES.host(i)
    if h.complex:
        CM.same_index(out, h.ref)
        assert flop == h.info["flop"]
        CM.within_bar(out, h.R, h.bound)
    else:
        bad = SW.compare_case(h.par, out, flop, h.ref, h.info)
        assert bad is None, (bad, h)


def same_bits(x, y):
    return x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


def same_result(i, got, want, where):
    (out, flop, kernel), (fout, fflop, fkernel) = got, want
    assert kernel == fkernel, "%s, %r: kernel %s, on a fresh engine %s" % (where, ES.host(i), kernel, fkernel)
    assert flop == fflop, (where, ES.host(i))
    assert same_bits(out.row_p, fout.row_p) and same_bits(out.col_i, fout.col_i) and same_bits(out.blk_p, fout.blk_p), "%s, %r: another index" % (where, ES.host(i))
    assert same_bits(out.data, fout.data), "%s, %r: %d elements differ from the fresh engine's" % (where, ES.host(i), int(np.sum(out.data != fout.data)))


@pytest.fixture(scope="module")
def fresh():
    """fresh(i, env=(), lab=False): pool[i] on an engine of its own made under `env`, computed once"""
    cache = {}

    def get(i, env=(), lab=False):
        key = (i, tuple(env), bool(lab))
        if key not in cache:
            with switches(env):
                cache[key] = run(MultiplyEngine(lab=lab), i)
        return cache[key]

    return get


def walk(eng, indices, fresh, env=(), lab=False, where=""):
    for step, i in enumerate(indices):
        got = run(eng, i)
        against_oracle(i, got[0], got[1])
        same_result(i, got, fresh(i, env, lab), "%s step %d" % (where, step))


# ---- A. a multiply does not depend on the engine's past ------------------------------------------------------------------------------------------------------
def test_pool_families_on_the_device(fresh):
    for i in range(len(ES.POOL)):
        out, flop, kernel = fresh(i)
        against_oracle(i, out, flop)
        assert ES.family_of(kernel) == ES.FAMILY[i], (ES.host(i), kernel)


@pytest.mark.parametrize("name", list(ES.WALKS))
def test_walk_on_one_engine(name, fresh):
    walk(MultiplyEngine(), ES.WALKS[name], fresh, where=name)


@pytest.mark.parametrize("switch,name", [(s, n) for s, names in ES.SWITCH_WALKS.items() for n in names])
def test_walk_under_a_switch(switch, name, fresh):
    """the run-time compiled class kernels (their handles live in the engine) and the product-driven symbolic kernels, against fresh engines made under
    the same switch"""
    env = (tuple(switch.split("=")),)
    with switches(env):
        eng = MultiplyEngine()
    walk(eng, ES.WALKS[name], fresh, env=env, where="%s under %s" % (name, switch))
    if "CLASSES" in switch:
        assert any(fresh(i, env)[2].startswith("mm_numeric_f64_class[") for i in ES.WALKS[name]), "no case of the walk ran the class kernels"


def test_shuffled_a_on_a_side_stream(fresh):
    """no host synchronisation between the cases beyond what the calls make themselves; the results are copied back after the last one"""
    eng = MultiplyEngine()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    pending = []
    with torch.cuda.stream(side):
        for i in ES.WALKS["shuffled_a"]:
            pending.append((i,) + launch(eng, i))
    side.synchronize()
    for step, (i, dC, flop, kernel) in enumerate(pending):
        out = dev_to_bcsr(dC)
        against_oracle(i, out, flop)
        same_result(i, (out, flop, kernel), fresh(i), "side stream step %d" % step)


# ---- B. other users of the engine between two multiplies ---------------------------------------------------------------------------------------------------
MIX = [1, 13, 1, 23, 1, 32, 1, 7]
B_CASE = (300, 280, 300, 0.5, 0.5, 0.6, MIX, [1, 23, 1, 5, 1, 32], MIX)    # (A is square with equal row and column block sizes: set_diag applies to it)
B_ALPHA, B_BETA = 0.7, 1.3
IN_PLACE = ES.STALE_OPS_FIRST
REBUILT = ("filtered", "filtered_in_place", "crop", "transpose", "add_union", "desymmetrized", "twin_moved")
REUSED = ("gather", "add_flat", "scale", "add_on_diag", "trace", "dot", "norm_frobenius", "norm_maxabs", "norm_gershgorin", "norm_column", "gershgorin_norm",
          "get_diag", "set_diag", "scale_by_vector", "matvec", "multivec", "rank_update",
          "get_block_diag", "invert_block_diag", "scale_by_block_diag", "to_dense", "from_dense", "create_from_dense", "submatrix_gather", "submatrix_scatter",
          "hadamard_flat", "hadamard_two_patterns", "copy_keep_sparsity", "function_of_elements")
SUBS = [0, 7, 31, 119]   # the submatrices of part B's gather and scatter (of one per block column)


class Between:
    """the operands of part B on the device, the unrelated matrix X, and the operations"""

    def __init__(self):
        self.A, self.B, self.C = O.perf_case(*B_CASE)
        self.dA, self.dB, self.dC = to_dev(self.A), to_dev(self.B), to_dev(self.C)
        sizes = O.make_block_sizes(600, [1, 5, 1, 7, 1, 3])
        X = O.make_random_matrix(sizes, sizes, 0.5, O.RANDMAT_SEED_INIT + 91)
        setup = MultiplyEngine()
        dX = to_dev(X)
        OPS.dbcsr_add_on_diag(dX, 0.0, engine=setup)    # (every diagonal block present: add_on_diag then writes values only)
        torch.cuda.synchronize()
        self.X = dev_to_bcsr(dX)
        self.Y = O.Bcsr(self.X.row_sizes, self.X.col_sizes, self.X.row_p, self.X.col_i, self.X.blk_p, np.cos(np.arange(self.X.data.size, dtype=np.float64)))
        self.Z = O.make_random_matrix(sizes, sizes, 0.6, O.RANDMAT_SEED_INIT + 92)
        self.T = ES.triangle(self.X)    # (the stored triangle of X, packed: what the twin moves and desymmetrize take)
        n = int(sizes.sum())
        rng = np.random.default_rng(8)
        self.v, self.V, self.W = rng.uniform(-1, 1, n), rng.uniform(-1, 1, (n, 5)), rng.uniform(-1, 1, (n, 5))
        self.window = rng.uniform(-1, 1, (n, n))    # (a dense tensor of X's full size)
        norms = np.sort(np.sqrt(FIP.block_sq_norms(self.X)))
        self.eps = float(0.5 * (norms[len(norms) // 2 - 1] + norms[len(norms) // 2]))
        assert self.X.nblks > 10 * self.C.nblks

    def multiply(self, eng, dA=None):
        dC = self.dC.copy()
        dbcsr_multiply("N", "N", B_ALPHA, dA or self.dA, self.dB, B_BETA, dC, engine=eng)
        torch.cuda.synchronize()
        return dev_to_bcsr(dC)

    def operation(self, name, eng):
        """the operation on a copy of X: what it returned or wrote, as a tuple of numpy arrays and numbers"""
        X, Y, dv = to_dev(self.X), to_dev(self.Y), torch.as_tensor(self.v).cuda()
        mat = lambda D: tuple(D.to_host()[2:])
        if name in ("filtered", "filtered_in_place"):
            R = eng.filtered(X, self.eps, in_place=name == "filtered_in_place")
            assert 0 < R.nblks < X.nblks
            res = mat(R)
        elif name == "crop":
            res = mat(eng.cropped(X, (50, 400), (30, 500)))
        elif name == "transpose":
            res = mat(eng.transposed(X))
        elif name == "gather":
            res = (gather_blocks(X.data, self.X.blk_p[::3], FIP.block_sizes(self.X)[::3]).cpu().numpy(),)
        elif name == "add_flat":
            assert OPS.dbcsr_add(X, Y, 0.5, 2.0, engine=eng) is True
            res = mat(X)
        elif name == "add_union":
            assert OPS.dbcsr_add(X, to_dev(self.Z), 0.5, 2.0, engine=eng) is False
            res = mat(X)
        elif name == "scale":
            OPS.dbcsr_scale(X, -1.5, engine=eng)
            res = mat(X)
        elif name == "add_on_diag":
            OPS.dbcsr_add_on_diag(X, 0.75, engine=eng)
            res = mat(X)
        elif name == "trace":
            res = (OPS.dbcsr_trace(X, engine=eng),)
        elif name == "dot":
            res = (OPS.dbcsr_dot(X, Y, engine=eng),)
        elif name.startswith("norm_"):
            kind = {"frobenius": OPS.dbcsr_norm_frobenius, "maxabs": OPS.dbcsr_norm_maxabsnorm, "gershgorin": OPS.dbcsr_norm_gershgorin,
                    "column": OPS.dbcsr_norm_column}[name[5:]]
            r = OPS.dbcsr_norm(X, kind, engine=eng)
            res = (r.cpu().numpy() if isinstance(r, torch.Tensor) else r,)
        elif name == "gershgorin_norm":
            res = (OPS.dbcsr_gershgorin_norm(X, engine=eng),)
        elif name == "get_diag":
            res = (OPS.dbcsr_get_diag(X, engine=eng).cpu().numpy(),)
        elif name == "set_diag":
            OPS.dbcsr_set_diag(X, dv, engine=eng)
            res = mat(X)
        elif name == "scale_by_vector":
            OPS.dbcsr_scale_by_vector(X, dv, "left", engine=eng)
            res = mat(X)
        elif name == "matvec":
            res = (OPS.dbcsr_matvec(X, dv, alpha=1.5, trans="T", engine=eng).cpu().numpy(),)
        elif name == "multivec":
            res = (OPS.dbcsr_multivec(X, torch.as_tensor(self.V).cuda(), alpha=-0.5, engine=eng).cpu().numpy(),)
        elif name == "rank_update":
            OPS.dbcsr_rank_update(X, torch.as_tensor(self.V).cuda(), torch.as_tensor(self.W).cuda(), 0.3, 0.6, engine=eng)
            res = mat(X)
        elif name in ("desymmetrized", "twin_moved"):
            T = to_dev(self.T)
            T.symmetry = "S"
            res = mat(eng.desymmetrized(T) if name == "desymmetrized" else eng.twin_moved(T, 1, "S"))
        elif name == "get_block_diag":
            res = mat(OPS.dbcsr_get_block_diag(X, engine=eng))
        elif name == "invert_block_diag":     # (X's own diagonal blocks: none above 7)
            res = OPS.dbcsr_invert_block_diag(X, engine=eng) + mat(X)
        elif name == "scale_by_block_diag":
            OPS.dbcsr_scale_by_block_diag(X, OPS.dbcsr_get_block_diag(Y, engine=eng), "both", "T", 0.5, engine=eng)
            res = mat(X)
        elif name == "to_dense":
            res = (OPS.dbcsr_to_dense(X, engine=eng).cpu().numpy(),)
        elif name == "from_dense":
            OPS.dbcsr_from_dense(torch.as_tensor(self.window).cuda(), X, engine=eng)
            res = mat(X)
        elif name == "create_from_dense":     # (Z's blocks out of its dense form: the blocks Z lacks are zero and are dropped)
            M = OPS.dbcsr_create_from_dense(torch.as_tensor(self.Z.to_dense()).cuda(), X.row_blk_size, X.col_blk_size, eps=1e-3, engine=eng)
            assert 0 < M.nblks <= self.Z.nblks
            res = mat(M)
        elif name == "submatrix_gather":
            res = (SUB.dbcsr_submatrix_gather(X, SUB.dbcsr_submatrix_plan(X), subs=SUBS, pad_diag=1.0, engine=eng).cpu().numpy(),)
        elif name == "submatrix_scatter":     # (Y has X's pattern: its windows onto X)
            plan = SUB.dbcsr_submatrix_plan(X)
            SUB.dbcsr_submatrix_scatter(SUB.dbcsr_submatrix_gather(Y, plan, subs=SUBS, engine=eng), X, plan, subs=SUBS, engine=eng)
            res = mat(X)
        elif name == "hadamard_flat":
            assert OPS.dbcsr_hadamard_product(X, Y, X, engine=eng) is True
            res = mat(X)
        elif name == "hadamard_two_patterns":
            assert OPS.dbcsr_hadamard_product(X, to_dev(self.Z), X, engine=eng) is False
            assert 0 < X.nblks < self.X.nblks
            res = mat(X)
        elif name == "copy_keep_sparsity":
            OPS.dbcsr_copy(X, to_dev(self.Z), keep_sparsity=True, engine=eng)
            res = mat(X)
        elif name == "function_of_elements":
            OPS.dbcsr_function_of_elements(X, OPS.dbcsr_func_tanh, 0.1, 2.0, engine=eng)
            res = mat(X)
        else:
            raise AssertionError(name)
        torch.cuda.synchronize()
        return tuple(np.asarray(r) for r in res)


@pytest.fixture(scope="module")
def between():
    b = Between()
    b.first = b.multiply(MultiplyEngine())
    ref, info = O.multiply("N", "N", B_ALPHA, b.A, b.B, B_BETA, b.C)
    assert SW.compare_case(dict(dtype=np.float64), b.first, info["flop"], ref, info) is None
    return b


@pytest.fixture(scope="module")
def long_lived():
    """ONE engine for every test of part B and C that does not ask for a state of its own: their order is its history"""
    return MultiplyEngine()


def same_matrix_bits(x, y):
    return same_bits(x.row_p, y.row_p) and same_bits(x.col_i, y.col_i) and same_bits(x.blk_p, y.blk_p) and same_bits(x.data, y.data)


@pytest.mark.parametrize("name", REBUILT + REUSED)
def test_operation_between_two_multiplies(name, between, long_lived):
    eng, b = long_lived, between
    assert same_matrix_bits(b.multiply(eng), b.first)
    hits, misses = eng.plan_stats()
    got = b.operation(name, eng)
    want = b.operation(name, MultiplyEngine())
    assert len(got) == len(want) and all(same_bits(g, w) for g, w in zip(got, want)), "%s gives other bits than on a fresh engine" % name
    assert same_matrix_bits(b.multiply(eng), b.first), "the multiply after %s differs from the one before it" % name
    # filter, crop, transpose and the union add take the symbolic phase's work areas; the rest of the algebra has its own
    assert eng.plan_stats() == ((hits, misses + 1) if name in REBUILT else (hits + 1, misses)), name


def apply_in_place(eng, D, op, host):
    """the in-place changes of tests/engine_sequences.py (changed_host is their oracle side) on the device matrix D through the engine"""
    v = [torch.as_tensor(np.ascontiguousarray(x)).cuda() for x in ES.stale_vectors(host, op)]
    if op == "scale":
        OPS.dbcsr_scale(D, 4.0, engine=eng)
    elif op == "add":
        twin = DbcsrMatrix(D.row_blk_size, D.col_blk_size, D.row_p, D.col_i, D.blk_p, D.data.clone(), "D")
        assert OPS.dbcsr_add(D, twin, 1.0, 3.0, engine=eng) is True, "the flat add"
    elif op == "set_diag":
        OPS.dbcsr_set_diag(D, v[0], engine=eng)
    elif op == "scale_by_vector":
        OPS.dbcsr_scale_by_vector(D, v[0], "right", engine=eng)
    elif op == "rank_update":
        OPS.dbcsr_rank_update(D, v[0], v[1], 40.0, 0.25, "T", engine=eng)
    elif op == "add_on_diag":
        stamp = D.index_stamp()
        OPS.dbcsr_add_on_diag(D, 10.0, engine=eng)
        assert D.index_stamp() == stamp, "every diagonal block is stored: values only"
    elif op == "invert_block_diag":
        assert OPS.dbcsr_invert_block_diag(D, engine=eng) == (0, -1)
    elif op == "scale_by_block_diag":
        OPS.dbcsr_scale_by_block_diag(D, to_dev(ES.stale_operand(op)), "left", engine=eng)
    elif op == "function_of_elements":
        OPS.dbcsr_function_of_elements(D, OPS.dbcsr_func_inverse, engine=eng)
    elif op == "hadamard_in_place":
        assert OPS.dbcsr_hadamard_product(D, to_dev(ES.stale_operand(op)), D, engine=eng) is True, "the flat pass"
    elif op == "copy_keep_sparsity":
        OPS.dbcsr_copy(D, to_dev(ES.stale_operand(op)), keep_sparsity=True, engine=eng)
    elif op == "from_dense":
        OPS.dbcsr_from_dense(v[0], D, engine=eng)
    elif op == "submatrix_scatter":
        SUB.dbcsr_submatrix_scatter(v[0], D, SUB.dbcsr_submatrix_plan(D), engine=eng)
    else:
        raise AssertionError(op)


@pytest.mark.parametrize("op", IN_PLACE)
def test_operand_changed_in_place_between_two_multiplies(op, between, long_lived):
    """the plan may be reused, the values may not: the second multiply is the oracle's product of the CHANGED A"""
    eng, b = long_lived, between
    dA = to_dev(b.A)
    assert same_matrix_bits(b.multiply(eng, dA), b.first)
    hits, misses = eng.plan_stats()
    stamp = dA.index_stamp()
    apply_in_place(eng, dA, op, b.A)
    assert dA.index_stamp() == stamp
    got = b.multiply(eng, dA)
    assert eng.plan_stats() == (hits + 1, misses), "%s of an operand in place keeps its index: the plan is reused" % op
    changed = O.Bcsr(b.A.row_sizes, b.A.col_sizes, b.A.row_p, b.A.col_i, b.A.blk_p, ES.changed_host(b.A, op))
    ref, info = O.multiply("N", "N", B_ALPHA, changed, b.B, B_BETA, b.C)
    bad = SW.compare_case(dict(dtype=np.float64), got, info["flop"], ref, info)
    assert bad is None, (op, bad)
    assert not same_bits(got.data, b.first.data)


# ---- C. two-call protocols and announcements, through the C entries ----------------------------------------------------------------------------------------
def two_phase(eng, dA, dB, dC, eps_fly=0.0, alpha=1.0, beta=1.0, announce=None, symbolic_only=False):
    """dbcsr_amd_mm_symbolic_filtered, [dbcsr_amd_mm_expect_filter,] dbcsr_amd_mm_numeric[_z] on eng's handle; C_out's data area starts full of canaries"""
    lib, sth = eng.L, StreamHandle(None)
    a, b, cin = dA.desc(), dB.desc(), dC.desc()
    row_p = torch.empty(dC.nblkrows + 1, dtype=torch.int32, device="cuda")
    counts = L.MmCounts()
    cplx = dA.dtype.is_complex
    assert lib.dbcsr_amd_mm_symbolic_filtered(eng.h, dA.dtype_code, abs(complex(alpha)) if cplx else float(alpha), float(eps_fly), C.byref(a), C.byref(b),
                                              C.byref(cin), 0, row_p.data_ptr(), C.byref(counts), sth.ptr) == 0
    if symbolic_only:
        return None
    out = DbcsrMatrix(dC.row_blk_size, dC.col_blk_size, row_p, torch.empty(counts.c_nblks, dtype=torch.int32, device="cuda"),
                      torch.empty(counts.c_nblks, dtype=torch.int64, device="cuda"), torch.full((counts.c_nze,), CANARY, dtype=dA.dtype, device="cuda"), "C")
    cout = out.desc(out=True)
    if announce is not None:
        assert lib.dbcsr_amd_mm_expect_filter(eng.h, float(announce)) == 0
    if cplx:
        rc = lib.dbcsr_amd_mm_numeric_z(eng.h, _z(alpha), C.byref(a), C.byref(b), _z(beta), C.byref(cin), C.byref(cout), sth.ptr)
    else:
        rc = lib.dbcsr_amd_mm_numeric(eng.h, dA.dtype_code, float(alpha), C.byref(a), C.byref(b), float(beta), C.byref(cin), C.byref(cout), sth.ptr)
    assert rc == 0
    torch.cuda.synchronize()
    return out


def every_block_written(out, ref):
    """out (downloaded) has ref's index, no element of a named block is a canary, and the values are the oracle's at the sweep's bar"""
    got = dev_to_bcsr(out)
    assert np.array_equal(got.row_p, ref.row_p) and np.array_equal(got.col_i, ref.col_i)
    data = FIP.gathered(got)
    left = int(np.sum(data == CANARY))
    assert left == 0, "%d elements of %d named blocks were not written" % (left, got.nblks)
    assert np.all(np.abs(data - ref.data) <= 1e-10 * float(np.max(np.abs(ref.data))))
    return got


def hot_case(case="23_with_tails"):
    A, B_, Cm = FIP.inputs(case)
    return A, B_, Cm, FIP.oracle_product(case), FIP.quantile_eps(case, 0.5)


def test_announcement_is_cancelled_by_a_new_symbolic_phase():
    """(i) dbcsr_amd_mm_expect_filter, then a new symbolic phase: the next numeric phase writes every block"""
    A, B_, Cm, P, eps = hot_case()
    eng = MultiplyEngine()
    assert eng.L.dbcsr_amd_mm_expect_filter(eng.h, eps) == 0
    out = two_phase(eng, to_dev(A), to_dev(B_), to_dev(Cm), eps_fly=ES.ON_THE_FLY)
    assert eng.last_kernel() == "mm_numeric_f64_hot<23,23,23>"
    every_block_written(out, P)


@pytest.mark.parametrize("family", ["small8", "big", "z64"])
def test_announcement_to_a_family_that_leaves_no_norms(family):
    """(ii) every block is written, and a filter with a SMALLER eps than the announced one is served"""
    if family == "z64":
        h = ES.host(33)
        A, B_, Cm = h.A, h.B, h.C
    else:
        A, B_, Cm = FIP.inputs("small") if family == "small8" else O.perf_case(*BIG)
        ref = O.multiply("N", "N", 1.0, A, B_, 1.0, Cm)[0]
    eng = MultiplyEngine()
    dA, dB, dC = to_dev(A), to_dev(B_), to_dev(Cm)
    eps = 1e3   # (far above every block norm: a kernel that honoured it would write nothing)
    out = two_phase(eng, dA, dB, dC, eps_fly=ES.ON_THE_FLY, announce=eps)
    assert ES.family_of(eng.last_kernel()) == family, eng.last_kernel()
    if family == "z64":
        got = dev_to_bcsr(out)
        assert not np.any(got.data == CANARY)
        ref, _ = CM.index_reference("N", "N", A, B_, Cm, 1.0, False)
        CM.same_index(got, ref)
        R, bound = CM.reference("N", "N", 1.0, A, B_, 1.0, Cm)
        CM.within_bar(got, R, bound)
        return
    got = every_block_written(out, ref)
    small = float(np.median(np.sqrt(FIP.block_sq_norms(ref)))) * 1.000001
    kept = eng.filtered(out, small)
    torch.cuda.synchronize()
    want = ~(FIP.block_sq_norms(got) < small * small)
    assert 0 < want.sum() < want.size and np.array_equal(dev_to_bcsr(kept).col_i, got.col_i[want])


def test_smaller_eps_than_honoured_is_refused_and_the_engine_goes_on(fresh):
    """(iii) a numeric phase that honours the announcement, then filter_count with a smaller eps: -3, nothing counted, and the next multiplies of a walk
    have the bits of their fresh-engine results"""
    A, B_, Cm, P, eps = hot_case()
    eng = MultiplyEngine()
    out = two_phase(eng, to_dev(A), to_dev(B_), to_dev(Cm), eps_fly=ES.ON_THE_FLY, announce=eps)
    data = FIP.gathered(dev_to_bcsr(out))
    assert np.any(data == CANARY), "the hot kernel did not honour the announcement: the case checks nothing"
    src = out.desc()
    row_p = torch.full((out.nblkrows + 1,), -7, dtype=torch.int32, device="cuda")
    nb, nz = C.c_int64(-5), C.c_int64(-5)
    sth = StreamHandle(None)
    assert eng.L.dbcsr_amd_bcsr_filter_count(eng.h, out.dtype_code, C.byref(src), 0.5 * eps, row_p.data_ptr(), C.byref(nb), C.byref(nz), sth.ptr) == -3
    dst = DbcsrMatrix(out.row_blk_size, out.col_blk_size, row_p, torch.full((out.nblks,), -7, dtype=torch.int32, device="cuda"),
                      torch.full((out.nblks,), -7, dtype=torch.int64, device="cuda"), torch.full((out.data.numel(),), CANARY, dtype=torch.float64, device="cuda"), "X")
    d = dst.desc(out=True)
    assert eng.L.dbcsr_amd_bcsr_filter_apply(eng.h, out.dtype_code, C.byref(src), C.byref(d), sth.ptr) == -1, "an apply half after a refused count"
    torch.cuda.synchronize()
    assert int(row_p.max()) == -7 and int(dst.col_i.max()) == -7 and not bool((dst.data != CANARY).any()), "a refused call wrote its destination"
    walk(eng, ES.WALKS["shuffled_b"][:6], fresh, where="after -3")
    # the announced eps itself is still served for a new product
    out = two_phase(eng, to_dev(A), to_dev(B_), to_dev(Cm), eps_fly=ES.ON_THE_FLY, announce=eps)
    kept = dev_to_bcsr(eng.filtered(out, eps))
    want = ~(FIP.block_sq_norms(P) < eps * eps)
    assert np.array_equal(kept.col_i, P.col_i[want]) and np.all(np.abs(kept.data - FIP.gathered(O.Bcsr(P.row_sizes, P.col_sizes, kept.row_p, kept.col_i,
                                                                                                   P.blk_p[want], P.data))) <= 1e-10 * np.max(np.abs(P.data)))


def test_an_announcement_reaches_one_multiply_only():
    """(iv) the announced multiply, then an unannounced multiply of other operands on a family that would honour one: every block of the second is
    written, and a filter of it with a small eps is served"""
    A, B_, Cm, P, eps = hot_case()
    eng = MultiplyEngine()
    two_phase(eng, to_dev(A), to_dev(B_), to_dev(Cm), eps_fly=ES.ON_THE_FLY, announce=eps)
    A2, B2, C2, P2, eps2 = ES.stale_product("set_diag")
    out = two_phase(eng, to_dev(A2), to_dev(B2), to_dev(C2), eps_fly=ES.ON_THE_FLY)
    assert eng.last_kernel() == "mm_numeric_f64_hot<23,23,23>"
    got = every_block_written(out, P2)
    kept = dev_to_bcsr(eng.filtered(out, 0.01 * eps2))
    want = ~(FIP.block_sq_norms(got) < (0.01 * eps2) ** 2)
    assert np.array_equal(kept.col_i, got.col_i[want])


def filtered_index(P, keep):
    rows = P.rows()
    return np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=P.nbr))]).astype(np.int32), P.col_i[keep]


@pytest.mark.parametrize("op", ES.STALE_OPS)
def test_norms_left_behind_then_c_changed_in_place(op):
    """A filtered two-phase multiply whose kernel leaves the block norms (mm_numeric_f64_hot<23,23,23>), then C changed in place through the engine, then
    filter_count / apply: the kept blocks are the oracle's for the CHANGED C.  (Before the engine forgot the norms in its value-writing entries this
    kept the blocks of the unchanged C: profiles/engine_sequences.txt.)"""
    A, B_, Cm, P, eps = ES.stale_product(op)
    before, after, Q = ES.kept_sets(op)
    eng = MultiplyEngine()
    out = two_phase(eng, to_dev(A), to_dev(B_), to_dev(Cm), eps_fly=ES.ON_THE_FLY)
    assert eng.last_kernel() == "mm_numeric_f64_hot<23,23,23>"
    every_block_written(out, P)
    apply_in_place(eng, out, op, P)
    kept = eng.filtered(out, eps)
    torch.cuda.synchronize()
    got = dev_to_bcsr(kept)
    row_p, col_i = filtered_index(P, after)
    stale_row_p, stale_col_i = filtered_index(P, before)
    assert not (np.array_equal(got.row_p, stale_row_p) and np.array_equal(got.col_i, stale_col_i)), "the filter kept the blocks of C before the change"
    assert np.array_equal(got.row_p, row_p) and np.array_equal(got.col_i, col_i), "%d blocks kept, the oracle keeps %d" % (got.nblks, int(after.sum()))
    want = FIP.gathered(O.Bcsr(Q.row_sizes, Q.col_sizes, row_p, col_i, Q.blk_p[after], Q.data))
    assert np.all(np.abs(got.data - want) <= 1e-10 * float(np.max(np.abs(want))))


def test_norms_do_not_survive_a_new_symbolic_phase():
    """The norms a numeric kernel left are good until the next symbolic phase (include/dbcsr_amd_mm.h).  A multiply that is started on the engine and
    abandoned after its symbolic phase ends them: the filter that follows forms C's norms again, here of values the caller wrote in between."""
    A, B_, Cm, P, eps = hot_case()
    eng = MultiplyEngine()
    out = two_phase(eng, to_dev(A), to_dev(B_), to_dev(Cm), eps_fly=ES.ON_THE_FLY)
    h = ES.host(5)   # (an "NN" case: its operands are stored as the phases take them)
    assert h.par["ta"] + h.par["tb"] == "NN"
    two_phase(eng, to_dev(h.A), to_dev(h.B), to_dev(h.C), symbolic_only=True)
    out.data.mul_(4.0)
    got = dev_to_bcsr(eng.filtered(out, eps))
    _, after, _ = ES.kept_sets("scale")
    row_p, col_i = filtered_index(P, after)
    assert np.array_equal(got.row_p, row_p) and np.array_equal(got.col_i, col_i)


# count / apply pairs with another engine call between their halves.  EXPECT is read from the code (csrc/mm_engine_state.h: engine_takes_work_areas): the
# symbolic phase and every count half take the work areas the pending count left its answer in, so its apply half refuses (-1) and writes nothing; a
# reduction of the algebra has buffers of its own and the apply half gives the undisturbed pair's result.  The flat add keeps its answer in scalars.
# "desymmetrize" and "twin_canonical" are dbcsr_amd_bcsr_twin_count / _apply with mode 0 and 1 (kind 0) on the stored triangle of X: their count is in c_bm,
# c_pre and c_blk_p_ws.  "same_size_count" is ANOTHER pair's count on the very matrix of the pending one -- the same block count, the one thing a guard that
# only compares block counts cannot tell apart; "algebra_scan" runs three entries of the algebra whose exclusive_scan rewrites the scan's partial sums and
# alg_i32 / alg_i64, none of which a pending count lives in.
PAIRS = ("filter", "filter_index", "crop", "add_union", "add_flat", "desymmetrize", "twin_canonical")
TWIN_MODE = {"desymmetrize": 0, "twin_canonical": 1}
DISTURB = ("multiply", "other_count", "same_size_count", "reduction", "algebra_scan")
EXPECT = {(p, d): ("result" if d in ("reduction", "algebra_scan") or p == "add_flat" else "refuse") for p in PAIRS for d in DISTURB}


class Pair:
    def __init__(self, b, pair, eng, X=None, eps=None):
        self.pair, self.eng, self.sth = pair, eng, StreamHandle(None)
        self.eps = b.eps if eps is None else eps
        self.mode = TWIN_MODE.get(pair)
        self.host = (b.X if self.mode is None else b.T) if X is None else X
        self.X = to_dev(self.host)
        self.Y = to_dev(b.Z if pair == "add_union" else b.Y)
        self.row_p = torch.full((self.X.nblkrows + 1,), -7, dtype=torch.int32, device="cuda")
        self.nb, self.nz = C.c_int64(), C.c_int64()

    def count(self):
        lib, h, X = self.eng.L, self.eng.h, self.X
        src = X.desc()
        args = (self.row_p.data_ptr(), C.byref(self.nb), C.byref(self.nz))
        if self.pair in ("filter", "filter_index"):
            rc = lib.dbcsr_amd_bcsr_filter_count(h, X.dtype_code, C.byref(src), self.eps, *args, self.sth.ptr)
        elif self.pair == "crop":
            rc = lib.dbcsr_amd_bcsr_crop_count(h, X.dtype_code, C.byref(src), 50, 400, 30, 500, *args, self.sth.ptr)
        elif self.mode is not None:
            rc = lib.dbcsr_amd_bcsr_twin_count(h, C.byref(src), self.mode, *args, self.sth.ptr)
        else:
            y, same = self.Y.desc(), C.c_int32()
            rc = lib.dbcsr_amd_bcsr_add_count(h, C.byref(src), C.byref(y), 0, *args, C.byref(same), self.sth.ptr)
            assert same.value == (1 if self.pair == "add_flat" else 0)
        assert rc == 0 and 0 < self.nb.value

    def apply(self):
        """(return code, the destination's col_i, blk_p and data on the host)"""
        lib, h, X = self.eng.L, self.eng.h, self.X
        nb = self.nb.value
        data = X.data if self.pair == "filter_index" else torch.full((self.nz.value,), CANARY, dtype=torch.float64, device="cuda")
        dst = DbcsrMatrix(X.row_blk_size, X.col_blk_size, self.row_p, torch.full((nb,), -7, dtype=torch.int32, device="cuda"),
                          torch.full((nb,), -7, dtype=torch.int64, device="cuda"), data, "dst", nze=self.nz.value)
        src, d = X.desc(), dst.desc(out=True)
        if self.pair == "filter":
            rc = lib.dbcsr_amd_bcsr_filter_apply(h, X.dtype_code, C.byref(src), C.byref(d), self.sth.ptr)
        elif self.pair == "filter_index":
            rc = lib.dbcsr_amd_bcsr_filter_apply_index(h, C.byref(src), C.byref(d), self.sth.ptr)
        elif self.pair == "crop":
            rc = lib.dbcsr_amd_bcsr_crop_apply(h, X.dtype_code, C.byref(src), C.byref(d), self.sth.ptr)
        elif self.mode is not None:
            rc = lib.dbcsr_amd_bcsr_twin_apply(h, X.dtype_code, C.byref(src), self.mode, 0, C.byref(d), self.sth.ptr)
        else:
            y = self.Y.desc()
            rc = lib.dbcsr_amd_bcsr_add_apply(h, X.dtype_code, _z(0.5), C.byref(src), _z(2.0), C.byref(y), C.byref(d), self.sth.ptr)
        torch.cuda.synchronize()
        return rc, dst.col_i.cpu().numpy(), dst.blk_p.cpu().numpy(), data.cpu().numpy()


@pytest.mark.parametrize("disturb", DISTURB)
@pytest.mark.parametrize("pair", PAIRS)
def test_another_call_between_count_and_apply(pair, disturb, between, long_lived, fresh):
    b, eng = between, long_lived
    alone = Pair(b, pair, MultiplyEngine())
    alone.count()
    rc0, *want = alone.apply()
    assert rc0 == 0
    p = Pair(b, pair, eng)
    x_before = p.X.data.cpu().numpy()
    p.count()
    assert (p.nb.value, p.nz.value) == (alone.nb.value, alone.nz.value)
    if disturb == "multiply":
        same_result(9, run(eng, 9), fresh(9), "between the halves of %s" % pair)
    elif disturb == "other_count":
        Pair(b, "crop" if pair != "crop" else "filter", eng, X=ES.host(16).C, eps=0.5).count()   # (of another matrix, of other sizes)
    elif disturb == "same_size_count":
        other = Pair(b, "crop" if pair != "crop" else "filter", eng, X=p.host)   # (of the pending count's own matrix: the same block count)
        assert other.X.nblks == p.X.nblks
        other.count()
    elif disturb == "algebra_scan":
        h16 = ES.host(16).C
        D = OPS.dbcsr_get_block_diag(to_dev(b.Z), engine=eng)
        M = OPS.dbcsr_create_from_dense(torch.as_tensor(h16.to_dense()).cuda(), h16.row_sizes, h16.col_sizes, eps=0.5, engine=eng)
        assert D.nblks > 0 and 0 < M.nblks <= h16.nblks and OPS.dbcsr_gershgorin_norm(to_dev(b.Y), engine=eng) > 0
    else:
        assert OPS.dbcsr_frobenius_norm(to_dev(ES.host(16).C), engine=eng) > 0 and np.isfinite(OPS.dbcsr_trace(to_dev(b.Y), engine=eng))
    rc, *got = p.apply()
    if EXPECT[pair, disturb] == "refuse":
        assert rc == -1
        assert np.all(got[0] == -7) and np.all(got[1] == -7), "a refused apply half wrote its destination's index"
        assert same_bits(got[2], x_before) if pair == "filter_index" else np.all(got[2] == CANARY), "a refused apply half wrote its destination's data"
    else:
        assert rc == 0
        assert all(same_bits(g, w) for g, w in zip(got, want)), "the pair's result differs from the undisturbed pair's"
    assert same_bits(p.X.data.cpu().numpy(), x_before)
    same_result(9, run(eng, 9), fresh(9), "after %s / %s" % (pair, disturb))


def test_refusals_leave_the_engine_usable(fresh, between):
    """between the cases of a walk: the refusals the C-ABI tests of the algebra files provoke (-1, -10) and Python's ValueError / TypeError (-3: test
    (iii)); every multiply of the walk has the bits of its fresh-engine result"""
    from tests.test_gpu_rank_update import c_update
    eng, b = MultiplyEngine(), between
    X = to_dev(b.X)
    n = int(b.X.row_sizes.sum())
    x = torch.ones((n, 3), dtype=torch.float64, device="cuda")
    before = X.data.clone()
    sth = StreamHandle(None)
    d = X.desc()
    out2 = (C.c_double * 2)()

    def expect(exc, f, *a, **k):
        with pytest.raises(exc):
            f(*a, **k)

    T = to_dev(b.T)
    t = T.desc()
    t_before = T.data.clone()
    t_row_p = torch.empty(T.nblkrows + 1, dtype=torch.int32, device="cuda")
    t_nb, t_nz = C.c_int64(), C.c_int64()

    def twin_with_another_mode():
        """a count of mode 1 (triangle -> canonical form), then the apply half of mode 0 (desymmetrize): its result would be larger than what was counted"""
        assert eng.L.dbcsr_amd_bcsr_twin_count(eng.h, C.byref(t), 1, t_row_p.data_ptr(), C.byref(t_nb), C.byref(t_nz), sth.ptr) == 0
        assert t_nb.value == T.nblks
        return eng.L.dbcsr_amd_bcsr_twin_apply(eng.h, T.dtype_code, C.byref(t), 0, 0, C.byref(t), sth.ptr) == -1

    refusals = [
        lambda: eng.L.dbcsr_amd_bcsr_twin_apply(eng.h, T.dtype_code, C.byref(t), 0, 0, C.byref(t), sth.ptr) == -1,   # this engine has never counted
        lambda: c_update(eng, X, "T", 1.0, 1.0, 3, x, n, 3, x, n, 3, code=L.dbcsr_type_complex_4) == -10,
        lambda: c_update(eng, X, "T", 1.0, 1.0, 3, None, n, 3, x, n, 3) == -1,
        lambda: c_update(eng, X, "N", 1.0, 1.0, 3, x, n, 3, x, n, 3) == -1,
        lambda: eng.L.dbcsr_amd_bcsr_add_apply(eng.h, X.dtype_code, _z(1.0), C.byref(d), _z(1.0), C.byref(d), C.byref(d), sth.ptr) == -1,   # no count
        lambda: eng.L.dbcsr_amd_bcsr_trace(eng.h, 99, C.byref(d), out2, sth.ptr) == -10,
        lambda: eng.L.dbcsr_amd_bcsr_crop_apply(eng.h, X.dtype_code, C.byref(d), C.byref(d), sth.ptr) == -1,                                 # no count
        lambda: eng.L.dbcsr_amd_bcsr_matvec(eng.h, X.dtype_code, b"N", _z(1.0), C.byref(d), -1, x.data_ptr(), n, _z(0.0), x.data_ptr(), n, sth.ptr) == -1,
        lambda: expect(ValueError, OPS.dbcsr_scale_by_vector, X, x[:, 0].contiguous(), "up", engine=eng) is None,
        lambda: expect(TypeError, OPS.dbcsr_rank_update, X, x.float(), x, engine=eng) is None,
        lambda: expect(ValueError, dbcsr_multiply, "N", "T", 1.0, to_dev(b.A), to_dev(b.B), 1.0, to_dev(b.C), engine=eng) is None,   # (after its transposes ran)
        lambda: expect(TypeError, dbcsr_multiply, "N", "N", 1.0, to_dev(b.A), to_dev(b.B), 1.0, to_dev(O.Bcsr(
            b.C.row_sizes, b.C.col_sizes, b.C.row_p, b.C.col_i, b.C.blk_p, b.C.data.astype(np.float32))), engine=eng) is None,
        lambda: expect(ValueError, eng.accumulate, 1.0, to_dev(b.A), to_dev(b.B), eng.filtered(to_dev(b.C), float(np.median(np.sqrt(FIP.block_sq_norms(b.C)))),
                                                                                                in_place=True)) is None,
        twin_with_another_mode,
    ]
    indices = ES.WALKS["shuffled_b"][:len(refusals)]
    for step, (i, refuse) in enumerate(zip(indices, refusals)):
        assert refuse(), "refusal %d" % step
        got = run(eng, i)
        against_oracle(i, got[0], got[1])
        same_result(i, got, fresh(i), "after refusal %d" % step)
    assert torch.equal(X.data, before), "a refusal wrote the matrix"
    assert torch.equal(T.data, t_before) and np.array_equal(T.to_host()[3], b.T.col_i), "a refused twin_apply wrote the matrix"


# ---- D. two engines in one process ---------------------------------------------------------------------------------------------------------------------------
def test_a_shipping_and_a_lab_engine_alive_together(fresh):
    ship, lab = MultiplyEngine(lab=False), MultiplyEngine(lab=True)
    assert ship.L is not lab.L
    for step, i in enumerate(ES.WALKS["shuffled_a"]):
        for eng, is_lab in ((ship, False), (lab, True)):
            got = run(eng, i)
            against_oracle(i, got[0], got[1])
            same_result(i, got, fresh(i, (), is_lab), "%s engine, step %d" % ("lab" if is_lab else "shipping", step))


# ---- E. an algebra walk --------------------------------------------------------------------------------------------------------------------------------------
# tests/engine_sequences.py has the pool, the operations and the walks.  alg_run is one operation on one pool matrix through an engine: what it returned or
# wrote, as a tuple of numpy arrays and numbers.  alg_check compares such a result with the reference that the operation's own test file uses, at that
# file's bar (the helpers are imported; this file has no tolerance of its own).  A step of a walk must have the bits of the same operation on a fresh
# engine; the fresh results are computed and checked once per (operation, matrix).
from tests import elementwise_ref as R                # noqa: E402
from tests import submatrix_ref as SR                 # noqa: E402
from tests import test_gpu_block_inverse as BI        # noqa: E402
from tests import test_gpu_block_scale as BS          # noqa: E402
from tests import test_gpu_dense as GD                # noqa: E402
from tests import test_gpu_elementwise as EW          # noqa: E402
from tests import test_gpu_matrix_norms as MN         # noqa: E402
from tests import test_gpu_matrix_ops as MO           # noqa: E402
from tests import test_gpu_matvec as MV               # noqa: E402
from tests import test_gpu_multivec as MVV            # noqa: E402
from tests import test_gpu_rank_update as RU          # noqa: E402


def cu(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def alg_scalar(h, name):
    """the scalars of an operation, as its own test file takes them"""
    cplx = h.dtype.kind == "c"
    if name in ("add_flat", "add_union"):
        return MO.scalars(h.dtype)
    if name == "scale":
        return MO.scalars(h.dtype)[1]
    if name == "add_on_diag":
        return 1.5 - 0.5j if cplx else -1.5
    if name == "scale_by_block_diag":
        return BS.alpha_of(h.dtype)
    return MV.scalars(h.dtype)    # matvec, multivec, rank_update


def alg_vectors(h, name):
    """the dense operands of an operation on the host"""
    n, dt = h.n, h.dtype
    if name == "set_diag":
        return (MN.random_vector(n, dt, 4),)
    if name == "scale_by_vector":
        return (MN.random_vector(n, dt, 5),)
    if name == "matvec":
        return MN.random_vector(n, dt, 21), MN.random_vector(n, dt, 22)
    if name == "multivec":
        return MVV.random_vectors(n, 5, dt, 41), MVV.random_vectors(n, 5, dt, 42)
    if name == "rank_update":
        return RU.inputs(h.M, 3)
    if name == "from_dense":
        return (np.ascontiguousarray(MN.random_vector(n * n, dt, 9).reshape(n, n)),)
    if name == "submatrix_scatter":
        return (np.ascontiguousarray(MN.random_vector(len(h.subs) * h.sub_n ** 2, dt, 11).reshape(len(h.subs), h.sub_n, h.sub_n)),)
    raise AssertionError(name)


def alg_block_diag(h):
    """the operand of dbcsr_scale_by_block_diag: the diagonal blocks of Q"""
    return MN.subset(h.Q, lambda r, c: r == c)


def alg_run(name, eng, k):
    h = ES.alg(k)
    M = to_dev(h.M)
    mat = lambda D: tuple(D.to_host()[2:])
    if name in ("add_flat", "add_union"):
        al, be = alg_scalar(h, name)
        assert OPS.dbcsr_add(M, to_dev(h.T if name == "add_flat" else h.Q), al, be, engine=eng) is (name == "add_flat")
        res = mat(M)
    elif name == "scale":
        OPS.dbcsr_scale(M, alg_scalar(h, name), engine=eng)
        res = mat(M)
    elif name == "add_on_diag":
        OPS.dbcsr_add_on_diag(M, alg_scalar(h, name), engine=eng)
        res = mat(M)
    elif name == "trace":
        res = (OPS.dbcsr_trace(M, engine=eng),)
    elif name == "dot":
        res = (OPS.dbcsr_dot(M, to_dev(h.Q), engine=eng),)
    elif name == "frobenius_norm":
        res = (OPS.dbcsr_frobenius_norm(M, engine=eng),)
    elif name == "maxabs_norm":
        res = (OPS.dbcsr_maxabs_norm(M, engine=eng),)
    elif name == "gershgorin_norm":
        res = (OPS.dbcsr_gershgorin_norm(M, engine=eng),)
    elif name == "norm_column":
        res = (OPS.dbcsr_norm(M, OPS.dbcsr_norm_column, engine=eng).cpu().numpy(),)
    elif name == "get_diag":
        res = (OPS.dbcsr_get_diag(M, engine=eng).cpu().numpy(),)
    elif name == "set_diag":
        OPS.dbcsr_set_diag(M, cu(alg_vectors(h, name)[0]), engine=eng)
        res = mat(M)
    elif name == "scale_by_vector":
        OPS.dbcsr_scale_by_vector(M, cu(alg_vectors(h, name)[0]), "right", engine=eng)
        res = mat(M)
    elif name == "matvec":
        x, y = alg_vectors(h, name)
        al, be = alg_scalar(h, name)
        res = (OPS.dbcsr_matvec(M, cu(x), cu(y), al, be, "T", engine=eng).cpu().numpy(),)
    elif name == "multivec":
        x, y = alg_vectors(h, name)
        al, be = alg_scalar(h, name)
        res = (OPS.dbcsr_multivec(M, cu(x), cu(y), al, be, "N", engine=eng).cpu().numpy(),)
    elif name == "rank_update":
        x, y = alg_vectors(h, name)
        al, be = alg_scalar(h, name)
        OPS.dbcsr_rank_update(M, cu(x), cu(y), al, be, "T", engine=eng)
        res = mat(M)
    elif name == "get_block_diag":
        res = mat(OPS.dbcsr_get_block_diag(M, engine=eng))
    elif name == "invert_block_diag":
        res = OPS.dbcsr_invert_block_diag(M, engine=eng) + mat(M)
    elif name == "scale_by_block_diag":
        OPS.dbcsr_scale_by_block_diag(M, to_dev(alg_block_diag(h)), "left", "T", alg_scalar(h, name), engine=eng)
        res = mat(M)
    elif name == "to_dense":
        res = (OPS.dbcsr_to_dense(M, engine=eng).cpu().numpy(),)
    elif name == "from_dense":
        OPS.dbcsr_from_dense(cu(alg_vectors(h, name)[0]), M, engine=eng)
        res = mat(M)
    elif name == "create_from_dense":
        res = mat(OPS.dbcsr_create_from_dense(cu(MN.dense(h.Q)), M.row_blk_size, M.col_blk_size, eps=GD.EPS, engine=eng))
    elif name in ("hadamard_flat", "hadamard_two_patterns"):
        assert OPS.dbcsr_hadamard_product(M, to_dev(h.T if name == "hadamard_flat" else h.Q), M, engine=eng) is (name == "hadamard_flat")
        res = mat(M)
    elif name == "copy_keep_sparsity":
        OPS.dbcsr_copy(M, to_dev(h.Q), keep_sparsity=True, engine=eng)
        res = mat(M)
    elif name == "function_of_elements":
        F = to_dev(h.F)
        OPS.dbcsr_function_of_elements(F, EW.FUNCS[ES.ALG_FUNCTION[0]], *ES.ALG_FUNCTION[1:], engine=eng)
        res = mat(F)
    elif name == "submatrix_gather":
        res = (SUB.dbcsr_submatrix_gather(M, SUB.dbcsr_submatrix_plan(M), subs=h.subs, pad_diag=1.0, engine=eng).cpu().numpy(),)
    elif name == "submatrix_scatter":
        SUB.dbcsr_submatrix_scatter(cu(alg_vectors(h, name)[0]), M, SUB.dbcsr_submatrix_plan(M), subs=h.subs, engine=eng)
        res = mat(M)
    elif name == "submatrix_apply":      # (an exact function, as the submatrix file's own test takes one)
        res = mat(SUB.dbcsr_submatrix_apply(M, lambda X: X.transpose(-1, -2).contiguous(), plan=SUB.dbcsr_submatrix_plan(M, h.groups), engine=eng))
    elif name == "filtered":
        res = mat(eng.filtered(M, h.eps))
    elif name == "cropped":
        res = mat(eng.cropped(M, *h.crop))
    elif name == "transposed":
        res = mat(eng.transposed(M))
    elif name == "desymmetrized":
        T = to_dev(h.tri)
        T.symmetry = h.symmetry
        res = mat(eng.desymmetrized(T))
    else:
        raise AssertionError(name)
    torch.cuda.synchronize()
    return tuple(np.asarray(r) for r in res)


def alg_check(name, k, res):
    """the result of alg_run against the reference of the operation's own test file, at that file's bar"""
    h = ES.alg(k)
    M, dt = h.M, h.dtype
    cplx = dt.kind == "c"
    host = lambda r, like=M: O.Bcsr(like.row_sizes, like.col_sizes, *r[-4:])

    def same_matrix(r, want):
        MO.same_index(host(r, want), want)
        assert MN.same_bits(r[-1], want.data), "%s of %r: the index is the reference's, the values are not" % (name, h)

    kept_index = lambda r: MO.same_index(host(r), M) is None
    if name in ("add_flat", "add_union"):
        ref, scale = MO.reference_add(M, h.T if name == "add_flat" else h.Q, *alg_scalar(h, name))
        MO.same_index(host(res), ref)
        assert np.all(np.abs(res[-1] - ref.data) <= 4 * MO.factor(dt) * MO.unit(dt) * scale)
    elif name == "scale":
        al = alg_scalar(h, name)
        assert kept_index(res) and np.all(np.abs(res[-1] - MO.times(al, M.data, dt)) <= 2 * MO.factor(dt) * MO.unit(dt) * abs(al) * np.abs(M.data))
    elif name == "add_on_diag":
        al = alg_scalar(h, name)
        at, _ = MN.diagonal_places(M)
        off = np.ones(M.data.size, bool)
        off[at] = False
        assert kept_index(res) and MN.same_bits(res[-1][off], M.data[off]), "everything off the diagonal stays as it is"
        ref = (M.data[at] + np.asarray(al, dt)).astype(dt)
        assert np.all(np.abs(res[-1][at] - ref) <= 4 * MO.factor(dt) * MO.unit(dt) * (np.abs(M.data[at]) + abs(al)))
    elif name == "trace":
        at, _ = MN.diagonal_places(M)
        got = res[0].item()
        if cplx:
            MO.check_sum(got.real, M.data[at].real)
            MO.check_sum(got.imag, M.data[at].imag)
        else:
            MO.check_sum(got, M.data[at])
    elif name == "dot":
        bx, by = MO.blocks_of(M), MO.blocks_of(h.Q)
        MO.check_sum(res[0].item(), np.concatenate([bx[key].astype(np.float64) * by[key].astype(np.float64) for key in sorted(set(bx) & set(by))]))
    elif name == "frobenius_norm":
        terms = MO.real_terms(M.data)
        ref = math.sqrt(math.fsum(terms.tolist()))
        assert abs(res[0].item() - ref) <= (len(terms) + 5) * MO.U53 * ref
    elif name == "maxabs_norm":
        ref = float(np.max(np.abs(M.data)))
        assert abs(res[0].item() - ref) <= 4 * MN.U53 * ref if cplx else res[0].item() == ref
    elif name == "gershgorin_norm":
        refs, bars = MN.reference_sums(MN.dense(M), MN.pattern_mask(M), 0, 0)
        assert abs(res[0].item() - float(np.max(refs))) <= float(np.max(bars))
    elif name == "norm_column":
        mask = MN.pattern_mask(M)
        refs, _ = MN.reference_sums(MN.dense(M), mask, 1, 1)
        counts = MN.real_terms(np.ones(1, dt)).size * mask.sum(axis=0)
        MN.check_vector(res[0], np.sqrt(refs), (counts + 5) * MN.U53 * np.sqrt(refs), "column norms")
    elif name == "get_diag":
        assert MN.same_bits(res[0], np.ascontiguousarray(np.diagonal(MN.dense(M))).astype(dt))
    elif name == "set_diag":
        at, idx = MN.diagonal_places(M)
        area = M.data.copy()
        area[at] = alg_vectors(h, name)[0][idx]
        assert kept_index(res) and MN.same_bits(res[-1], area)
    elif name == "scale_by_vector":
        ref, scale = MN.scaled_area(M, alg_vectors(h, name)[0], "right")
        assert kept_index(res) and (np.all(np.abs(res[-1] - ref) <= 4 * MN.U53 * scale) if cplx else MN.same_bits(res[-1], ref))
    elif name == "matvec":
        x, y = alg_vectors(h, name)
        ref, bar = MV.reference(MV.dense_parts(M, "N"), "T", *alg_scalar(h, name), x, y)
        MV.within(res[0], ref, bar, "matvec")
    elif name == "multivec":
        x, y = alg_vectors(h, name)
        ref, bar = MVV.reference_columns(MV.dense_parts(M, "N"), "N", *alg_scalar(h, name), x, y)
        MVV.within_columns(res[0], ref, bar, "multivec")
    elif name == "rank_update":
        x, y = alg_vectors(h, name)
        F, absF, mask = RU.parts_of(M)
        ref, bar = RU.reference(F, absF, *alg_scalar(h, name), x, y, "T")
        assert kept_index(res)
        RU.stored_within(res[-1], M, ref, bar, mask, "rank update")
    elif name == "get_block_diag":
        same_matrix(res, MN.subset(M, lambda r, c: r == c))
    elif name == "invert_block_diag":
        assert (res[0].item(), res[1].item()) == (0, -1) and kept_index(res)
        BI.check_inverses(M, host(res), "alg[%d]" % k)
        assert BI.others_kept(M, host(res))
    elif name == "scale_by_block_diag":
        ref, bar = BS.reference(MN.dense(M).astype(BS.wide(dt)), alg_block_diag(h), "left", "T", alg_scalar(h, name), dt)
        assert kept_index(res)
        BS.stored_within(res[-1], M, ref, bar, MN.pattern_mask(M), "block scale")
    elif name == "to_dense":
        assert MN.same_bits(res[0], MN.dense(M))
    elif name == "from_dense":
        assert kept_index(res) and MN.same_bits(res[-1], GD.expected_area(M, M.data, alg_vectors(h, name)[0]))
    elif name == "create_from_dense":
        same_matrix(res, GD.filtered_host(MN.dense(h.Q), h.sizes, h.sizes, GD.EPS))
    elif name in ("hadamard_flat", "hadamard_two_patterns"):
        EW.assert_product(host(res), M, h.T if name == "hadamard_flat" else h.Q, None)
    elif name == "copy_keep_sparsity":
        assert kept_index(res) and R.same_bits(res[-1], R.reference_copy_onto(h.Q, M))
    elif name == "function_of_elements":
        assert EW.function_excess(h.F, *ES.ALG_FUNCTION, res[-1]) <= (1 if dt == np.float32 else EW.C64)
    elif name == "submatrix_gather":
        assert MN.same_bits(res[0], SR.gathered(M, "N", h.sets, h.subs, h.sub_n, 1.0))
    elif name == "submatrix_scatter":
        area, written = SR.scattered_area(M, M.data, h.sets, h.owner, alg_vectors(h, name)[0], h.subs)
        assert written and kept_index(res) and MN.same_bits(res[-1], area)
    elif name == "submatrix_apply":
        D = MN.dense(M)
        windows = [np.ascontiguousarray(SR.window(D, S, h.sizes, int(SR.elements_of(S, h.sizes).size), 1.0).T) for S in h.group_sets]
        area, written = SR.scattered_area(M, M.data, h.group_sets, h.group_owner, windows)
        assert written and kept_index(res) and MN.same_bits(res[-1], area)
    elif name == "filtered":
        keep = ~(ES.block_sq_moduli(M) < h.eps * h.eps)
        assert 0 < keep.sum() < keep.size
        same_matrix(res, ES.subset(M, keep))
    elif name == "cropped":
        same_matrix(res, O.crop(M, *h.crop))
    elif name == "transposed":
        same_matrix(res, O.transposed(M))
    elif name == "desymmetrized":
        got = host(res)
        assert got.nblks == 2 * h.tri.nblks - h.nb and np.array_equal(got.blk_p, np.concatenate([[0], np.cumsum(FIP.block_sizes(got))[:-1]]))
        assert MN.same_bits(MN.dense(got), MN.desymmetrized_dense(h.tri, h.symmetry).astype(dt))
    else:
        raise AssertionError(name)


@pytest.fixture(scope="module")
def fresh_alg():
    """fresh_alg(name, k): the operation on pool matrix k on an engine of its own, computed once and checked once against its reference"""
    cache = {}

    def get(name, k):
        if (name, k) not in cache:
            cache[name, k] = alg_run(name, MultiplyEngine(), k)
            alg_check(name, k, cache[name, k])
        return cache[name, k]

    return get


@pytest.mark.parametrize("name", list(ES.ALG_WALKS))
def test_algebra_walk_on_one_engine(name, fresh, fresh_alg):
    eng = MultiplyEngine()
    same_result(9, run(eng, 9), fresh(9), "before the %s walk of the algebra" % name)
    for step, (op, k) in enumerate(ES.ALG_WALKS[name]):
        got, want = alg_run(op, eng, k), fresh_alg(op, k)
        assert len(got) == len(want) and all(same_bits(g, w) for g, w in zip(got, want)), \
            "%s step %d: %s of %r gives other bits than on a fresh engine" % (name, step, op, ES.alg(k))
    same_result(9, run(eng, 9), fresh(9), "after the %s walk of the algebra" % name)
