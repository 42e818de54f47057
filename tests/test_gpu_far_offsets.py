"""Block offsets at and above 2^31 and 2^32 elements in every kernel that decodes a product record or takes a matrix' data area.

The operands of each case are a few hundred small blocks scattered through one arena of 2^36 + 2^26 bytes (tests/far_arena.py: zones around the
element offsets 2^29, 2^31, 2^32, 2^32 + 2^31, 2^33, 2^34; one block straddles each; canaries around every run of blocks; NaN where a decode that
drops or swaps a high byte would read).  tests/test_far_placement.py checks without a GPU that the placements of every case here reach the high bytes and
top bits they are meant to.

Every multiply kernel family (the switches, cases and expected names of tests/test_gpu_kernel_variants.py, plus the small / mid / big / complex kernels
and the lab's band, tile and group kernels) runs with A, B and C_in far under both plans and once more with A's and B's placements exchanged:
the kernel's name, C's index against the oracle, the values within rel_err 1e-10 (float64, complex128; the modulus for complex) / 2e-5 (float32) of
the oracle's multiply of the packed host matrices, and every guard bit for bit."""
import functools

import numpy as np
import pytest
import torch

from dbcsr_amd import lib as L
from dbcsr_amd.matrix import DbcsrMatrix, StreamHandle
from dbcsr_amd.multiply import MultiplyEngine, dbcsr_multiply
from dbcsr_amd.operations import (dbcsr_add, dbcsr_add_on_diag, dbcsr_dot, dbcsr_get_diag, dbcsr_scale, dbcsr_scale_by_vector, dbcsr_set_diag)
from oracle import oracle as O
from tests import far_arena as FA
from tests import test_gpu_band_kernel as BAND
from tests import test_gpu_big_blocks as BIGB
from tests import test_gpu_f32_group as G32
from tests import test_gpu_f64_group as G64
from tests import test_gpu_kernel_variants as KV
from tests import test_gpu_small_blocks as SMALL
from tests import test_gpu_tile_kernel as TILE
from tests.gpu_util import dev_to_bcsr, rel_err, to_dev

pytestmark = pytest.mark.gpu

F64, F32, Z64 = np.float64, np.float32, np.complex128
TOL = {np.dtype(F64): 1e-10, np.dtype(F32): 2e-5, np.dtype(Z64): 1e-10}
CLEAR = tuple(sorted(set(SMALL.ENV + BIGB.ENV + G32.ENV + G64.ENV + BAND.ENV_KEYS + TILE.ENV_KEYS + ("DBCSR_AMD_LAB", "DBCSR_AMD_MM_SMALL", "DBCSR_AMD_MM_F64_GROUP"))))
PLANS = ["lines", "blocks", "lines_exchanged"]
# the lab's group kernels share B along a block column and take it only with offsets that ascend with the block index (the engine passes them over for any
# other B and the kernel of the default choice runs: DESIGN 6); their entries run under the plan that keeps the index order
ASCENDING_PLANS = ["ascending", "ascending_exchanged"]


def _keeps(env):
    """switches that change who decodes the record: these variants stay even where the kernel's name repeats"""
    return env.get("DBCSR_AMD_MM_WORK") == "0" or "DBCSR_AMD_MM_SYMBOLIC" in env or env.get("DBCSR_AMD_MM_WG_WAVES") in ("1", "4")


def _representatives(variants, dtype):
    """one entry per distinct expected kernel name (ablation variants of one kernel body fall away), and every variant _keeps names"""
    seen, out = set(), []
    for env, case, expect in variants:
        if expect in seen and not _keeps(env):
            continue
        seen.add(expect)
        out.append((dict(env), case, dtype, expect, False))
    return out


def _group_case(c):
    M, N, K, sa, sb, sc, bs = c
    return (M, N, K, sa, sb, sc, [1, bs], [1, bs], [1, bs])


# (switches, case, data type, expected kernel-name prefix, lab build)
ENTRIES = _representatives(KV.VARIANTS, F64) + _representatives(KV.F32_VARIANTS, F32) + [
    # one wave per C block of at most 8 x 8: with the launch records and without, two prefetch depths
    ({}, SMALL.CASES["mix_1_to_8"], F64, "mm_numeric_f64_small<2>", False),
    ({"DBCSR_AMD_MM_SMALL": "4"}, SMALL.CASES["long_lists"], F64, "mm_numeric_f64_small<4>", False),
    ({"DBCSR_AMD_MM_SMALL": "2", "DBCSR_AMD_MM_WORK": "0"}, SMALL.CASES["7cube_tails"], F64, "mm_numeric_f64_small<2>", False),
    # the one-wave slab kernel and the workgroup-per-C-block kernel
    # (36cube_tails and 45x67x78 of that file with more block rows and columns: every zone gets several lines)
    ({}, (36 * 12 + 20, 36 * 12 + 7, 36 * 8 + 30, 0.4, 0.4, 0.5, [1, 36], [1, 36], [1, 36]), F64, BIGB.CASES["36cube_tails"][1], False),
    ({}, BIGB.CASES["mix_30_to_48"][0], F64, BIGB.CASES["mix_30_to_48"][1], False),
    ({}, BIGB.CASES["mixed_sizes"][0], F64, BIGB.CASES["mixed_sizes"][1], False),
    ({}, (45 * 13, 67 * 12, 78 * 5, 0.4, 0.4, 0.5, [1, 45], [1, 67], [1, 78]), F64, BIGB.CASES["45x67x78"][1], False),
    # complex_8 (cases of tests/test_gpu_complex_multiply.py: the mix of sizes, and 5 x 13 x 23 with more block rows and columns)
    ({}, (270, 250, 290, 0.4, 0.4, 0.6, [1, 13, 1, 23, 1, 32, 1, 40], [1, 13, 1, 23, 1, 32, 1, 40], [1, 13, 1, 23, 1, 32, 1, 40]), Z64, "mm_numeric_z64<4,4>", False),
    ({}, (5 * 14 + 1, 12 * 13 + 6, 4 * 23 + 3, 0.3, 0.3, 0.5, [1, 5], [1, 13], [1, 23]), Z64, "mm_numeric_z64<1,2>", False),
    # the lab's dataflows with record layouts of their own
    ({"DBCSR_AMD_MM_BAND": "2", "DBCSR_AMD_MM_BAND_SHAPE": "0"}, BAND.TAILS, F64, "mm_numeric_f64_band<23,23,23>", True),
    ({"DBCSR_AMD_MM_BAND": "2", "DBCSR_AMD_MM_BAND_SHAPE": "1"}, BAND.H2O, F64, "mm_numeric_f64_band<23,23,23>", True),
    ({"DBCSR_AMD_MM_TILE": "2", "DBCSR_AMD_MM_TILE_SHAPE": "0"}, TILE.TAILS, F64, "mm_numeric_f64_tile<23,23,23>", True),
    ({"DBCSR_AMD_MM_TILE": "2", "DBCSR_AMD_MM_TILE_SHAPE": "1"}, TILE.H2O, F64, "mm_numeric_f64_tile<23,23,23>", True),
    ({"DBCSR_AMD_MM_F32_GROUP": "4"}, _group_case(G32.CASES["edges32"]), F32, "mm_numeric_f32_group<32,32,32;4>", True),
    ({"DBCSR_AMD_MM_F32_GROUP": "3"}, _group_case(G32.CASES["cube16"]), F32, "mm_numeric_f32_group<16,16,16;3>", True),
    ({"DBCSR_AMD_MM_F64_GROUP": "4"}, _group_case(G64.CASES["edges23"]), F64, "mm_numeric_f64_group<23,23,23;4>", True),
    ({"DBCSR_AMD_MM_F64_GROUP": "3"}, _group_case(G64.CASES["cube16"]), F64, "mm_numeric_f64_group<16,16,16;3>", True),
]
ALPHA, BETA = 0.7, 1.3


def plans_of(i):
    return ASCENDING_PLANS if "_group<" in ENTRIES[i][3] else PLANS


def entry_id(i):
    env, case, dtype, expect, lab = ENTRIES[i]
    return "%02d-%s-%s" % (i, np.dtype(dtype).name, "-".join("%s=%s" % (k[13:], v) for k, v in sorted(env.items())) or "default")


def bcsr(M, data):
    return O.Bcsr(M.row_sizes, M.col_sizes, M.row_p, M.col_i, M.blk_p, data)


def typed(M, dtype, seed):
    """the oracle's float64 matrix in the case's data type; complex: uniform(-1, 1) imaginary parts laid over it"""
    if np.dtype(dtype).kind == "c":
        return bcsr(M, (M.data + 1j * np.random.default_rng(seed).uniform(-1.0, 1.0, M.data.size)).astype(dtype))
    return bcsr(M, M.data.astype(dtype))


def oracle_multiply(alpha, A, B, beta, Cm, **kw):
    """the oracle's multiply of the packed host matrices in float64 (complex: its four real multiplies); alpha and beta real, beta != 0"""
    if A.data.dtype.kind != "c":
        w = lambda M: bcsr(M, M.data.astype(np.float64))
        return O.multiply("N", "N", alpha, w(A), w(B), beta, w(Cm), **kw)
    re, im = (lambda M: bcsr(M, np.ascontiguousarray(M.data.real))), (lambda M: bcsr(M, np.ascontiguousarray(M.data.imag)))
    zero = bcsr(Cm, np.zeros(Cm.data.size))
    rr, info = O.multiply("N", "N", alpha, re(A), re(B), beta, re(Cm), **kw)
    ii, _ = O.multiply("N", "N", alpha, im(A), im(B), 1.0, zero, **kw)
    ri, _ = O.multiply("N", "N", alpha, re(A), im(B), beta, im(Cm), **kw)
    ir, _ = O.multiply("N", "N", alpha, im(A), re(B), 1.0, zero, **kw)
    assert all(np.array_equal(x.col_i, rr.col_i) and np.array_equal(x.blk_p, rr.blk_p) for x in (ii, ri, ir))
    return bcsr(rr, (rr.data - ii.data) + 1j * (ri.data + ir.data)), info


@functools.lru_cache(maxsize=None)
def operands(i):
    """(A, B, C_in) of entry i on the host, in its data type: computed once, never written"""
    env, case, dtype, expect, lab = ENTRIES[i]
    A, B, Cm = O.perf_case(*case)
    return typed(A, dtype, 1), typed(B, dtype, 2), typed(Cm, dtype, 3)


@functools.lru_cache(maxsize=None)
def reference(i):
    A, B, Cm = operands(i)
    return oracle_multiply(ALPHA, A, B, BETA, Cm)


def placements(A, B, Cm, dtype, plan, nbytes=FA.ARENA_LARGE):
    """far blk_p of (A, B, C_in) under one of PLANS"""
    wa, wb = (1, 0) if plan.endswith("_exchanged") else (0, 1)
    p = plan.split("_")[0]
    return (FA.place(A, dtype, p, wa, nbytes, lines="row"), FA.place(B, dtype, p, wb, nbytes, lines="col"), FA.place(Cm, dtype, p, 2, nbytes, lines="row"))


def values_err(out, ref):
    """rel_err of the project (gpu_util); complex: the modulus of the difference over the modulus of the reference"""
    if ref.data.dtype.kind == "c":
        return float(np.max(np.abs(out.data - ref.data) / np.maximum(np.abs(ref.data), 1e-300))) if ref.data.size else 0.0
    return rel_err(out.data, ref.data)


def same_index(out, ref):
    return np.array_equal(out.row_p, ref.row_p) and np.array_equal(out.col_i, ref.col_i)


def repacked(M):
    """the same matrix with its blocks in index order (mm_group.hip orders a result's blocks by its own rule)"""
    size = FA.block_sizes(M)
    blk_p = np.concatenate([[0], np.cumsum(size)[:-1]]).astype(np.int64) if len(size) else np.zeros(0, np.int64)
    if np.array_equal(blk_p, M.blk_p):
        return M
    data = np.concatenate([M.data[M.blk_p[b]:M.blk_p[b] + size[b]] for b in range(M.nblks)])
    return O.Bcsr(M.row_sizes, M.col_sizes, M.row_p, M.col_i, blk_p, data)


# ---- the arena: one per module ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def arena():
    torch.cuda.reset_peak_memory_stats()
    a = FA.arena()
    yield a
    if a is not None:
        print("far arena of %d bytes: torch.cuda.max_memory_allocated() over the arena %d bytes" % (a.nbytes, torch.cuda.max_memory_allocated() - a.nbytes))
        a.release()
        del a
    torch.cuda.empty_cache()


def view_of(arena, dtype):
    """the arena's view in the data type, or a skip that names the bytes missing"""
    if arena is None:
        pytest.skip("the device has less than %d bytes free: no far arena" % (FA.ARENA_SMALL + FA.MARGIN))
    if np.dtype(dtype).kind == "c" and arena.nbytes < FA.ARENA_LARGE:
        pytest.skip("complex128 offsets above 2^32 need the arena of %d bytes: %d bytes missing" % (FA.ARENA_LARGE, FA.ARENA_LARGE - arena.nbytes))
    return arena.view(dtype)


def far_operands(arena, mats, dtype, plan):
    """(Far, device matrices) of the host matrices under the plan"""
    view = view_of(arena, dtype)
    far = FA.Far(view)
    dev = [far.on_device(M, p) for M, p in zip(mats, placements(*mats, dtype, plan, arena.nbytes))]
    far.seal()
    return far, dev


# ---- 1. every multiply kernel family ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i,plan", [(i, plan) for i in range(len(ENTRIES)) for plan in plans_of(i)], ids=lambda v: entry_id(v) if isinstance(v, int) else v)
def test_multiply_with_far_operands(monkeypatch, arena, i, plan):
    env, case, dtype, expect, lab = ENTRIES[i]
    eng = KV.engine_for(monkeypatch, env, clear=CLEAR)
    if lab and not eng.lab:
        eng = MultiplyEngine(lab=True)
    A, B, Cm = operands(i)
    ref, info = reference(i)
    far, (dA, dB, dC) = far_operands(arena, (A, B, Cm), dtype, plan)
    flop = [0]
    dbcsr_multiply("N", "N", ALPHA, dA, dB, BETA, dC, flop=flop, engine=eng)
    torch.cuda.synchronize()
    name = eng.last_kernel()
    print("far operands up to high byte %d: %s" % (far.max_high_byte(), name))
    assert name.replace(" ", "").startswith(expect.replace(" ", "")), (name, expect)
    assert dC.data is not far.view and dC.packed, "the product is a packed matrix of its own"
    out = repacked(dev_to_bcsr(dC))
    assert same_index(out, ref)
    assert flop[0] == info["flop"]
    err = values_err(out, ref)
    print("rel_err %.3e against %.1e" % (err, TOL[np.dtype(dtype)]))
    assert err <= TOL[np.dtype(dtype)]
    assert far.guards_kept()


# ---- 2. around the kernels: transposes, stored triangles, crop, filter, checksum, plan reuse, limits -------------------------------------------------------
from tests import test_gpu_matrix_norms as MN   # noqa: E402  (the host helpers and check functions of the algebra's tests)
from tests import test_gpu_matrix_ops as MO     # noqa: E402
from tests import test_gpu_matvec as MV         # noqa: E402
from tests import test_gpu_multivec as MVV      # noqa: E402

DTYPES, IDS = [F64, F32, Z64], ["fp64", "fp32", "z64"]


@pytest.fixture
def eng(monkeypatch):
    return KV.engine_for(monkeypatch, {}, clear=CLEAR)


@functools.lru_cache(maxsize=None)
def square(dtype_name, symmetry="N"):
    """(A, B, C_in) on one square blocking of 200 rows in blocks of 13, 5 and 7; symmetry: A is a stored triangle"""
    dtype = np.dtype(dtype_name)
    sizes = O.make_block_sizes(200, [1, 13, 1, 5, 1, 7])
    A = O.make_random_matrix(sizes, sizes, 0.5, O.RANDMAT_SEED_INIT + 31) if symmetry == "N" else MN.symmetric_base(symmetry)
    B = O.make_random_matrix(sizes, sizes, 0.6, O.RANDMAT_SEED_INIT + 32)
    Cm = O.make_random_matrix(sizes, sizes, 0.7, O.RANDMAT_SEED_INIT + 33)
    assert np.array_equal(A.row_sizes, sizes)
    return typed(A, dtype, 1), typed(B, dtype, 2), typed(Cm, dtype, 3)


def real_part(M):
    return bcsr(M, np.ascontiguousarray(M.data.real, np.float64))


def check_against_dense(dC, R, ref_index, dtype):
    """the packed product on the device against the dense reference R on the oracle's pattern"""
    assert dC.packed
    got = dev_to_bcsr(dC)
    assert same_index(repacked(got), ref_index)
    G, mask = MN.dense(got), MN.pattern_mask(got)
    err = np.abs(G - R)[mask] / np.maximum(np.abs(R)[mask], 1e-300)
    print("rel_err %.3e against %.1e" % (float(err.max()), TOL[np.dtype(dtype)]))
    assert float(err.max()) <= TOL[np.dtype(dtype)]


def wide_dense(M):
    return MN.dense(M).astype(np.complex128 if M.data.dtype.kind == "c" else np.float64)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("plan", ["lines", "blocks"])
def test_transposed_far_operands(eng, arena, dtype, plan):
    """'T' (real) / 'C' (complex) of a far A and 'T' of a far B: the transposes read the far blocks"""
    A, B, Cm = square(np.dtype(dtype).name)
    ta = "C" if np.dtype(dtype).kind == "c" else "T"
    far, (dA, dB, dC) = far_operands(arena, (A, B, Cm), dtype, plan)
    dbcsr_multiply(ta, "T", ALPHA, dA, dB, BETA, dC, engine=eng)
    torch.cuda.synchronize()
    Ad, Bd = wide_dense(A), wide_dense(B)
    R = ALPHA * ((Ad.conj().T if ta == "C" else Ad.T) @ Bd.T) + BETA * wide_dense(Cm)
    ref, _ = O.multiply("T", "T", 1.0, real_part(A), real_part(B), 1.0, real_part(Cm))
    check_against_dense(dC, R, ref, dtype)
    assert far.guards_kept()


@pytest.mark.parametrize("dtype,symmetry", [(F64, "S"), (F32, "S"), (Z64, "H")], ids=["fp64_S", "fp32_S", "z64_H"])
@pytest.mark.parametrize("plan", ["lines", "blocks"])
def test_far_stored_triangle(eng, arena, dtype, symmetry, plan):
    """a far 'S' / 'H' operand: desymmetrized from its far blocks, and moved to its twins and back bit for bit"""
    A, B, Cm = square(np.dtype(dtype).name, symmetry)
    far, (dA, dB, dC) = far_operands(arena, (A, B, Cm), dtype, plan)
    dA.symmetry = symmetry
    dbcsr_multiply("N", "N", ALPHA, dA, dB, BETA, dC, engine=eng)
    torch.cuda.synchronize()
    R = ALPHA * (MN.desymmetrized_dense(A, symmetry).astype(wide_dense(A).dtype) @ wide_dense(B)) + BETA * wide_dense(Cm)
    ref, _ = O.multiply("N", "N", 1.0, O.desymmetrize(real_part(A), "S"), real_part(B), 1.0, real_part(Cm))
    check_against_dense(dC, R, ref, dtype)
    # stored triangle -> canonical form -> stored triangle: the blocks come back bit for bit, and the full matrix is the host's
    canon = eng.twin_moved(dA, 1, symmetry)
    back = eng.twin_moved(canon, 2, symmetry)
    full = eng.desymmetrized(dA)
    torch.cuda.synchronize()
    assert canon.packed and back.packed and full.packed
    hb = repacked(dev_to_bcsr(back))
    assert same_index(hb, A) and MN.same_bits(hb.data, A.data)
    assert MN.same_bits(MN.dense(dev_to_bcsr(full)), MN.desymmetrized_dense(A, symmetry).astype(dtype))
    assert far.guards_kept()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("plan", ["lines", "blocks"])
def test_crop_transpose_checksum_and_gather_of_a_far_matrix(eng, arena, dtype, plan):
    """cropped(far) and transposed(far) are the host blocks bit for bit; the checksum is that of the packed matrix"""
    A = square(np.dtype(dtype).name)[0]
    view = view_of(arena, dtype)
    far = FA.Far(view)
    dA = far.on_device(A, FA.place(A, dtype, plan, 0, arena.nbytes))
    far.seal()
    gathered = FA.blocks_to_host(dA)
    assert same_index(gathered, A) and MN.same_bits(gathered.data, A.data)
    packed = dev_to_bcsr(eng.cropped(dA))
    assert same_index(packed, A) and np.array_equal(packed.blk_p, A.blk_p) and MN.same_bits(packed.data, A.data)
    window = dev_to_bcsr(eng.cropped(dA, (20, 150), (33, 170)))
    want = dev_to_bcsr(eng.cropped(to_dev(A), (20, 150), (33, 170)))
    assert same_index(window, want) and MN.same_bits(window.data, want.data) and 0 < window.nblks < A.nblks
    for conj in (False, True):
        t = dev_to_bcsr(eng.transposed(dA, conjugate=conj))
        D = MN.dense(A)
        assert MN.same_bits(MN.dense(t), np.ascontiguousarray(D.conj().T if conj else D.T) + 0)   # (+ 0: the conjugate of a zero outside the blocks is -0)
    if np.dtype(dtype).kind != "c":   # (the checksum is offered for real data)
        cs_far, cs_packed = eng.checksum(dA), eng.checksum(to_dev(A))
        terms = MN.real_terms(A.data)
        print("checksum %r against %r" % (cs_far, cs_packed))
        MO.check_sum(cs_far[0], terms)
        # (the second sum: the same terms x ln|row col| >= 0 from the same kernel, added in another order -- each sum within (n - 1) u of the exact one)
        assert abs(cs_far[1] - cs_packed[1]) <= 2 * (A.data.size + 4) * MN.U53 * abs(cs_packed[1])
    assert far.guards_kept()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("plan", ["lines", "blocks"])
def test_filter_of_a_far_matrix(eng, arena, dtype, plan):
    """filtered(far, eps), as a packed copy and in place: the kept set is the host's, the kept blocks are the host's bit for bit"""
    A = square(np.dtype(dtype).name)[0]
    blocks = {k: (v * 1e-9).astype(dtype) if (k[0] + 2 * k[1]) % 3 == 0 else v for k, v in MN.blocks_of(A).items()}
    M = MN.from_blocks(A.row_sizes, A.col_sizes, blocks, dtype)
    eps = 1e-6
    kept = {k: v for k, v in blocks.items() if float(np.sum(MN.real_terms(v))) >= eps * eps}
    assert 0 < len(kept) < len(blocks)
    want = MN.from_blocks(A.row_sizes, A.col_sizes, kept, dtype)
    view = view_of(arena, dtype)
    far = FA.Far(view)
    dM = far.on_device(M, FA.place(M, dtype, plan, 1, arena.nbytes))
    far.seal()
    copy = eng.filtered(dM, eps)
    torch.cuda.synchronize()
    assert copy.packed and copy.data is not view
    got = dev_to_bcsr(copy)
    assert same_index(got, want) and MN.same_bits(repacked(got).data, want.data)
    inpl = eng.filtered(dM, eps, in_place=True)
    torch.cuda.synchronize()
    assert inpl.data is view and inpl.nze == want.data.size and inpl.nblks == want.nblks
    got = FA.blocks_to_host(inpl)
    assert same_index(got, want) and MN.same_bits(got.data, want.data)
    far_p = dict(zip(zip(M.rows().tolist(), M.col_i.tolist()), dM.blk_p.cpu().tolist()))
    assert inpl.blk_p.cpu().tolist() == [far_p[k] for k in sorted(kept)], "the kept blocks stay where they are"
    assert far.guards_kept()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_second_multiply_on_far_operands_reuses_its_plan(monkeypatch, arena, dtype):
    monkeypatch.delenv("DBCSR_AMD_MM_PLAN", raising=False)
    eng = KV.engine_for(monkeypatch, {}, clear=CLEAR)
    A, B, Cm = square(np.dtype(dtype).name)
    far, (dA, dB, dC0) = far_operands(arena, (A, B, Cm), dtype, "blocks")
    R = ALPHA * (wide_dense(A) @ wide_dense(B)) + BETA * wide_dense(Cm)
    ref, _ = O.multiply("N", "N", 1.0, real_part(A), real_part(B), 1.0, real_part(Cm))
    for it in range(2):
        dC = DbcsrMatrix(dC0.row_blk_size, dC0.col_blk_size, dC0.row_p, dC0.col_i, dC0.blk_p, dC0.data, nze=dC0.nze)
        dbcsr_multiply("N", "N", ALPHA, dA, dB, BETA, dC, engine=eng)
        torch.cuda.synchronize()
        assert eng.plan_stats() == (it, 1)
        check_against_dense(dC, R, ref, dtype)
    assert far.guards_kept()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_limits_on_far_operands(eng, arena, dtype):
    """row, column and k limits once (beta = 1: the window of C_in is not scaled, so nothing copies C_in's data area)"""
    A, B, Cm = square(np.dtype(dtype).name)
    far, (dA, dB, dC) = far_operands(arena, (A, B, Cm), dtype, "blocks")
    fr, lr, fc, lc, fk, lk = 21, 150, 34, 171, 9, 160   # 1-based, inclusive
    dbcsr_multiply("N", "N", ALPHA, dA, dB, 1.0, dC, first_row=fr, last_row=lr, first_column=fc, last_column=lc, first_k=fk, last_k=lk, engine=eng)
    torch.cuda.synchronize()
    Ad, Bd = wide_dense(A), wide_dense(B)
    R = wide_dense(Cm)
    R[fr - 1:lr, fc - 1:lc] += ALPHA * (Ad[fr - 1:lr, fk - 1:lk] @ Bd[fk - 1:lk, fc - 1:lc])
    ref, _ = O.multiply_limits("N", "N", 1.0, real_part(A), real_part(B), 1.0, real_part(Cm), (fr, lr, fc, lc, fk, lk))
    check_against_dense(dC, R, ref, dtype)
    assert far.guards_kept()


# ---- 3. the algebra on far matrices ------------------------------------------------------------------------------------------------------------------------
def one_far(arena, M, dtype, plan, who=0, symmetry="N"):
    far = FA.Far(view_of(arena, dtype))
    dM = far.on_device(M, FA.place(M, dtype, plan, who, arena.nbytes), symmetry=symmetry)
    far.seal()
    return far, dM


@pytest.fixture
def gather_by_blocks(monkeypatch):
    """the check functions of the algebra's tests read a device matrix back through blocks_to_host: never the whole arena"""
    for mod in (MN, MO):
        monkeypatch.setattr(mod, "dev_to_bcsr", FA.blocks_to_host)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("plan", ["lines", "blocks"])
def test_sums_and_norms_of_a_far_matrix(eng, arena, dtype, plan):
    M = MN.typed(MN.base("mixed"), dtype, 1)
    far, dM = one_far(arena, M, dtype, plan)
    MN.check_everything_read_only(eng, M, dM)
    assert far.guards_kept()


@pytest.mark.parametrize("dtype,symmetry", [(F64, "S"), (F32, "S"), (Z64, "H")], ids=["fp64_S", "fp32_S", "z64_H"])
def test_gershgorin_and_products_of_a_far_stored_triangle(eng, arena, dtype, symmetry):
    X = MN.typed(MN.symmetric_base(symmetry), dtype, 3)
    far, dX = one_far(arena, X, dtype, "blocks", who=1)
    MN.check_everything_read_only(eng, X, dX, symmetry)
    parts = MV.dense_parts(X, symmetry)
    MV.check_product(eng, X, dX, parts, symmetry, "N")
    MVV.check_product(eng, X, dX, parts, symmetry, "N", 17, view=True)
    assert far.guards_kept()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("plan", ["lines", "blocks"])
def test_matvec_and_multivec_of_a_far_matrix(eng, arena, dtype, plan):
    M, *parts = MV.host_matrix("mixed", np.dtype(dtype).name, "N")
    far, dM = one_far(arena, M, dtype, plan)
    for trans in ("N", "T") + (("C",) if np.dtype(dtype).kind == "c" else ()):
        MV.check_product(eng, M, dM, tuple(parts), "N", trans)
        MVV.check_product(eng, M, dM, tuple(parts), "N", trans, 17, view=True)
    assert far.guards_kept()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_diag_of_a_far_matrix(eng, arena, dtype):
    """check_diag of tests/test_gpu_matrix_norms.py with the data area read block by block: get_diag bit for bit, set_diag writes the diagonal elements
    of the diagonal blocks present and nothing else -- no other element of a block, no guard"""
    M = repacked(MN.typed(MN.base("square"), dtype, 1))
    far, dM = one_far(arena, M, dtype, "blocks")
    n = MN.full_len(M.row_sizes)
    got = dbcsr_get_diag(dM, engine=eng).cpu().numpy()
    assert MN.same_bits(got, np.ascontiguousarray(np.diagonal(MN.dense(M))).astype(dtype))
    at, idx = MN.diagonal_places(M)
    assert at.size and at.size < n
    v = MN.random_vector(n, dtype, 4)
    before = (dM.index_stamp(), dM.row_p, dM.col_i, dM.blk_p, dM.data)
    dbcsr_set_diag(dM, torch.as_tensor(v).cuda(), engine=eng)
    torch.cuda.synchronize()
    assert dM.index_stamp() == before[0] and dM.row_p is before[1] and dM.col_i is before[2] and dM.blk_p is before[3] and dM.data is before[4]
    area = M.data.copy()
    area[at] = v[idx]
    assert MN.same_bits(FA.blocks_to_host(dM).data, area), "the diagonal elements are the vector's, every other element of the blocks is unchanged"
    want = np.zeros(n, dtype)
    want[idx] = v[idx]
    assert MN.same_bits(dbcsr_get_diag(dM, engine=eng).cpu().numpy(), want)
    assert far.guards_kept()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_scale_by_vector_of_a_far_matrix(eng, arena, dtype):
    """check_scale_by_vector of tests/test_gpu_matrix_norms.py with the data area read block by block, and the guards"""
    M = repacked(MN.typed(MN.base("mixed"), dtype, 1))
    far, dM = one_far(arena, M, dtype, "blocks", who=1)
    cur = M
    stamp = dM.index_stamp()
    for side, sizes, seed in (("right", M.col_sizes, 5), ("left", M.row_sizes, 6)):
        v = MN.random_vector(MN.full_len(sizes), dtype, seed)
        ref, scale = MN.scaled_area(cur, v, side)
        dbcsr_scale_by_vector(dM, torch.as_tensor(v).cuda(), side, engine=eng)
        torch.cuda.synchronize()
        got = FA.blocks_to_host(dM).data
        if MN.is_complex(dtype):
            assert np.all(np.abs(got - ref) <= 4 * MN.U53 * scale)
        else:
            assert MN.same_bits(got, ref), side
        cur = bcsr(M, got.copy())
    assert dM.index_stamp() == stamp and far.guards_kept()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_add_scale_and_reductions_of_far_matrices(eng, arena, gather_by_blocks, dtype):
    """the add / scale / trace / dot / norm checks of tests/test_gpu_matrix_ops.py on far operands"""
    X, Y = (repacked(M) for M in MO.square_pair(dtype))
    view = view_of(arena, dtype)
    far = FA.Far(view)
    dX = far.on_device(X, FA.place(X, dtype, "blocks", 0, arena.nbytes))
    dY = far.on_device(Y, FA.place(Y, dtype, "blocks", 1, arena.nbytes))
    far.seal()
    MO.check_trace(eng, dX, X)
    MO.check_norm(eng, dX, MO.real_terms(X.data))
    if np.dtype(dtype).kind != "c":
        bx, by = MO.blocks_of(X), MO.blocks_of(Y)
        terms = np.concatenate([bx[k].astype(np.float64) * by[k].astype(np.float64) for k in sorted(set(bx) & set(by))])
        MO.check_sum(dbcsr_dot(dX, dY, engine=eng), terms)
    # scale in place: the blocks within the bar of tests/test_gpu_matrix_ops.py::test_scale, the index and the guards as they were
    stamp = dX.index_stamp()
    al = MO.scalars(dtype)[1]
    dbcsr_scale(dX, al, engine=eng)
    torch.cuda.synchronize()
    got = FA.blocks_to_host(dX)
    assert same_index(got, X) and dX.index_stamp() == stamp and dX.data is view
    assert np.all(np.abs(got.data - MO.times(al, X.data, dtype)) <= 2 * MO.factor(dtype) * MO.unit(dtype) * abs(al) * np.abs(X.data))
    assert far.guards_kept()
    # add of independent patterns: far operands, a packed result (the far blocks of X hold the scaled values now)
    a2, b2 = MO.scalars(dtype)
    MO.check_add(eng, bcsr(X, got.data), Y, a2, b2, dA=dX, dB=dY)
    assert dX.data is not view and far.guards_kept()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_flat_add_in_a_far_data_area(eng, arena, dtype):
    """the flat in-place add needs a packed A: here its data area (and B's) starts above element 2^32 of the arena, between guards"""
    A = MO.typed(MO.base_pair()[0], dtype, 1)
    B = bcsr(A, MO.typed(MO.base_pair()[0], dtype, 3).data[::-1].copy())
    view = view_of(arena, dtype)
    n, G = A.data.size, FA.GUARD
    base = FA.TWO32 + 12345
    spots = [base + G, base + 3 * G + n]
    view[base:base + 4 * G + 2 * n].fill_(FA.CANARY)
    mats = []
    for M, s in zip((A, B), spots):
        d = to_dev(M)
        view[s:s + n].copy_(d.data)
        mats.append(DbcsrMatrix(d.row_blk_size, d.col_blk_size, d.row_p, d.col_i, d.blk_p, view[s:s + n]))
    al, be = MO.scalars(dtype)
    assert dbcsr_add(mats[0], mats[1], al, be, engine=eng) is True
    torch.cuda.synchronize()
    area = view[base:base + 4 * G + 2 * n].cpu().numpy()
    ref, scale = MO.reference_add(A, B, al, be)
    got = area[G:G + n]
    assert np.all(np.abs(got - ref.data) <= 4 * MO.factor(dtype) * MO.unit(dtype) * scale)
    assert MN.same_bits(area[3 * G + n:3 * G + 2 * n], B.data), "B is only read"
    guards = np.concatenate([area[:G], area[G + n:3 * G + n], area[3 * G + 2 * n:]])
    assert MN.same_bits(guards, np.full(guards.shape, FA.CANARY, guards.dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("diag", ["all", "some"])
def test_add_on_diag_of_a_far_matrix(eng, arena, gather_by_blocks, dtype, diag):
    """every diagonal block present: in place in the far blocks; some missing: they come in through dbcsr_add and the result is packed"""
    X = MO.square_pair(dtype)[0]
    blocks = {k: v for k, v in MO.blocks_of(X).items() if k[0] != k[1] or diag == "all" or k[0] % 2}
    if diag == "all":
        rng = np.random.default_rng(9)
        for r in range(X.nbr):
            blocks.setdefault((r, r), rng.uniform(-1, 1, int(X.row_sizes[r]) ** 2).astype(dtype))
    A = MO.from_blocks(X.row_sizes, X.col_sizes, blocks, dtype)
    far, dA = one_far(arena, A, dtype, "blocks")
    alpha = (1.5 - 0.5j) if np.dtype(dtype).kind == "c" else -1.5
    stamp = dA.index_stamp()
    dbcsr_add_on_diag(dA, alpha, engine=eng)
    torch.cuda.synchronize()
    assert (dA.data is far.view and dA.index_stamp() == stamp) if diag == "all" else dA.packed
    got = FA.blocks_to_host(dA)
    u4 = 4 * MO.factor(dtype) * MO.unit(dtype)
    seen = 0
    for (r, c), v in MO.blocks_of(got).items():
        if r != c:
            assert MN.same_bits(v, blocks[(r, c)])
            continue
        m = int(A.row_sizes[r])
        on = np.arange(m) * (m + 1)
        old = blocks.get((r, r), np.zeros(m * m, dtype))
        off = np.ones(m * m, bool)
        off[on] = False
        assert MN.same_bits(v[off], old[off])
        assert np.all(np.abs(v[on] - (old[on] + np.asarray(alpha, dtype)).astype(dtype)) <= u4 * (np.abs(old[on]) + abs(alpha)))
        seen += 1
    assert seen == A.nbr and far.guards_kept()


# ---- 4. the acc ABI: stack offsets up to 2^31 - 1 ----------------------------------------------------------------------------------------------------------
def acc_sites(sizes):
    """0-based element offsets for the blocks of a, b and c (sizes: elements per block of each) at three sites of the arena: behind its start, around
    element 2^29 (for float64 byte offset 2^32; one block of each straddles a multiple of 2^28 there), and below element 2^31 - 1, where the topmost
    block -- one of c -- ends exactly.  Returns ([offsets of a, of b, of c], guard windows)."""
    G = FA.GUARD
    offs, guards = [[], [], []], []
    per = [(len(s) + 2) // 3 for s in sizes]

    def lay(at, which, lo, hi):
        guards.append((at - G, at))
        for blk in range(lo, min(hi, len(sizes[which]))):
            offs[which].append(at)
            at += sizes[which][blk]
        guards.append((at, at + G))
        return at + G

    at = G
    for w in range(3):                                    # site 0: the arena's start
        at = lay(at, w, 0, per[w]) + G + 1
    at = 2 ** 29 - sum(sizes[0][per[0]:per[0] + 2]) - sizes[0][per[0] + 2] // 2    # site 1: a's third block here straddles 2^29
    for w in range(3):
        at = lay(at, w, per[w], 2 * per[w]) + G + 1
    top = 2 ** 31 - 1                                      # site 2: c topmost, then b, then a below it
    for w in (2, 1, 0):
        n = sum(sizes[w][2 * per[w]:])
        lay(top - n, w, 2 * per[w], len(sizes[w]))
        top -= n + 2 * G + 1
    iv = guards + [(o, o + z) for w in range(3) for o, z in zip(offs[w], sizes[w])]
    assert all(len(offs[w]) == len(sizes[w]) for w in range(3))
    return offs, guards, iv


@pytest.mark.parametrize("dtype,m,n,k,nstack,kernel", [
    (F64, 23, 23, 23, 300, "smm_stack_f64_exact<23,23,23"),   # a homogeneous stack of 256 entries or more: the kernel compiled at run time
    (F64, 22, 21, 19, 100, "smm_stack_f64_lds(22,21,19"),      # a short one of a triplet no other test compiles a kernel for: the generic stack kernel
    (F64, 13, 5, 7, 200, "smm_stack_f64_lds(13,5,7"),
    (F32, 23, 23, 23, 300, None),                              # (the float32 stack kernels record no name)
    (F32, 13, 23, 7, 200, None),
], ids=["fp64_exact23", "fp64_generic_22x21x19", "fp64_generic_13x5x7", "fp32_23", "fp32_13x23x7"])
def test_acc_stacks_with_offsets_up_to_the_last_element_a_stack_can_name(arena, dtype, m, n, k, nstack, kernel):
    view = view_of(arena, dtype)
    lib = L.load_library()
    na, nb, nc = 60, 60, 12
    rng = np.random.default_rng(m + 100 * n + 10000 * k + nstack)
    sizes = [[m * k] * na, [k * n] * nb, [m * n] * nc]
    offs, guards, iv = acc_sites(sizes)
    assert not FA.overlaps(iv)
    host = [[rng.random(z).astype(dtype) for z in sizes[w]] for w in range(3)]
    for s, e in guards:
        view[s:e].fill_(FA.CANARY)
    for w in range(3):
        for o, blk in zip(offs[w], host[w]):
            view[o:o + blk.size].copy_(torch.from_numpy(blk))
    ia, ib = rng.integers(0, na, nstack), rng.integers(0, nb, nstack)
    ic = np.sort(rng.integers(0, nc, nstack))
    ia[:3], ib[:3], ic[-1] = [na - 1, 0, na // 3 + 2], [nb - 1, 0, nb // 3], nc - 1    # the topmost, the first and the straddling blocks take part
    stack = np.empty(3 * nstack, np.int32)
    stack[0::3], stack[1::3], stack[2::3] = np.asarray(offs[0])[ia] + 1, np.asarray(offs[1])[ib] + 1, np.asarray(offs[2])[ic] + 1   # 1-based by the ABI
    assert int(stack[2::3].max()) + m * n - 1 == 2 ** 31 - 1
    # B transposed in place by libsmm_acc_transpose (float64; 0-based offsets), as the host does before it hands the stack over
    st = StreamHandle()
    bt = np.dtype(dtype) == np.float64
    if bt:
        trs = torch.as_tensor(np.asarray(offs[1], np.int32)).cuda()
        assert lib.libsmm_acc_transpose(trs.data_ptr(), 0, nb, view.data_ptr(), L.dbcsr_type_real_8, k, n, 80, st.ptr) == 0
        torch.cuda.synchronize()
        for o, blk in zip(offs[1], host[1]):
            assert MN.same_bits(view[o:o + k * n].cpu().numpy(), np.ascontiguousarray(blk.reshape(n, k).T).reshape(-1)), "libsmm_acc_transpose of a far block"
    tstack = torch.as_tensor(stack).cuda()
    code = L.dbcsr_type_real_8 if bt else L.dbcsr_type_real_4
    rc = lib.libsmm_acc_process(None, tstack.data_ptr(), nstack, code, view.data_ptr(), view.data_ptr(), view.data_ptr(), m, n, k, 80 if bt else 0, 1, st.ptr, st.ptr)
    torch.cuda.synchronize()
    assert rc >= 0
    if kernel is not None:
        name = lib.dbcsr_amd_smm_last_kernel().decode()
        print("acc stack with offsets up to 2^31 - 1: %s" % name)
        assert name.startswith(kernel), name
    # the reference: numpy long double, entry by entry
    ref = [blk.astype(np.longdouble) for blk in host[2]]
    for e in range(nstack):
        Ab = host[0][ia[e]].astype(np.longdouble).reshape(k, m).T
        Bb = host[1][ib[e]].astype(np.longdouble).reshape(n, k).T
        ref[ic[e]] += (Ab @ Bb).T.reshape(-1)
    got = np.concatenate([view[o:o + m * n].cpu().numpy() for o in offs[2]])
    ref = np.concatenate(ref)
    if bt:
        err = float(np.max(np.abs(got - ref) / np.abs(ref)))
        print("rel_err %.3e against 1e-10" % err)
        assert err <= 1e-10
    else:
        err = float(np.max(np.abs(got - ref)))
        print("max error %.3e against %.3e" % (err, 2e-5 * float(np.max(np.abs(ref)))))
        assert err <= 2e-5 * float(np.max(np.abs(ref)))
    for w in (0, 1):
        for o, blk in zip(offs[w], host[w]):
            if w == 0 or not bt:
                assert MN.same_bits(view[o:o + blk.size].cpu().numpy(), blk), "a and b are only read"
    g = torch.cat([view[s:e] for s, e in guards]).cpu().numpy()
    assert MN.same_bits(g, np.full(g.shape, FA.CANARY, g.dtype))
