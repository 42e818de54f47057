"""What the element-wise operations' tests rest on, checked without a GPU: the host reference (tests/elementwise_ref.py) against dense numpy, the
properties tests/test_gpu_elementwise.py relies on in its seeded inputs, the argument errors of dbcsr_hadamard_product / dbcsr_copy /
dbcsr_function_of_elements (raised before anything touches a device), and the C entries in the library."""
import ctypes

import numpy as np
import pytest
import torch

import dbcsr_amd
from dbcsr_amd import lib as L
from dbcsr_amd import operations as OPS
from dbcsr_amd.matrix import DbcsrMatrix
from tests import elementwise_ref as R

PAIRS = {"mixed": R.mixed_pair, "tiny": R.tiny_pair}


def pattern(M):
    """1 where the full matrix has an element of a stored block"""
    return R.dense(R.with_data(M, np.ones(M.data.size))) != 0


# ---- the reference against dense numpy --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.IDS)
@pytest.mark.parametrize("which", sorted(PAIRS))
def test_reference_hadamard_is_the_dense_product_on_the_intersection(which, dtype):
    A, B = (R.typed(M, dtype, 1 + i) for i, M in enumerate(PAIRS[which]()))
    ref, scale = R.reference_hadamard(A, B)
    both = pattern(A) & pattern(B)
    assert np.array_equal(pattern(ref), both)
    assert np.array_equal(R.dense(ref), np.where(both, R.dense(A) * R.dense(B), 0).astype(dtype))
    assert np.array_equal(R.dense(R.with_data(ref, scale)), np.where(both, np.abs(R.dense(A)) * np.abs(R.dense(B)), 0))
    # packed, sorted
    assert np.array_equal(ref.blk_p, np.concatenate([[0], np.cumsum(R.sizes_of(ref))[:-1]]))
    assert all(np.all(np.diff(ref.col_i[ref.row_p[r]:ref.row_p[r + 1]]) > 0) for r in range(ref.nbr))
    # an assumed value: A's pattern, B's missing elements taken as the value
    v = 0.5 - 2j if np.dtype(dtype).kind == "c" else -0.5
    ref, _ = R.reference_hadamard(A, B, v)
    filled = np.where(pattern(B), R.dense(B), np.asarray(v, dtype))
    assert np.array_equal(pattern(ref), pattern(A)) and np.array_equal(R.dense(ref), np.where(pattern(A), R.dense(A) * filled, 0).astype(dtype))
    one, _ = R.reference_hadamard(A, B, 1)
    ba, bb, bo = R.blocks_of(A), R.blocks_of(B), R.blocks_of(one)
    assert all(R.same_bits(bo[k], ba[k]) for k in ba if k not in bb)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.IDS)
def test_reference_copy_onto_is_the_dense_matrix_on_the_pattern(dtype):
    A, B = (R.typed(M, dtype, 1 + i) for i, M in enumerate(R.mixed_pair()))
    hB = R.with_holes(B)
    got = R.with_data(hB, R.reference_copy_onto(R.with_holes(A), hB))
    assert np.array_equal(R.dense(got), np.where(pattern(B), R.dense(A), 0))
    mask = R.named_mask(hB)
    assert R.same_bits(got.data[~mask], hB.data[~mask]) and np.all(hB.data[~mask] == R.CANARY)
    assert not np.signbit(got.data[mask].real).any() or (R.dense(A) < 0).any()


def test_reference_functions_against_float64_numpy():
    x = np.linspace(-0.8, 0.8, 41)
    a0, a1 = 0.25, -0.5
    y = a1 * x + a0
    t = np.tanh(y)
    want = {"inverse": 1 / y, "tanh": t, "dtanh": a1 * (1 - t * t), "ddtanh": -2 * a1 * a1 * t * (1 - t * t), "artanh": np.arctanh(y), "sin": np.sin(y),
            "dsin": a1 * np.cos(y), "ddsin": -a1 * a1 * np.sin(y), "asin": np.arcsin(y), "cos": np.cos(y), "dcos": -a1 * np.sin(y),
            "ddcos": -a1 * a1 * np.cos(y)}
    assert sorted(want) == sorted(R.FUNC_NAMES)
    h = 1e-6
    for name in R.FUNC_NAMES:
        f, df = R.reference_function(name, x, a0, a1)
        assert f.dtype == np.longdouble
        assert np.allclose(np.asarray(f, np.float64), want[name], rtol=1e-13, atol=0), name
        # the derivative by y: a central difference of the value (x moves by h / a1)
        up, dn = R.reference_function(name, x + h / a1, a0, a1)[0], R.reference_function(name, x - h / a1, a0, a1)[0]
        assert np.allclose(np.asarray((up - dn) / (2 * h), np.float64), np.asarray(df, np.float64), rtol=1e-6, atol=1e-9), name
        excess, ref = R.function_errors(name, x, a0, a1, want[name])
        assert ref.dtype == np.float64 and excess.max() <= 8, "numpy's own float64 result lies within a few units of the reference"


# ---- what the GPU test relies on in its inputs ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", sorted(PAIRS))
def test_seeded_pairs_populate_every_case(which):
    A, B = PAIRS[which]()
    ka, kb = set(R.blocks_of(A)), set(R.blocks_of(B))
    assert ka & kb and ka - kb and kb - ka, "intersection, A-only and B-only"
    assert np.array_equal(A.row_sizes, B.row_sizes) and np.array_equal(A.col_sizes, B.col_sizes)
    for M in (A, B):
        assert all(np.all(np.diff(M.col_i[M.row_p[r]:M.row_p[r + 1]]) > 0) for r in range(M.nbr)), "ascending block columns"
        assert M.data.min() >= 0.0 and M.data.max() < 1.0
    if which == "mixed":
        assert A.nbr > 1 and (A.row_sizes.max(), A.col_sizes.max()) == (13, 23)
    else:
        assert A.nbc == 76 and np.diff(A.row_p).max() > 64 and np.diff(B.row_p).max() > 64, "rows of more than 64 blocks"
    for dtype in R.DTYPES:
        for M in (A, R.with_holes(A)):
            assert ((M.blk_p * np.dtype(dtype).itemsize) % 16 != 0).any() or np.dtype(dtype).itemsize == 16, "a block that starts off a 16-byte boundary"


def test_edge_patterns_are_what_their_names_say():
    for name in R.EDGE_PATTERNS:
        A, B = R.edge_pair(name, np.float64)
        assert set(R.blocks_of(A)) == set(R.EDGE_PATTERNS[name][0]) and set(R.blocks_of(B)) == set(R.EDGE_PATTERNS[name][1])
    ka, kb = R.EDGE_PATTERNS["disjoint"]
    assert ka and kb and not ka & kb
    ka, kb = R.EDGE_PATTERNS["rows"]
    row = lambda keys, r: sorted(c for rr, c in keys if rr == r)
    assert row(ka, 1) and not row(kb, 1), "a row where A has blocks and B none"
    assert row(kb, 3) and not row(ka, 3), "and the reverse"
    assert [c for c in row(ka, 0) if c in row(kb, 0)] == [row(kb, 0)[0]], "the partner is the first block of B's row"
    assert [c for c in row(ka, 2) if c in row(kb, 2)] == [row(kb, 2)[-1]], "the partner is the last block of B's row"
    assert R.EDGE_PATTERNS["a_empty"][0] == frozenset() and R.EDGE_PATTERNS["b_empty"][1] == frozenset()


def test_matrix_with_holes_has_gaps_and_odd_offsets():
    A = R.mixed_pair()[0]
    H = R.with_holes(A)
    mask = R.named_mask(H)
    assert mask.sum() == A.data.size and not mask.all() and np.all(H.data[~mask] == R.CANARY)
    assert (H.blk_p % 2 == 1).any() and (H.blk_p % 2 == 0).any() and (H.blk_p % 4 == 3).any()
    assert all(R.same_bits(x, y) for x, y in zip(R.blocks_of(H).values(), R.blocks_of(A).values()))


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("a0,a1", R.PARAMS)
@pytest.mark.parametrize("name", R.FUNC_NAMES)
def test_function_inputs_keep_their_ranges(name, a0, a1, dtype):
    for M in (R.mixed_pair()[0], R.tiny_pair()[0]):
        X = R.function_input(M, name, a0, a1, dtype)
        assert X.data.dtype == dtype
        y = np.asarray(R.y_of(X.data, a0, a1), np.float64)
        lo, hi = R.y_range(name)
        assert np.abs(y).min() >= lo and np.abs(y).max() <= hi
        assert (y > 0).any() and (y < 0).any() and np.abs(y).max() >= 0.8 * hi


# ---- argument errors, without a device ---------------------------------------------------------------------------------------------------------------------
class NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("the library was about to be called (%s)" % name)


def host_matrix(M, symmetry="N"):
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt)
    return DbcsrMatrix(t(M.row_sizes, torch.int32), t(M.col_sizes, torch.int32), t(M.row_p, torch.int32), t(M.col_i, torch.int32), t(M.blk_p, torch.int64),
                       torch.as_tensor(M.data), symmetry=symmetry)


def test_argument_errors_raise_without_a_device():
    A, B = R.mixed_pair()
    no = NoLibrary()
    a, b = host_matrix(A), host_matrix(B)
    f32, tiny, s = host_matrix(R.typed(A, np.float32)), host_matrix(R.tiny_pair()[0]), host_matrix(B, "S")
    for other, error in ((f32, TypeError), (tiny, ValueError), (s, ValueError)):
        with pytest.raises(error):
            OPS.dbcsr_hadamard_product(a, other, host_matrix(A), engine=no)
        with pytest.raises(error):
            OPS.dbcsr_hadamard_product(a, b, other, engine=no)
        with pytest.raises(error):
            OPS.dbcsr_copy(other, a, keep_sparsity=True, engine=no)
    for sym in ("A", "K"):
        with pytest.raises(ValueError):
            OPS.dbcsr_hadamard_product(host_matrix(A, sym), host_matrix(B, sym), host_matrix(A, sym), engine=no)
    with pytest.raises(ValueError):
        OPS.dbcsr_hadamard_product(host_matrix(A, "X"), host_matrix(B, "X"), host_matrix(A, "X"), engine=no)
    with pytest.raises(TypeError):
        OPS.dbcsr_hadamard_product(a, b, host_matrix(A), b_assume_value=2j, engine=no)
    with pytest.raises(ValueError):
        OPS.dbcsr_copy(a, a, keep_sparsity=True, engine=no)
    view = DbcsrMatrix(a.row_blk_size, a.col_blk_size, b.row_p, b.col_i, b.blk_p, a.data[8:])
    with pytest.raises(ValueError):
        OPS.dbcsr_copy(view, a, keep_sparsity=True, engine=no)
    with pytest.raises(TypeError):
        OPS.dbcsr_copy(f32, a, engine=no)
    z = host_matrix(R.typed(A, np.complex128))
    for func in (5, 6, 14, 99, -1, True, 1.0, "tanh", None):
        with pytest.raises(NotImplementedError):
            OPS.dbcsr_function_of_elements(a, func, engine=no)
    with pytest.raises(NotImplementedError):
        OPS.dbcsr_function_of_elements(a, OPS.dbcsr_func_sin, a2=0.5, engine=no)
    with pytest.raises(NotImplementedError):
        OPS.dbcsr_function_of_elements(z, OPS.dbcsr_func_sin, engine=no)


def test_function_codes_and_exports():
    codes = {name: getattr(dbcsr_amd, "dbcsr_func_" + name) for name in R.FUNC_NAMES}
    assert codes == {"inverse": 0, "tanh": 1, "dtanh": 2, "ddtanh": 3, "artanh": 4, "sin": 7, "dsin": 8, "ddsin": 9, "asin": 10, "cos": 11, "dcos": 12,
                     "ddcos": 13}
    for name in ("dbcsr_hadamard_product", "dbcsr_copy", "dbcsr_function_of_elements"):
        assert name in dbcsr_amd.__all__ and getattr(dbcsr_amd, name) is getattr(OPS, name) and name in OPS.__doc__


def test_c_entries_are_exported():
    lib = ctypes.CDLL(L.library_path())
    for name in ("dbcsr_amd_bcsr_hadamard_count", "dbcsr_amd_bcsr_hadamard_apply", "dbcsr_amd_bcsr_copy_onto", "dbcsr_amd_bcsr_function_of_elements"):
        assert name in L.MM_SYMBOLS and hasattr(lib, name)
    loaded = L.load_library()
    assert len(loaded.dbcsr_amd_bcsr_hadamard_count.argtypes) == 9 and len(loaded.dbcsr_amd_bcsr_hadamard_apply.argtypes) == 7
    assert len(loaded.dbcsr_amd_bcsr_copy_onto.argtypes) == 5 and len(loaded.dbcsr_amd_bcsr_function_of_elements.argtypes) == 7
