"""The conditions on the inputs of tests/test_gpu_special_values.py, on the oracle alone (no GPU): what makes the oracle's classes the reference for
every summation order (tests/special_values.py: the class rule), and what makes each case mean something -- enough C blocks reached and not too
many, all four classes in C, a column of C that is Inf in every element (the 0 x Inf of a padded tail k step would make it NaN), blocks that hold NaN
and no Inf, filter cases that drop blocks and keep every NaN block, scaled results that stay normal numbers.  These are conditions, not measurements."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import special_values as SV

N = len(SV.entries())


def parts(x):
    x = np.asarray(x)
    return np.concatenate([x.real, x.imag]) if x.dtype.kind == "c" else x


def test_classes_and_assert_same_on_hand_made_data():
    x = np.array([1.0, np.inf, -np.inf, np.nan, -0.0, 1e308])
    assert SV.classes(x).tolist() == [0, 1, 2, 3, 0, 0]
    z = np.array([complex(np.inf, 1.0), complex(2.0, np.nan), complex(-np.inf, -np.inf)])
    assert SV.classes(z).tolist() == [[1, 0], [0, 3], [2, 2]]
    M = O.Bcsr([2], [3], [0, 1], [0], [0], x.copy())
    SV.assert_same(M, M, 1e-10)
    for e, v in ((0, 1.0 + 1e-9), (1, np.nan), (3, np.inf), (2, np.inf), (4, np.nan)):
        y = x.copy()
        y[e] = v
        with pytest.raises(AssertionError):
            SV.assert_same(O.Bcsr([2], [3], [0, 1], [0], [0], y), M, 1e-10, kernel="hand-made")
    with pytest.raises(AssertionError):   # another index
        SV.assert_same(O.Bcsr([2], [3], [0, 1], [0], [6], np.concatenate([np.zeros(6), x])), M, 1e-10)


@pytest.mark.parametrize("i", range(N), ids=SV.entry_id)
def test_conditions_on_the_seeded_operands(i):
    env, case, dtype, expect, lab, opt = SV.entries()[i]
    alpha, beta = opt.get("alpha", SV.ALPHA), opt.get("beta", SV.BETA)
    assert np.isfinite(alpha) and alpha != 0 and np.isfinite(beta)
    if np.dtype(dtype).kind == "c":   # no zero component in a scalar either: it would meet the Inf of a complex product's other component
        assert complex(alpha).real != 0 and complex(alpha).imag != 0 and complex(beta).real != 0 and complex(beta).imag != 0
    assert beta != 0 or opt.get("beta") == 0.0, "only the beta == 0 case itself has beta == 0 (the oracle then empties C: no product with beta)"
    for M in SV.clean_operands(i):
        v = parts(M.data)
        assert M.data.dtype == np.dtype(dtype)
        assert np.all(v != 0), "an operand element (component) is exactly 0: 0 x Inf would be a NaN of the true product"
        assert np.all(np.isfinite(v)) and np.max(np.abs(v)) <= 10.0
    A, B, Cm, placed = SV.seeded_operands(i)
    for M, clean in zip((A, B, Cm), SV.clean_operands(i)):
        v, w = parts(M.data), parts(clean.data)
        assert M.data.dtype == np.dtype(dtype) and np.array_equal(M.blk_p, clean.blk_p) and np.array_equal(M.col_i, clean.col_i)
        fin = np.isfinite(v)
        assert np.all(v[fin] != 0) and np.all(np.abs(v[fin]) <= 10.0)
        if beta != 0 or M is not Cm:
            assert np.array_equal(v[fin], w[fin]), "seed() changed a finite element"
            assert 0 < np.count_nonzero(~fin) <= 8 * SV.rounds_of(case)
        if np.dtype(dtype).kind == "c":   # Inf in real parts only
            assert not np.any(np.isinf(M.data.imag))
    # what was put where
    inB = [p for p in placed if p["matrix"] == "B"]
    inA = [p for p in placed if p["matrix"] == "A"]
    tails = [p for p in inB if p["role"].startswith("B +Inf at (0, c)")]
    assert len(tails) >= 3 and all(p["row"] == 0 and p["value"].real == np.inf for p in tails)
    for group, M in ((inB, B), (inA, A)):
        assert any(p["first"] for p in group) and any(p["last"] for p in group) and any(not p["first"] and not p["last"] for p in group)
    assert any(p["dominant"] for p in inA + inB), "no seeded block has the dominant size of its matrix"
    opB = O.transposed(B) if opt.get("tb", "N") != "N" else B
    if np.any(SV.tail_flags(opB)):
        assert any(p["tail"] for p in inB), "the case has tail-size blocks in B and none is seeded"
    assert any(p["role"] == "B -Inf at (k-1, n-1)" for p in inB) and any(p["role"] == "B NaN" for p in inB)
    assert {"A -Inf at (r, 0)", "A +Inf at (m-1, k-1)", "A NaN"} <= {p["role"] for p in inA}
    assert (beta != 0) == any(p["matrix"] == "C" for p in placed)
    # the oracle's product
    ref, info, ref2 = SV.seeded_reference(i)
    nonfinite, has_nan, has_inf, inf_column = SV.block_class_summary(ref)
    share = np.count_nonzero(nonfinite) / float(ref.nblks)
    print("%s: %d of %d C blocks hold a non-finite element, %d hold NaN and no Inf" % (SV.entry_id(i), np.count_nonzero(nonfinite), ref.nblks,
                                                                                      np.count_nonzero(has_nan & ~has_inf)))
    assert 0.05 <= share <= 0.50, share
    if np.dtype(dtype).kind == "c":
        # An Inf in a real part puts Inf of one sign into BOTH components of op(A) op(B), and alpha (no zero component) combines them with both
        # signs in one of the components of alpha P: NaN there, whatever alpha is.  (With a zero component in alpha it would be 0 x Inf.)  So a
        # complex case shows each Inf as one Inf and one NaN component, and tells a kernel's stray NaN from a finite element, not from an Inf.
        assert {0, 3} <= set(np.unique(SV.classes(ref.data)).tolist()) and {1, 2} & set(np.unique(SV.classes(ref.data)).tolist())
    else:
        assert set(np.unique(SV.classes(ref.data)).tolist()) == {0, 1, 2, 3}
        assert inf_column, "no C block has a column that is +-Inf in every element"
    assert np.count_nonzero(has_nan & ~has_inf) >= 5
    if beta == 0:   # the old C (all NaN) is gone: the clean part of the product is finite
        assert np.count_nonzero(~nonfinite) > 0


@pytest.mark.parametrize("case", SV.filter_cases())
def test_conditions_on_the_filter_cases(case):
    from tests import test_gpu_filter_in_place as FIP
    clean, (A, B, Cm, placed), eps = SV.filter_operands(case)
    assert eps == FIP.quantile_eps(case, 0.5)   # (with its own two assertions: 5 % to 95 % dropped, no norm on the threshold -- on the clean operands)
    for M in clean:
        assert np.all(M.data != 0) and np.max(np.abs(M.data)) <= 10.0
    ref, info, full = SV.filter_reference(case)
    nonfinite, has_nan, has_inf, _ = SV.block_class_summary(full)
    rows = full.rows()
    nan_blocks = {(int(rows[b]), int(full.col_i[b])) for b in np.flatnonzero(has_nan)}
    nan_only = {(int(rows[b]), int(full.col_i[b])) for b in np.flatnonzero(has_nan & ~has_inf)}
    kept = SV.coordinates(ref)
    print("%s: eps %.6g keeps %d of %d blocks, %d hold NaN (%d of them no Inf)" % (case, eps, ref.nblks, full.nblks, len(nan_blocks), len(nan_only)))
    assert len(nan_only) >= 5
    assert nan_blocks <= kept, "the oracle dropped a block that holds NaN"
    assert ref.nblks < full.nblks, "the filter drops nothing"
    # the stand-alone filter's rule on the oracle's own product: a NaN norm is not below the threshold
    norms = SV.block_sq_norms(full)
    keep = ~(norms < eps * eps)
    assert np.all(keep[has_nan]) and 0 < np.count_nonzero(keep) < full.nblks


@pytest.mark.parametrize("i,pq", SV.scaling_entries(), ids=lambda v: SV.entry_id(v) if isinstance(v, int) else "p%d_q%d" % v)
def test_scaled_results_stay_normal(i, pq):
    env, case, dtype, expect, lab, opt = SV.entries()[i]
    p, q = pq
    ref, _ = SV.clean_reference(i)
    v = np.abs(parts(ref.data).astype(np.float64))
    v = v[v != 0]
    fi = np.finfo(np.float32 if np.dtype(dtype) == np.float32 else np.float64)
    hi, lo = np.ldexp(np.max(v), p + q), np.ldexp(np.min(v), p + q)
    assert float(fi.tiny) <= lo and hi <= float(fi.max) / 4, (lo, hi)
    # the operands themselves, and the largest product of two of them
    for M, s in zip(SV.clean_operands(i), (p, q, p + q)):
        w = np.abs(parts(M.data).astype(np.float64))
        assert float(fi.tiny) <= np.ldexp(np.min(w), s) and np.ldexp(np.max(w), s) <= float(fi.max) / 4


def test_every_pair_meets_the_families_with_enough_entries():
    seen = {}
    for i, pq in SV.scaling_entries():
        env, case, dtype, expect, lab, opt = SV.entries()[i]
        seen.setdefault((np.dtype(dtype).name, expect.split("<")[0].split("[")[0]), []).append(pq)
    for (name, family), pairs in seen.items():
        want = SV.PAIRS[np.dtype(name)]
        assert set(pairs) == set(want) or len(pairs) < len(want), (name, family, pairs)
    for name in ("float64", "float32"):
        assert {pq for (n, f), pairs in seen.items() if n == name for pq in pairs} == set(SV.PAIRS[np.dtype(name)])


@pytest.mark.parametrize("case", ["mixed", "23_with_tails"])
def test_float_norms_of_the_scaled_filter_cases(case):
    """the premises of test_saturated_float_norms_with_the_filter_on: the single-precision block norms (sums of squares, as the oracle and the device
    keep them) of A * 2^70 are all +Inf, those of A * 2^40 and B * 2^-40 are normal numbers, and the filter drops blocks on the clean operands"""
    from tests import test_gpu_filter_in_place as FIP
    A, B, Cm = FIP.inputs(case)
    eps = FIP.quantile_eps(case, 0.5)

    def float_norms(M, p):
        S = SV.scaled(M, p)
        with np.errstate(over="ignore", under="ignore"):
            return O.norms(S.data, S.blk_p.astype(np.int32), SV.block_sizes(S).astype(np.int32))

    tiny, big = float(np.finfo(np.float32).tiny), float(np.finfo(np.float32).max)
    assert np.all(np.isposinf(float_norms(A, 70)))
    for M, p in ((A, 40), (B, -40), (A, 0), (B, 0)):
        v = float_norms(M, p)
        assert np.all(v >= tiny) and np.all(v <= big)
    assert np.all(float_norms(B, -70) < tiny), "B * 2^-70: norms below the normal range (Inf x 0 is NaN, Inf x subnormal is Inf: neither is below a threshold)"
    ref, info = O.multiply("N", "N", 1.0, SV.scaled(A, 70), SV.scaled(B, -70), 1.0, Cm, filter_eps=eps)
    full, full_info = O.multiply("N", "N", 1.0, A, B, 1.0, Cm)
    clean, clean_info = O.multiply("N", "N", 1.0, A, B, 1.0, Cm, filter_eps=eps)
    assert info["flop"] == full_info["flop"] > clean_info["flop"], "saturated norms: no product is skipped, and the clean case skips some"
    assert ref.nblks < full.nblks, "the final filter still drops blocks"
