"""What tests/test_gpu_option_sweep.py relies on, checked without a GPU: the block-level restatement of tests/option_sweep.py reproduces the oracle's index,
flop and values on every real case; no default case fails a condition on its inputs; the default ranges cover what they are meant to cover; and the
reference notices the three mistakes it is there to notice (a dropped conjugation, a crop bound off by one, a complex norm from the real part alone)."""
import numpy as np
import pytest

from tests import option_sweep as S
from tests.test_numeric_choice import choose, shims  # noqa: F401  (the host build of mm_choose.h, a module-scoped fixture)

if not S.LONG_DOUBLE_OK:
    pytest.skip("np.longdouble has no 63-bit mantissa here: the reference of the option sweep needs one", allow_module_level=True)

ALL = [(name, i) for name in S.STRATA for i in range(S.count(name))]


@pytest.mark.parametrize("name", S.STRATA)
def test_restatement_reproduces_the_oracle_on_real_cases(name):
    """index, flop and values (at the fp64 bar: the oracle sums in float64) on every real case, the filtered ones among them"""
    seen = filtered = 0
    for i in range(S.count(name)):
        c = S.case(name, i)
        if c["dtype"] == S.Z64:
            continue
        ref = S.reference(name, i)
        orc, info = S.oracle_result(c, *S.operands(name, i))
        assert np.array_equal(orc.row_p, ref.row_p) and np.array_equal(orc.col_i, ref.col_i), (name, i, "index")
        assert int(info["flop"]) == ref.flop and int(info["nproducts"]) == ref.nproducts, (name, i, info["flop"], ref.flop)
        (_, _, (k0, k1), _, _) = S.window_of(c)
        n = k1 - k0 + 1
        g = (n + 8) * 2.0 ** -53 / (1 - (n + 8) * 2.0 ** -53)
        D = S.dense_ld(orc)
        assert np.all(np.abs(D - ref.R)[ref.stored] <= g * ref.bound[ref.stored]), (name, i, "values")
        seen += 1
        filtered += c["eps"] > 0
    if name != "complex":
        assert seen >= 10 and filtered >= 1, (seen, filtered)   # (symmetry: its one filtered fp32 product)


def test_complex_index_without_a_filter_is_the_oracles_on_the_real_parts():
    """the restatement's own index and flop against the second reference the device is held to"""
    seen = 0
    for name, i in ALL:
        c = S.case(name, i)
        if c["dtype"] == S.Z64 and c["eps"] == 0:
            ref = S.reference(name, i)
            row_p, col_i, flop = S.expected_index(name, i)
            assert np.array_equal(row_p, ref.row_p) and np.array_equal(col_i, ref.col_i) and flop == ref.flop, (name, i)
            seen += 1
    assert seen >= 40


def test_no_default_case_fails_a_condition():
    bad = {(name, i): S.conditions(name, i) for name, i in ALL}
    bad = {k: v for k, v in bad.items() if v}
    assert not bad, bad


def test_limit_cases_cut_inside_blocks():
    cuts = np.zeros(3, int)
    for i in range(S.count("limits")):
        cuts += np.asarray(S.cuts_inside(S.case("limits", i)), int)
    assert np.all(cuts >= 5), cuts


def test_coverage_of_the_default_ranges():
    cases = [S.case(name, i) for name, i in ALL]
    for dt, pairs in ((S.Z64, S.PAIRS_Z), (S.F64, S.PAIRS_R), (S.F32, S.PAIRS_R)):
        assert {c["ta"] + c["tb"] for c in cases if c["dtype"] == dt} >= set(pairs), dt
    for d in range(3):
        assert {c["kinds"][d] for c in cases if c["kinds"]} == set(S.LIMIT_KINDS), d
    for s in "SAHK":
        assert any(c["symm_a"] == s for c in cases) and any(c["symm_b"] == s for c in cases) and any(c["symm_c"] == s for c in cases), s
    assert any(c["alpha"] == 0 for c in cases) and any(c["beta"] == 0 for c in cases) and any(c["beta"] == 1 for c in cases)
    ops = [S.operands(name, i) for name, i in ALL]
    assert any(A.nblks == 0 or B.nblks == 0 for A, B, _ in ops) and any(Cm.nblks == 0 for _, _, Cm in ops)
    assert any(S.reference(name, i).col_i.size == 0 for name, i in ALL)
    assert sum(c["retain"] for c in cases) >= 20 and sum(bool(c["env"]) for c in cases) >= 20
    assert sum(c["dtype"] == S.Z64 and c["eps"] > 0 for c in cases) >= 10
    assert sum(c["symm_c"] != "N" for c in cases) == 10 and sum(c["symm_c"] != "N" and c["eps"] > 0 for c in cases) == 2
    assert any(c["symm_c"] != "N" and c["retain"] for c in cases)
    assert max(max(c["mix_m"][1::2] + c["mix_n"][1::2] + c["mix_k"][1::2]) for c in cases if c["dtype"] == S.F32) > 80


@pytest.fixture(scope="module")
def predicted(shims):  # noqa: F811
    out = {}
    for name, i in ALL:
        q = S.choice_case(name, i)
        if q is not None:
            out[(name, i)] = S.family(choose(shims, S.case(name, i)["env"], q[0], **q[1])[0])
    return out


def test_kernel_families_the_choice_predicts(predicted):
    fams = set(predicted.values())
    print(sorted(fams))
    assert {"f64_generic", "f32_generic", "f64_big", "f64_mid"} <= fams and fams & {"f32_direct", "f32_hot"}, fams


# ---- the reference notices what it is there to notice ------------------------------------------------------------------------------------------------------
def first(pred):
    return next((name, i) for name, i in ALL if pred(S.case(name, i), S.reference(name, i)))


def as_result(name, i, R):
    """the dense R in the storage form of the reference's result, rounded to the case's data type: what a device would hand back"""
    ref, (_, _, Cm) = S.reference(name, i), S.operands(name, i)
    rs, cs = Cm.row_sizes, Cm.col_sizes
    ro, co = S.offsets(rs), S.offsets(cs)
    rows = np.repeat(np.arange(len(rs)), np.diff(ref.row_p))
    chunks = [R[ro[r]:ro[r + 1], co[c]:co[c + 1]].T.reshape(-1) for r, c in zip(rows, ref.col_i)]
    size = np.asarray([x.size for x in chunks], np.int64)
    data = (np.concatenate(chunks) if chunks else np.zeros(0)).astype(Cm.data.dtype)
    return S.O.Bcsr(rs, cs, ref.row_p, ref.col_i, np.concatenate([[0], np.cumsum(size)[:-1]]) if chunks else np.zeros(0, np.int64), data)


def test_the_references_own_result_passes_and_a_wrong_one_fails():
    for name in S.STRATA:
        for i in range(0, S.count(name), 7):
            ref = S.reference(name, i)
            bad, worst = S.compare(name, i, as_result(name, i, ref.R), ref.flop)
            assert bad is None and worst <= 1.0, (name, i, bad)   # (rounding R to the data type: half an ulp, inside every bar)
    # a dropped conjugation: the 'T' twin's values on a case with 'C'
    name, i = first(lambda c, r: "C" in c["ta"] + c["tb"] and c["eps"] == 0 and c["limits"] is None and r.col_i.size)
    t = S.restate(S.twin_case(S.case(name, i)), *S.operands(name, i))
    bad, _ = S.compare(name, i, as_result(name, i, t.R), t.flop)
    assert bad is not None and bad["what"] == "values", bad
    # a crop bound shifted by one element, in rows, columns and k: on the cases cut inside a block there, the shifted window's result is caught (by the
    # index where the shift drops or adds a block, else by the values or by the bits outside the window) in at least five cases per dimension
    for d in range(3):
        caught = 0
        for i in range(S.count("limits")):
            c, ref = S.case("limits", i), S.reference("limits", i)
            if not (S.cuts_inside(c)[d] and c["limits"][2 * d + 1] > 1 and c["alpha"] != 0 and ref.col_i.size):
                continue
            lim = list(c["limits"])
            lim[2 * d + 1] -= 1
            lim[2 * d] = min(lim[2 * d], lim[2 * d + 1])
            t = S.restate(dict(c, limits=tuple(lim)), *S.operands("limits", i))
            same_index = np.array_equal(t.row_p, ref.row_p) and np.array_equal(t.col_i, ref.col_i)
            caught += not same_index or S.compare("limits", i, as_result("limits", i, t.R), t.flop)[0] is not None
        assert caught >= 5, (d, caught)


def test_a_complex_norm_from_the_real_part_alone_changes_a_filtered_complex_case():
    changed = 0
    for name, i in ALL:
        c = S.case(name, i)
        if c["dtype"] == S.Z64 and c["eps"] > 0:
            ref = S.reference(name, i)
            t = S.restate(c, *S.operands(name, i), norm_of=lambda X: X.real * X.real)
            changed += not (np.array_equal(t.row_p, ref.row_p) and np.array_equal(t.col_i, ref.col_i) and t.flop == ref.flop)
    assert changed >= 3, changed
