"""The tables of tests/kernel_instances.py, checked without a GPU: every row is given the instance it names by the choice rules (the shim of
tests/test_numeric_choice.py around mm_choose.h, tests/test_numeric_choice_complex.py's for complex data), the rows reach exactly the instances the
source lists, and the reference (the CPU oracle) confirms what the cases are built for -- product lists of every length the kernels' look-ahead
distinguishes, a C_in that holds some product blocks and lacks others, a filter threshold no block sits on.  tests/test_gpu_kernel_instances.py runs
the same rows on the device."""
import functools
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import kernel_instances as KI
from tests.test_numeric_choice import block_sizes, choose, shims  # noqa: F401  (shims: the module's fixture, used here as it is there)
from tests.test_numeric_choice_complex import FAMILY_Z64
from tests.test_numeric_choice_complex import choose as choose_z

MID, MID_CLASS, BIG, Z64, CLASS = KI.mid_cases(), KI.mid_class_cases(), KI.big_cases(), KI.z64_cases(), KI.class_cases()
CLASS_ENV = {"DBCSR_AMD_MM_CLASSES": "2"}


@functools.lru_cache(maxsize=None)
def reference(table, name):
    """(A, B, C_in, the reference's product at the general multiply's alpha / beta, its info) of a real case"""
    case = {"mid": MID, "mid_class": MID_CLASS, "big": BIG, "class": CLASS}[table][name][0]
    A, B, Cm = O.perf_case(*case)
    ref, info = O.multiply("N", "N", KI.FILTER_ALPHA, A, B, KI.FILTER_BETA, Cm)
    return A, B, Cm, ref, info


def real_counts(table, name):
    _, _, _, ref, info = reference(table, name)
    return dict(c_nblks=ref.nblks, products_per_block=info["nproducts"] / max(ref.nblks, 1))


# ---- the lists ------------------------------------------------------------------------------------------------------------------------------------------
def test_the_lists_are_read_from_the_source():
    mid, big, z64 = KI.mid_shapes(), KI.big_shapes(), KI.z64_shapes()
    assert len(mid) == len(set(mid)) == 43 and len(big) == 16 and len(z64) == 16
    assert set(KI.MID_CLASS_SHAPES) == {s for s in mid if max(s) <= 8}   # both dimensions within 32: (m, n) classes only
    assert set(big) == {(a, b) for a in range(2, 6) for b in range(2, 6)} and set(z64) == {(a, b) for a in range(1, 5) for b in range(1, 5)}


def test_every_listed_instance_has_a_case():
    """an instance added to mm_choose.h fails here until a case reaches it"""
    assert {s for _, s in MID.values()} | {s for _, s in MID_CLASS.values()} == set(KI.mid_shapes())
    assert {s for _, s in BIG.values()} == set(KI.big_shapes())
    assert {s for _, s in Z64.values()} == set(KI.z64_shapes())
    kinds = {}
    for name, (_, s) in MID.items():
        kinds.setdefault(s, set()).add(name.split("-")[1])
    assert all(k == ({"full"} if min(s) >= 11 else {"least", "full"}) for s, k in kinds.items()), kinds
    assert {name.split("-k")[1] for name in MID} == {str(k) for k in KI.MID_K}
    assert len(CLASS) == 24 and [s for _, s in CLASS.values()] == KI.class_shapes()
    with open(os.path.join(KI.ROOT, "tests", "test_gpu_class_mode.py")) as fh:
        assert KI.CLASS_TAIL_RULE in fh.read()


# ---- the choice -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MID))
def test_mid_rows_are_given_their_instance(shims, name):
    case, (rb, cb) = MID[name]
    counts = real_counts("mid", name)
    for kw in ({}, {"retain": True}, {"retain": True, "skip_empty": True}, {"filter_active": True}):
        got, o = choose(shims, {}, case, **counts, **kw)
        assert got == "mm_numeric_f64_mid<%d,%d>" % (rb, cb) and (o["mid_rb"], o["mid_cb"]) == (rb, cb) and o["work"], (got, o)
        assert o["flags"] == int(bool(kw.get("skip_empty")))
        assert bool(o["norms"]) == bool(o["leaves_norms"]) == bool(kw.get("filter_active")), o
    # the tail row and column are blocks of another size: the second launch is part of the case
    sm, sn = block_sizes(case[0], case[6]), block_sizes(case[1], case[7])
    assert len(set(sm)) == 2 and len(set(sn)) == 2 and sm[-1] < sm[0] and sn[-1] < sn[0]


@pytest.mark.parametrize("name", sorted(MID_CLASS))
def test_mid_class_rows_are_in_class_mode_with_one_slab_class(shims, name):
    case, (rb, cb) = MID_CLASS[name]
    for kw in ({}, {"filter_active": True}):
        got, o = choose(shims, CLASS_ENV, case, **real_counts("mid_class", name), **kw)
        assert got == "mm_numeric_f64_class[" and o["cls_mode"] and o["mid_class_mode"] == 1 and o["work"], (got, o)
        assert bool(o["leaves_norms"]) == bool(kw.get("filter_active"))
    sm, sn = sorted(set(block_sizes(case[0], case[6]))), sorted(set(block_sizes(case[1], case[7])))
    served = [(m, n) for m in sm for n in sn if KI.mid_serves(m, n, 1)]
    assert served == [(sm[-1], sn[-1])] and ((sm[-1] + 3) // 4, (sn[-1] + 3) // 4) == (rb, cb)
    # uniform blocks of that size by themselves (mode 0) are not the slab kernel's: only the class takes them
    assert not KI.mid_serves(sm[-1], sn[-1], 0) and not choose(shims, {}, (5 * sm[-1], 5 * sn[-1], 65, 0.5, 0.5, 0.5, [1, sm[-1]], [1, sn[-1]], [1, 13]))[0].startswith("mm_numeric_f64_mid")


def test_mid_serves_restates_the_header(shims):
    """uniform m x n blocks: the slab kernel is chosen exactly where KI.mid_serves(m, n, 0) says so"""
    for m in range(17, 49):
        for n in range(17, 49):
            got = choose(shims, {}, (5 * m, 5 * n, 65, 0.5, 0.5, 0.5, [1, m], [1, n], [1, 13]))[0]
            assert got.startswith("mm_numeric_f64_mid<") == KI.mid_serves(m, n, 0), (m, n, got)
            if KI.mid_serves(m, n, 0):
                assert got == "mm_numeric_f64_mid<%d,%d>" % ((m + 3) // 4, (n + 3) // 4)


@pytest.mark.parametrize("name", sorted(BIG))
def test_big_rows_are_given_their_instance(shims, name):
    case, (tm, tn) = BIG[name]
    for kw in ({}, {"retain": True}, {"retain": True, "skip_empty": True}):
        got, o = choose(shims, {}, case, **real_counts("big", name), **kw)
        assert got == "mm_numeric_f64_big<%d,%d>" % (tm, tn), got
        assert o["flags"] == int(bool(kw.get("skip_empty"))) and not o["work"]
    m = case[6][1]
    assert (-(-m // 8)) % 2 == {13: 0, 45: 0, 53: 1, 69: 1}[m]   # both parities of ceil(m / 8) between the two wave rows
    assert {(-(-KI.BIG_M[t] // 8)) % 2 for t in KI.BIG_M} == {0, 1}


@pytest.mark.parametrize("name", sorted(Z64))
def test_z64_rows_are_given_their_instance(name):
    (M, N, K, _, mix_m, mix_n, mix_k), (ma, nc) = Z64[name]
    sm, sn, sk = block_sizes(M, mix_m), block_sizes(N, mix_n), block_sizes(K, mix_k)
    nblk = max(1, len(sm) * len(sn) // 2)
    c = choose_z(dict(max_m=max(sm), min_m=min(sm), max_n=max(sn), min_n=min(sn), max_k=max(sk), min_k=min(sk), nbr=len(sm), nbc=len(sn), c_nblks=nblk,
                      nproducts=3 * nblk, order_len=(nblk + 7) // 8 + 8, cplx=1, fp64=0))
    assert c["family"] == FAMILY_Z64 and c["name"] == "mm_numeric_z64<%d,%d>" % (ma, nc), c
    assert len(set(sm)) == 2 and len(set(sn)) == 2


@pytest.mark.parametrize("name", sorted(CLASS))
def test_class_rows_are_in_class_mode(shims, name):
    case, (m, n, k) = CLASS[name]
    got, o = choose(shims, CLASS_ENV, case, **real_counts("class", name))
    assert got == "mm_numeric_f64_class[" and o["cls_mode"], (got, o)
    sm, sn, sk = block_sizes(case[0], case[6]), block_sizes(case[1], case[7]), block_sizes(case[2], case[8])
    assert (sm[0], sn[0], sk[0]) == (m, n, k) and sm[-1] == KI.class_tail(m, 1) and sn[-1] == KI.class_tail(n, 2) and sk[-1] == KI.class_tail(k, 3)
    # the class of the shape itself is one hiprtc compiles (the slab kernel takes none of these at their own size except where mid_serves says so)
    assert max(sm + sn + sk) <= 32


# ---- what the reference says about the cases ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table,name", [("mid", n) for n in sorted(MID)] + [("mid_class", n) for n in sorted(MID_CLASS)] + [("big", n) for n in sorted(BIG)])
def test_product_lists_of_every_length_and_a_partial_c_in(table, name):
    A, B, Cm, ref, info = reference(table, name)
    case = {"mid": MID, "mid_class": MID_CLASS, "big": BIG}[table][name][0]
    m, n = case[6][1], case[7][1]
    lengths = KI.product_list_lengths(A, B, ref, m, n)
    assert lengths.size > 0 and {int(min(v, 3)) for v in lengths} == {0, 1, 2, 3}, sorted(lengths)
    all_lengths = KI.block_pattern(A).astype(np.int64) @ KI.block_pattern(B).astype(np.int64)
    assert int(all_lengths.sum()) == info["nproducts"]   # (the lengths are the reference's: its count of products is their sum)
    # C_in holds some of the blocks that receive products and lacks others, among the blocks of the instance's size
    PC, rows = KI.block_pattern(Cm), ref.rows()
    own = (ref.row_sizes[rows] == m) & (ref.col_sizes[ref.col_i] == n) & (all_lengths[rows, ref.col_i] > 0)
    in_cin = PC[rows[own], ref.col_i[own]]
    assert in_cin.any() and not in_cin.all()


@pytest.mark.parametrize("table,name", [("mid", n) for n in sorted(MID)] + [("mid_class", n) for n in sorted(MID_CLASS)])
def test_filter_threshold_splits_the_blocks_and_none_sits_on_it(table, name):
    A, B, Cm, full, _ = reference(table, name)
    eps = KI.filter_eps(full)
    below, _ = O.multiply("N", "N", KI.FILTER_ALPHA, A, B, KI.FILTER_BETA, Cm, filter_eps=eps * (1 - 1e-6))
    at, _ = O.multiply("N", "N", KI.FILTER_ALPHA, A, B, KI.FILTER_BETA, Cm, filter_eps=eps)
    above, _ = O.multiply("N", "N", KI.FILTER_ALPHA, A, B, KI.FILTER_BETA, Cm, filter_eps=eps * (1 + 1e-6))
    assert 0.25 * full.nblks <= at.nblks <= 0.75 * full.nblks, (at.nblks, full.nblks)
    for other in (below, above):
        assert np.array_equal(other.row_p, at.row_p) and np.array_equal(other.col_i, at.col_i) and np.array_equal(other.blk_p, at.blk_p)
        assert np.array_equal(other.data, at.data)   # (nor does a product sit on the on-the-fly filter's threshold: the same products were summed)
    # the surviving blocks' norms are clear of the threshold by more than any rounding of a sum of this length
    norms = KI.block_norms(at)
    assert norms.min() > eps * (1 + 1e-6)
