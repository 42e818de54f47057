"""What makes the walks of tests/engine_sequences.py worth running, asserted on the host from the oracle alone (tests/test_gpu_engine_sequences.py runs
them on one long-lived engine): the pool holds the kernel families and options it is meant to hold, every walk has the property it is named for, and the
stale-norms scenario can tell stale norms from fresh ones."""
import numpy as np
import pytest

from tests import engine_sequences as ES
from tests.test_numeric_choice import choose, shims  # noqa: F401  (the host build of mm_choose.h, a module-scoped fixture)


def test_the_pool_holds_what_it_is_meant_to_hold():
    n = ES.pool_counts()
    print("pool:", n)
    assert n["cases"] == len(ES.POOL) == len(ES.FAMILY) <= 36 and len(set(ES.POOL)) == len(ES.POOL)
    assert sum(k == ES.Z for k, _ in ES.POOL) == 4
    assert all(n["families"][f] >= 2 for f in ES.FAMILIES), n["families"]
    assert n["eps > 0"] >= 6 and n["retain"] >= 4 and n["symmetric C"] >= 4
    assert {"NN", "NT", "TN", "TT"} <= set(n["transposes"]) and "CN" in n["transposes"] and "TC" in n["transposes"]
    assert n["alpha == 0"] >= 1 and n["beta == 0"] >= 1
    assert n["C_in without a block"] >= 1 and n["result without a block"] >= 1 and n["A without a block"] >= 1
    for i in range(len(ES.POOL)):
        print(ES.host(i))


def test_the_families_are_those_of_the_host_build_of_the_choice(shims):  # noqa: F811
    answered = 0
    for i in range(len(ES.POOL)):
        h = ES.host(i)
        q = ES.choice_case(h)
        if h.complex:
            assert ES.FAMILY[i] == "z64"
        if q is None:
            continue
        name, _ = choose(shims, {}, q[0], **q[1])
        print("pool[%d]: %s" % (i, name))
        assert ES.family_of(name) == ES.FAMILY[i], (i, name)
        answered += 1
    assert answered >= 22   # (the rest, products with symmetry and complex data, from last_kernel() on the device)


def test_walks_are_lists_of_pool_indices_of_16_to_20():
    assert set(ES.WALKS) == {"descending", "ascending", "shuffled_a", "shuffled_b", "types", "filters"}
    assert all(len(w) == 3 and set(w) <= set(ES.WALKS) for w in ES.SWITCH_WALKS.values())
    for name, w in ES.WALKS.items():
        assert 16 <= len(w) <= 20 and all(0 <= i < len(ES.POOL) for i in w), name
    used = set().union(*ES.WALKS.values())
    assert used == set(range(len(ES.POOL))), "every pool entry is walked: %s are not" % sorted(set(range(len(ES.POOL))) - used)
    for name in ("shuffled_a", "shuffled_b"):
        assert len(set(ES.WALKS[name])) == len(ES.WALKS[name])


def test_descending_and_ascending():
    d = [ES.host(i) for i in ES.WALKS["descending"]]
    print("descending:", [(h.c_blocks, h.products) for h in d])
    assert all(a.c_blocks > b.c_blocks and a.products > b.products for a, b in zip(d, d[1:]))
    a = [ES.host(i) for i in ES.WALKS["ascending"]]
    print("ascending:", [h.c_blocks for h in a])
    assert all(x.c_blocks < y.c_blocks for x, y in zip(a, a[1:]))


def test_types_changes_the_data_type_at_every_step():
    t = [ES.host(i).dtype for i in ES.WALKS["types"]]
    print("types:", t)
    assert all(x != y for x, y in zip(t, t[1:])) and set(t) == {"float64", "float32", "complex128"}
    assert t[:3] == ["float64", "float32", "complex128"]


def test_filters_alternates_and_every_filtered_case_drops_blocks():
    f = [ES.host(i) for i in ES.WALKS["filters"]]
    print("filters:", [(h.filtered, h.unfiltered_blocks, h.c_blocks, round(h.dropped, 2)) for h in f])
    assert all(x.filtered != y.filtered for x, y in zip(f, f[1:]))
    for h in f:
        if h.filtered:
            assert 0.10 <= h.dropped <= 0.90 and not h.par["retain"], h
        else:
            assert h.par["eps"] == 0.0
    for kind in (True, False):   # large then small, each kind
        sizes = [h.unfiltered_blocks for h in f if h.filtered == kind]
        assert sizes == sorted(sizes, reverse=True)


@pytest.mark.parametrize("op", ES.STALE_OPS)
def test_stale_norms_would_keep_another_set_of_blocks(op):
    """the in-place change moves at least 10 % of the blocks across the final filter's eps: a filter that used the norms of the values before the change
    returns another index than the oracle's for the changed matrix"""
    before, after, _ = ES.kept_sets(op)
    differ = float(np.count_nonzero(before != after)) / before.size
    print("%s: %d blocks, %d kept before the change, %d after it, %.0f %% change sides" % (op, before.size, before.sum(), after.sum(), 100 * differ))
    assert differ >= 0.10
    assert 0 < after.sum() < after.size


# ---- part E: the algebra walks ---------------------------------------------------------------------------------------------------------------------------
def test_the_algebra_pool_is_what_the_walks_need():
    hs = [ES.alg(k) for k in range(len(ES.ALG_POOL))]
    for h in hs:
        print(h)
        assert np.array_equal(h.M.row_sizes, h.M.col_sizes) and all(h.M.col_i[h.M.row_p[r]:h.M.row_p[r + 1]].tolist().count(r) == 1 for r in range(h.nb))
        assert 55 <= h.n <= 600 and h.sizes.max() <= 96, "what the block inverse and the block scale accept"
        assert 0.3 <= h.M.nblks / h.nb ** 2 <= 0.6 and 0.3 <= h.Q.nblks / h.nb ** 2 <= 0.6
        assert h.Q.nblks != h.M.nblks or not np.array_equal(h.Q.col_i, h.M.col_i), "Q has another pattern"
        assert max(h.subs) < h.nb and h.sub_n <= h.n
    types = [h.dtype.name for h in hs]
    assert len(hs) == 10 and (types.count("float64"), types.count("float32"), types.count("complex128")) == (5, 3, 2)
    assert len({h.sizes.tobytes() for h in hs}) > 8, "more sets of block sizes than the engine remembers: its ring wraps"


def test_the_algebra_walks_cover_every_operation():
    assert set(ES.ALG_WALKS) == {"descending", "ascending", "shuffled"} and len(set(ES.ALG_OPS)) == len(ES.ALG_OPS) >= 30
    preds = {op: set() for op in ES.ALG_OPS}
    for name, w in ES.ALG_WALKS.items():
        assert all(op in ES.ALG_OPS and ES.alg(k).admits(op) for op, k in w), name
        for op in ES.ALG_OPS:
            assert sum(o == op for o, _ in w) >= 2, (name, op)
        t = [ES.alg(k).dtype.name for _, k in w]
        changes = sum(x != y for x, y in zip(t, t[1:]))
        print("%s: %d steps, the element type changes %d times" % (name, len(w), changes))
        assert changes >= 10, name
        for (a, _), (b, _) in zip(w, w[1:]):
            preds[b].add(a)
    assert all(len(p) >= 3 for p in preds.values()), {op: sorted(p) for op, p in preds.items() if len(p) < 3}
    full = lambda name: [ES.alg(k).n for _, k in ES.ALG_WALKS[name]]
    assert all(x >= y for x, y in zip(full("descending"), full("descending")[1:])) and full("descending")[0] > full("descending")[-1]
    assert all(x <= y for x, y in zip(full("ascending"), full("ascending")[1:])) and full("ascending")[0] < full("ascending")[-1]
    assert len({k for _, k in ES.ALG_WALKS["shuffled"]}) >= 8
