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
