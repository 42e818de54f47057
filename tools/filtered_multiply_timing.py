#!/usr/bin/env python3
"""filtered multiply of sparse matrices (config 4's shape): unfiltered, filter that drops nothing, filter that drops about a third
of the blocks; candidate-driven against product-driven symbolic kernels.

Every filtered multiply is timed in BOTH forms of the final block filter -- the copying one (the default) and the in-place one
(MultiplyEngine.filter_in_place: C's index is compacted, its data area stays) -- on the same operands in the same process,
alternating, REPS repetitions of each, so that the spread of the copying form is known.  Before a time is printed the two results
are compared (row_p and col_i equal, every kept block bit-identical): faster and different is not faster.  A difference counts as a
gain only beyond three times that spread."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch

from dbcsr_amd.multiply import MultiplyEngine
from dbcsr_amd.randmat import perf_matrices

SHAPE = os.environ.get("SHAPE", "config4")
REPS = max(5, int(os.environ.get("REPS", "7")))
PER_REP = 4   # multiplies per repetition
SIZE, FILL, MIX, EPS = {"config4": (131072, 0.01, [1, 23], 140.0), "config3": (32768, 0.05, [1, 13, 1, 23, 1, 32], 300.0),
                        "config2": (32768, 0.10, [1, 23], 500.0)}[SHAPE]


def multiply(E, A, B, Cm, eps, in_place):
    E.filter_in_place = in_place
    return E.multiply_local(1.0, A, B, 1.0, Cm, filter_eps=eps)


def one_rep(E, A, B, Cm, eps, in_place):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(PER_REP):
        out, cnt = multiply(E, A, B, Cm, eps, in_place)
        del out
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / PER_REP * 1e3


def compare(E, A, B, Cm, eps):
    """the two forms' results at the timed size; returns (blocks before the filter, blocks after, products, elements kept, elements of the data area)"""
    Y, cnt = multiply(E, A, B, Cm, eps, False)
    X, _ = multiply(E, A, B, Cm, eps, True)
    torch.cuda.synchronize()
    assert torch.equal(X.row_p, Y.row_p) and torch.equal(X.col_i, Y.col_i), "the two forms' index differs"
    assert X.nze == Y.data.numel(), "the two forms keep different element counts"
    if X.nblks != cnt.c_nblks:
        assert X.data.numel() == cnt.c_nze and not X.packed, "the in-place form did not keep the product's data area"
        assert bool((X.blk_p[1:] > X.blk_p[:-1]).all()), "blk_p of the in-place result is not increasing"
    packed = E.cropped(X)   # the packing copy: the kept blocks in index order
    torch.cuda.synchronize()
    assert torch.equal(packed.blk_p, Y.blk_p), "the packed in-place result is laid out differently"
    assert torch.equal(packed.data.view(torch.int64), Y.data.view(torch.int64)), "a kept block differs between the two forms"
    res = (cnt.c_nblks, X.nblks, cnt.nproducts, X.nze, X.data.numel())
    del X, Y, packed
    return res


def line(times):
    return "%.2f ms (min %.2f, max %.2f)" % (statistics.median(times), min(times), max(times))


for symbolic in (sys.argv[1:] or ["grid", "auto"]):
    if symbolic == "auto":
        os.environ.pop("DBCSR_AMD_MM_SYMBOLIC", None)
    else:
        os.environ["DBCSR_AMD_MM_SYMBOLIC"] = symbolic
    E = MultiplyEngine()
    A, B, Cm = perf_matrices(SIZE, SIZE, SIZE, (1 - FILL,) * 3, MIX, MIX, MIX, dtype=torch.float64, engine=E)
    for eps in (0.0, 1.0e-3, EPS):
        before, after, nprod, nze, area = compare(E, A, B, Cm, eps)
        forms = (False,) if eps == 0.0 else (False, True)
        for in_place in forms:   # warm-up
            one_rep(E, A, B, Cm, eps, in_place)
        times = {f: [] for f in forms}
        for _ in range(REPS):
            for in_place in forms:
                times[in_place].append(one_rep(E, A, B, Cm, eps, in_place))
        head = "symbolic=%s filter_eps=%g:" % (symbolic, eps)
        tail = "%d blocks before the final filter, %d after, %d products" % (before, after, nprod)
        if eps == 0.0:
            print("%s %s per multiply, %s" % (head, line(times[False]), tail), flush=True)
            continue
        print("%s copying  %s per multiply, %s" % (head, line(times[False]), tail), flush=True)
        print("%s in place %s per multiply, results identical, %d of %d elements of the data area referenced" %
              (head, line(times[True]), nze, area), flush=True)
        spread = max(times[False]) - min(times[False])
        gain = statistics.median(times[False]) - statistics.median(times[True])
        verdict = "in place faster" if gain > 3 * spread else ("in place SLOWER" if -gain > 3 * spread else "no gain (within 3 x the spread)")
        print("%s copying - in place = %.2f ms, spread of the copying form %.2f ms over %d repetitions of %d multiplies: %s" %
              (head, gain, spread, REPS, PER_REP, verdict), flush=True)
    E.filter_in_place = False
    del A, B, Cm, E
