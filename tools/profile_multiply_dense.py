#!/usr/bin/env python
"""Times dbcsr_multiply_dense (dbcsr_amd/operations.py; kernels of dbcsr_amd/csrc/mm_spmm.h) against the routes that served the product before it and
writes profiles/multiply_dense.txt.  One process; every variant is warmed, then the variants of a width alternate round by round; reported are median,
min, max and spread = (max - min) / median over the samples.  A sample of an asynchronous call is the mean of `calls` calls between two device events; a
sample of a route that synchronises by itself (dbcsr_create_from_dense) is a host clock around it, ended by a device synchronise.
TFLOP/s = 2 * stored elements of A * columns / time (complex data: 8 *).

Workload: A is the operand shape of the benchmark's config 2 -- uniform 23 x 23 blocks, n = 32775, one block in ten stored --, Y = A X with X of 16, 32,
48, 64, 256 and 1024 columns, float64, row by row and column by column; one float32 and one complex128 line at 256 columns.  Yardsticks, all in the same run:
    dbcsr_multivec at the same width (row by row; for the column-by-column case plus the two transposing copy_ calls it would need);
    dbcsr_create_from_dense -> dbcsr_multiply -> dbcsr_to_dense;
    dbcsr_rank_update at the same width: the same flop count in the opposite direction.
--block-product-tflops: the rate bench.py reported in the same session, for the fraction; without it the fraction is not reported."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dbcsr_amd.matrix import DbcsrMatrix  # noqa: E402
from dbcsr_amd.multiply import MultiplyEngine, dbcsr_multiply  # noqa: E402
from dbcsr_amd.operations import (dbcsr_create_from_dense, dbcsr_multiply_dense, dbcsr_multivec, dbcsr_rank_update,  # noqa: E402
                                  dbcsr_to_dense)

LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def stat_line(name, samples, flop):
    med = float(np.median(samples))
    say("  %-34s median %9.4f ms  min %9.4f  max %9.4f  spread %5.1f %%  %7.3f TFLOP/s   samples: %s"
        % (name, med, min(samples), max(samples), 100.0 * (max(samples) - min(samples)) / med, flop / med / 1e9, " ".join("%.4f" % s for s in samples)))
    return med


def device_sample(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def host_sample(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / calls


def alternate(variants, rounds, warm):
    """{name: samples}: the variants (name, fn, sampler, calls) take turns, round by round"""
    out = {name: [] for name, _, _, _ in variants}
    for r in range(warm + rounds):
        for name, fn, sample, calls in variants:
            s = sample(fn, calls)
            if r >= warm:
                out[name].append(s)
    return out


def matrix(nb, bs, fill, seed, dtype):
    """nb x nb blocks of bs x bs, about `fill` of them stored, random values; built on the device, packed"""
    dev = torch.device("cuda")
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    sizes = torch.full((nb,), bs, dtype=torch.int32, device=dev)
    idx = torch.nonzero(torch.rand(nb * nb, device=dev, generator=g) < fill).flatten()
    rows, cols = idx // nb, idx % nb
    row_p = torch.zeros(nb + 1, dtype=torch.int32, device=dev)
    row_p[1:] = torch.cumsum(torch.bincount(rows, minlength=nb), 0).to(torch.int32)
    blk_p = torch.arange(idx.numel(), dtype=torch.int64, device=dev) * (bs * bs)
    data = torch.randn(idx.numel() * bs * bs, dtype=dtype, device=dev, generator=g)
    return DbcsrMatrix(sizes, sizes, row_p, cols.to(torch.int32).contiguous(), blk_p, data)


def column_blocks(ncol, bs, dev):
    sizes = [bs] * (ncol // bs) + ([ncol % bs] if ncol % bs else [])
    return torch.as_tensor(np.asarray(sizes, np.int32)).to(dev)


def one_width(E, A, ncol, rounds, warm, calls, yardsticks):
    """the medians {name: ms} of one width"""
    dev, n = A.row_p.device, 23 * A.nblkrows
    flop = (8.0 if A.dtype.is_complex else 2.0) * A.data.numel() * ncol   # (a complex product and sum are four real ones of each)
    g = torch.Generator(device=dev)
    g.manual_seed(7 + ncol)
    X = torch.randn((n, ncol), dtype=A.dtype, device=dev, generator=g)
    Y = torch.empty_like(X)
    Xc, Yc = torch.empty((ncol, n), dtype=A.dtype, device=dev).t(), torch.empty((ncol, n), dtype=A.dtype, device=dev).t()
    Xc.copy_(X)
    variants = [("multiply_dense, row by row", lambda: dbcsr_multiply_dense(A, X, Y, engine=E), device_sample, calls),
                ("multiply_dense, column by column", lambda: dbcsr_multiply_dense(A, Xc, Yc, engine=E), device_sample, calls)]
    if yardsticks:
        Xr, Ym = torch.empty_like(X), torch.empty_like(X)

        def multivec_from_columns():
            Xr.copy_(Xc)
            dbcsr_multivec(A, Xr, Ym, engine=E)
            Yc.copy_(Ym)
        cols = column_blocks(ncol, 23, dev)
        B = A.copy()

        def block_route():
            Xb = dbcsr_create_from_dense(X, A.col_blk_size, cols, engine=E)
            Cb = DbcsrMatrix.empty_like_pattern(A.row_blk_size, cols, A.dtype, device=dev)
            dbcsr_multiply("N", "N", 1.0, A, Xb, 0.0, Cb, engine=E)
            return dbcsr_to_dense(Cb, engine=E)
        variants += [("multivec (row by row)", lambda: dbcsr_multivec(A, X, Ym, engine=E), device_sample, calls),
                     ("multivec + two transposing copy_", multivec_from_columns, device_sample, calls),
                     ("from_dense -> multiply -> to_dense", block_route, host_sample, 1),
                     ("rank_update (opposite direction)", lambda: dbcsr_rank_update(B, X, X, 1.0, 0.0, engine=E), device_sample, calls)]
    got = alternate(variants, rounds, warm)
    med = {name: stat_line(name, got[name], flop) for name, _, _, _ in variants}
    if yardsticks:
        ref = dbcsr_multivec(A, X, engine=E)
        scale = float(ref.abs().max())
        dbcsr_multiply_dense(A, X, Y, engine=E)
        dbcsr_multiply_dense(A, Xc, Yc, engine=E)
        say("  agreement with multivec, max |difference| / max |Y|: row by row %.2e, column by column %.2e"
            % (float((Y - ref).abs().max()) / scale, float((Yc - ref).abs().max()) / scale))
    return med, flop


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nb", type=int, default=1425)
    ap.add_argument("--fill", type=float, default=0.10)
    ap.add_argument("--widths", type=int, nargs="+", default=[16, 32, 48, 64, 256, 1024])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--block-product-tflops", type=float, default=None)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "multiply_dense.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU: there is no fallback"
    E = MultiplyEngine()
    A = matrix(a.nb, 23, a.fill, 1, torch.float64)
    say("dbcsr_multiply_dense, Y = A X; A: %d x %d blocks of 23 x 23 (n = %d), %d stored (fill %.3f), float64; %s"
        % (a.nb, a.nb, 23 * a.nb, A.nblks, A.nblks / float(a.nb * a.nb), torch.cuda.get_device_name(0)))
    say("%d alternations after %d warm-up round(s), %d calls per device-event sample, 1 call per host-clock sample; ms per call; "
        "TFLOP/s = 2 * stored elements * columns / time (complex data: 8 *)" % (a.rounds, a.warm, a.calls))
    if a.block_product_tflops:
        say("block-product rate of bench.py in the same session: %.2f TFLOP/s" % a.block_product_tflops)
    say()
    ratios = []
    for ncol in a.widths:
        say("%d columns" % ncol)
        med, flop = one_width(E, A, ncol, a.rounds, a.warm, a.calls, True)
        row, col = med["multiply_dense, row by row"], med["multiply_dense, column by column"]
        r_mv, c_mv = row / med["multivec (row by row)"], col / med["multivec + two transposing copy_"]
        ratios.append((ncol, r_mv))
        say("  ratios (median / median): row by row / multivec %.3f; column by column / (multivec + copies) %.3f; row by row / block route %.3f; "
            "row by row / rank_update %.3f; column by column / row by row %.3f"
            % (r_mv, c_mv, row / med["from_dense -> multiply -> to_dense"], row / med["rank_update (opposite direction)"], col / row))
        if a.block_product_tflops:
            say("  fraction of the block-product rate: row by row %.3f, column by column %.3f"
                % (flop / row / 1e9 / a.block_product_tflops, flop / col / 1e9 / a.block_product_tflops))
        say()
    wins = [n for n, r in ratios if r < 1.0]
    loses = [n for n, r in ratios if r >= 1.0]
    say("against dbcsr_multivec, row by row: faster at %s columns, not faster at %s columns (of the widths measured)"
        % (", ".join(map(str, wins)) or "none of the", ", ".join(map(str, loses)) or "none of the"))
    say()
    for dtype, label in ((torch.float32, "float32"), (torch.complex128, "complex128")):
        del A
        torch.cuda.empty_cache()
        A = matrix(a.nb, 23, a.fill, 1, dtype)
        say("%s, 256 columns" % label)
        one_width(E, A, 256, a.rounds, a.warm, a.calls, False)
        say()
    say("what bounds the kernel: not measured (no counter pass was made)")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
