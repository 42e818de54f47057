#!/usr/bin/env python3
"""Time of the complex_8 twin / desymmetrize fill (dbcsr_amd_bcsr_twin_apply with 16-byte elements: twin_fill_z64) next to a device-to-device copy of
the same byte count, in the same process, alternating:

    python tools/twin_bench.py --n 32768 --fill 0.1 --blocks 23 32 --alternations 7 --warmup 2

The matrix is the stored triangle (row <= column, diagonal included) of an n x n complex matrix of uniform b x b blocks at the given fill, desymmetrized
as a hermitian matrix (mode 0, kind 2).  A sample is `--reps` applies back to back between two device events, divided by reps; the index work
(dbcsr_amd_bcsr_twin_count) is done once before and is not timed.  Bytes are counted from the shapes: 16 * (elements read + elements written), index
arrays left out.  The torch copy moves the same number of bytes (a copy of half of them: it reads and writes each).  Spread = (max - min) / median over
the samples.  profiles/hermitian_twin.txt holds the run of this tool that chose the kernel (then with a second column, desym_fill<z64>)."""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dbcsr_amd import lib as L  # noqa: E402
from dbcsr_amd.matrix import DbcsrMatrix, StreamHandle  # noqa: E402
from dbcsr_amd.multiply import MultiplyEngine  # noqa: E402


def stored_triangle(n, b, fill, seed):
    nb = n // b
    rng = np.random.default_rng(seed)
    mask = np.triu(rng.random((nb, nb)) < fill)
    rows, cols = np.nonzero(mask)
    row_p = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=nb))]).astype(np.int32)
    sizes = torch.full((nb,), b, dtype=torch.int32, device="cuda")
    data = torch.view_as_complex(torch.rand(len(rows) * b * b, 2, dtype=torch.float64, device="cuda") - 0.5)
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda()
    return DbcsrMatrix(sizes, sizes, t(row_p, torch.int32), t(cols, torch.int32), t(np.arange(len(rows), dtype=np.int64) * b * b, torch.int64), data, "triangle")


def prepared(E, M):
    """(src descriptor, dst matrix, dst descriptor) after the counting pass of E: what dbcsr_amd_bcsr_twin_apply needs"""
    st = StreamHandle()
    src = M.desc()
    row_p = torch.empty(M.nblkrows + 1, dtype=torch.int32, device="cuda")
    nb, nz = C.c_int64(0), C.c_int64(0)
    assert E.L.dbcsr_amd_bcsr_twin_count(E.h, C.byref(src), 0, row_p.data_ptr(), C.byref(nb), C.byref(nz), st.ptr) == 0
    out = DbcsrMatrix(M.row_blk_size, M.col_blk_size, row_p, torch.empty(nb.value, dtype=torch.int32, device="cuda"),
                      torch.empty(nb.value, dtype=torch.int64, device="cuda"), torch.empty(nz.value, dtype=M.dtype, device="cuda"), "full")
    return src, out, out.desc(out=True)


def sample(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--fill", type=float, default=0.1)
    ap.add_argument("--blocks", type=int, nargs="+", default=[23, 32])
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "twin_bench.py measures on the GPU"
    lines = []
    say = lambda s: (print(s, flush=True), lines.append(s))
    say("complex_8 twin fill, mode 0 (desymmetrize), kind 2 (hermitian): stored triangle of a %d^2 matrix at %.0f %% fill; %s"
        % (args.n, 100 * args.fill, torch.cuda.get_device_name(0)))
    say("%d alternations after %d warm-up rounds, %d applies per sample; ms per apply; GB/s = 16 * (elements read + written) / time" % (args.alternations, args.warmup, args.reps))
    E, st = MultiplyEngine(), StreamHandle()
    for b in args.blocks:
        M = stored_triangle(args.n, b, args.fill, seed=b)
        src, out, dst = prepared(E, M)
        nbytes = 16 * (M.nze + out.nze)
        cp_src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
        cp_dst = torch.empty_like(cp_src)
        fill = lambda: E.L.dbcsr_amd_bcsr_twin_apply(E.h, L.dbcsr_type_complex_8, C.byref(src), 0, 2, C.byref(dst), st.ptr)
        run = {"fill": fill, "copy": lambda: cp_dst.copy_(cp_src)}
        times = {k: [] for k in run}
        assert fill() == 0
        for step in range(args.warmup + args.alternations):
            for k in run:
                t = sample(run[k], args.reps)
                if step >= args.warmup:
                    times[k].append(t)
        say("")
        say("%d x %d blocks: %d block rows, %d stored blocks (%.1f MB) -> %d blocks (%.1f MB); %.1f MB moved per apply"
            % (b, b, M.nblkrows, M.nblks, 16e-6 * M.nze, out.nblks, 16e-6 * out.nze, 1e-6 * nbytes))
        med = {}
        for k in run:
            v = sorted(times[k])
            med[k] = v[len(v) // 2]
            say("  %-5s  median %8.4f ms  min %8.4f  max %8.4f  spread %5.1f %%  %8.1f GB/s   samples: %s"
                % (k, med[k], v[0], v[-1], 100 * (v[-1] - v[0]) / med[k], 1e-6 * nbytes / med[k], " ".join("%.4f" % x for x in times[k])))
        say("  fill against the copy: %.2f of its rate" % (med["copy"] / med["fill"]))
        del cp_src, cp_dst, M, out
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
