#!/usr/bin/env python3
"""Time of the complex_8 multiply (kernel family mm_numeric_z64) against what the real kernels can do for the same product: the four real
fp64 multiplies ArBr, AiBi, ArBi, AiBr of the same pattern (mm_numeric_f64_hot<b,b,b> for a cube of b = 9 ... 32), in the same process,
alternating.

    python tools/complex_bench.py --sizes 8192 16384 --block 23 --fill 0.1 --steps 5 --warmup 2

Per size it prints the kernel times of both (dbcsr_amd_mm_timing: HIP events around the block kernel, warm plan), the wall time of both
between HIP events on the stream, the achieved fraction of the fp64 MFMA peak (a complex product of m x n x k counts 8 m n k real flop,
four times what the engine's flop counter says), and how far the two results are apart.  One JSON line per size at the end."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dbcsr_amd.matrix import DbcsrMatrix  # noqa: E402
from dbcsr_amd.multiply import MultiplyEngine  # noqa: E402
from dbcsr_amd.randmat import perf_matrices  # noqa: E402

FP64_MFMA_PEAK = 76.5e12   # measured with v_mfma_f64_4x4x4_4b on this chip (profiles/r01_ubench_fp64_mfma.txt)


def real_part(M, which, sign=1.0):
    d = torch.view_as_real(M.data)[:, which]
    return DbcsrMatrix(M.row_blk_size, M.col_blk_size, M.row_p, M.col_i, M.blk_p, (d * sign).contiguous(), M.name)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return out, e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[8192, 16384])
    ap.add_argument("--block", type=int, default=23)
    ap.add_argument("--fill", type=float, default=0.1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    results = []
    for n in args.sizes:
        mix, sp = [1, args.block], 1.0 - args.fill
        ez = MultiplyEngine()
        A, B, Cm = perf_matrices(n, n, n, (sp, sp, sp), mix, mix, mix, dtype=torch.complex128, engine=ez)
        Ar, Ai, Ain = real_part(A, 0), real_part(A, 1), real_part(A, 1, -1.0)
        Br, Bi = real_part(B, 0), real_part(B, 1)
        Cr, Ci = real_part(Cm, 0), real_part(Cm, 1)
        er = [MultiplyEngine() for _ in range(4)]   # one engine per real multiply: each keeps its plan warm, as the complex engine does

        def complex_multiply():
            out, counts = ez.multiply_local(1.0, A, B, 1.0, Cm)
            return out, counts, ez.last_timing()[1]

        def four_real_multiplies():
            kern = 0.0
            re1, counts = er[0].multiply_local(1.0, Ar, Br, 1.0, Cr)      # Re = Cr + Ar Br - Ai Bi
            kern += er[0].last_timing()[1]
            re2, _ = er[1].multiply_local(1.0, Ain, Bi, 1.0, re1)
            kern += er[1].last_timing()[1]
            im1, _ = er[2].multiply_local(1.0, Ar, Bi, 1.0, Ci)           # Im = Ci + Ar Bi + Ai Br
            kern += er[2].last_timing()[1]
            im2, _ = er[3].multiply_local(1.0, Ai, Br, 1.0, im1)
            kern += er[3].last_timing()[1]
            return (re2, im2), counts, kern

        tz, tr, kz, kr = [], [], [], []
        for step in range(args.warmup + args.steps):
            (zout, zc, k1), w1 = timed(complex_multiply)
            ((re, im), rc, k2), w2 = timed(four_real_multiplies)
            if step >= args.warmup:
                tz.append(w1), tr.append(w2), kz.append(k1), kr.append(k2)
        assert zc.flop == rc.flop and zc.c_nblks == rc.c_nblks
        zr = torch.view_as_real(zout.data)
        scale = float(zr.abs().max())
        apart = max(float((zr[:, 0] - re.data).abs().max()), float((zr[:, 1] - im.data).abs().max())) / scale
        med = lambda v: sorted(v)[len(v) // 2]
        r = {"n": n, "block": args.block, "fill": args.fill, "c_nblks": int(zc.c_nblks), "products": int(zc.nproducts), "real_flop_of_the_complex_product": 4 * int(zc.flop),
             "complex_kernel": ez.last_kernel(), "real_kernel": er[0].last_kernel(),
             "complex_kernel_ms": med(kz), "four_real_kernels_ms": med(kr), "complex_wall_ms": med(tz), "four_real_wall_ms": med(tr),
             "complex_fraction_of_fp64_mfma_peak": 4 * zc.flop / (med(kz) * 1e-3) / FP64_MFMA_PEAK,
             "four_real_fraction_of_fp64_mfma_peak": 4 * zc.flop / (med(kr) * 1e-3) / FP64_MFMA_PEAK,
             "results_apart_relative_to_largest_element": apart}
        print("%d^2, %d^3 blocks at %.0f %% fill: %s %.3f ms kernel (%.3f wall, %.3f of the fp64 MFMA peak) against four %s %.3f ms kernel (%.3f wall, %.3f of peak); "
              "results %.1e apart" % (n, args.block, 100 * args.fill, r["complex_kernel"], r["complex_kernel_ms"], r["complex_wall_ms"],
                                      r["complex_fraction_of_fp64_mfma_peak"], r["real_kernel"], r["four_real_kernels_ms"], r["four_real_wall_ms"],
                                      r["four_real_fraction_of_fp64_mfma_peak"], apart))
        results.append(r)
        del A, B, Cm, Ar, Ai, Ain, Br, Bi, Cr, Ci, zout, re, im, ez, er
        torch.cuda.empty_cache()
    for r in results:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
