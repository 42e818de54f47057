#!/usr/bin/env python3
"""Times of the matrix algebra between multiplies (dbcsr_amd/operations.py, kernels of dbcsr_amd/csrc/mm_algebra.h) on matrices of the shape of
config 2's product (n x n, uniform b x b blocks; BASELINE.json: 32768, 23), next to torch kernels that move the same bytes, in the same process,
alternating:

    python tools/ops_bench.py --n 32768 --block 23 --alternations 7 --warmup 2 --out profiles/matrix_ops.txt

  flat        dbcsr_add on the same pattern (A <- A + beta B in place): the comparison of the two indices on the device with its synchronisation
              (flat.count: dbcsr_amd_bcsr_add_count alone) and the flat pass algebra_add_flat; pattern fill --fill-flat
  torch.add   torch.add(a.data, b.data, alpha=beta, out=a.data) on the two flat data tensors: the same bytes through a kernel that is not ours
  general     dbcsr_amd_bcsr_add_count + _add_apply at 50 % pattern overlap (A and B of fill --fill-general, half of each one's blocks in the other):
              bitmaps, union, scans, one synchronisation, index emission, algebra_add_blocks; dst allocated once
  apply       of that, the part after the count's synchronisation (index emission + algebra_add_blocks), from the difference to a count alone
  norm        dbcsr_amd_bcsr_norm2 of A (algebra_norm2 + the final sum + one synchronisation)
  torch.norm  torch.linalg.vector_norm(a.data): the same bytes read
  gersh.N     dbcsr_amd_bcsr_gershgorin of A without symmetry: the row sums of |x| (algebra_row_sums), the sum of the partial vectors, the maximum, one
              synchronisation.  Yardstick: norm (the same bytes read by algebra_norm2, the same run)
  gersh.S     the same of the stored upper triangle T of a symmetric matrix: row sums plus the column sums of the blocks off the diagonal (the per-column
              block lists, algebra_col_sums) -- T's data is read twice.  Yardstick: norm.T, dbcsr_amd_bcsr_norm2 of T (read once)
  colnorm     dbcsr_amd_bcsr_col_sums of |x|^2 of A (lists + algebra_col_sums + the sum of the partial vectors; asynchronous).  Yardstick: norm
  maxabs      dbcsr_amd_bcsr_maxabs of A.  Yardstick: norm
  scale.R/.L  dbcsr_amd_bcsr_scale_by_vector of A on the right / left with a vector of ones (A is read and written)
  torch.mul   torch.mul(a.data, s, out=a.data) with a scalar: the same bytes through a kernel that is not ours, the yardstick of scale.R / scale.L

  matvec.N/.T dbcsr_amd_bcsr_matvec of A with a vector of ones, y <- A x and y <- A^T x (element offsets, algebra_matvec_rows or the per-column lists and
              algebra_matvec_cols, algebra_matvec_combine; asynchronous).  Yardstick: norm
  matvec.S    the same of the stored triangle T as a symmetric matrix (row pass plus column pass off the diagonal: T's data is read twice).  Yardstick: norm.T

With --matvec only norm, norm.T, the three matvec rows and the sums they are made from (gersh.N: the row pass without the reads of x; colnorm: the column
pass without them; gersh.S: both) are timed, alternating, and the report has the ratios of the matvec rows alone:

    python tools/ops_bench.py --matvec --alternations 7 --warmup 2 --out profiles/matrix_vector.txt

With --colsums (lab build: DBCSR_AMD_LAB=1) only this is timed, alternating: norm, and dbcsr_amd_bcsr_col_sums of |x|^2 of A through an engine per form of
algebra_col_sums (DBCSR_AMD_ALG_COLSUMS; csrc/mm_algebra.h): col.0 what ships, col.1 staging without the per-lane add loop, col.2 loads added in registers
without LDS, col.3 no block walked (list build, launch, sum of the partial vectors), col.4 the lane-per-column form without staging; col.lists is col.3.

With --multivec only the matrix times several dense vectors is timed (dbcsr_amd_bcsr_multivec, kernels of dbcsr_amd/csrc/mm_multivec.h), alternating with
its yardsticks: norm (one read of A), matvec.N / matvec.T (the existing code, one right-hand side per call), multivec.N at nrhs 1, 4, 8, 16, 32, 64,
multivec.T at 8 and 16, multivec.S at 16 (the stored triangle T as a symmetric matrix) against norm.T.  X is a contiguous (n, nrhs) tensor of ones.  The
report has multivec(k) / norm, the time per column multivec(k) / k, the condition multivec(k) < k * matvec for k >= 4 in every alternation, and the split
S with the volume of the partial matrices:

    python tools/ops_bench.py --multivec --alternations 7 --warmup 2 --out profiles/matrix_multivec.txt

With DBCSR_AMD_LAB=1 it also times multivec.N at 32 and 64 through an engine with DBCSR_AMD_MULTIVEC_WAVES=1 (rows ind.N: independent waves, every
tile of 16 right-hand sides loads the block itself, against the shared staging of what ships).

With --rank-update only the rank-k update on the stored pattern is timed (dbcsr_amd_bcsr_rank_update, kernels of dbcsr_amd/csrc/mm_rank_update.h),
alternating with its yardsticks: scale (dbcsr_amd_bcsr_scale_window of the whole matrix: A read and written once, the same traffic), norm (one read of A),
rank(k) = A <- 0.5 A + 1e-3 X Y^T at nrhs 1, 4, 16, 64, 256 and rank.xx(64) with Y = X (the same pointer).  X and Y are contiguous (n, k) tensors of
ones (ld = k; a run stops when the self-check -- alpha = 1, beta = 0 gives nrhs in every element -- fails).  The report has rank(k) / scale, 2 nze nrhs / time in TFLOP/s -- and, with --mfma-tflops T (the fp64 MFMA figure bench.py --full
measured in the same session: roofline.achieved of its block-product kernel), the fraction of T -- and the condition rank(k) < k * rank(1) for k = 4, 16, 64
in every alternation:

    python tools/ops_bench.py --rank-update --alternations 7 --warmup 2 --mfma-tflops T --out profiles/rank_update.txt

With --block-scale only the block diagonal applied to a matrix is timed (dbcsr_scale_by_block_diag; kernels of dbcsr_amd/csrc/mm_block_scale.h) on the
standard matrix (--n / --block, full as config 2's product is) and on blocks of 32: the left, right and both passes against dbcsr_scale of the same matrix
(the floor: A read and written once) and against what replaces it without the kernel, dbcsr_multiply(D, A -> C) with a warm plan and with a cold one
(DBCSR_AMD_MM_PLAN=0), all alternating in one process; 2 nze b / time against --mfma-tflops.

    python tools/ops_bench.py --block-scale --alternations 7 --warmup 2 --mfma-tflops T --out profiles/block_scale.txt

With --block-inverse only the block diagonal is timed (dbcsr_get_block_diag, dbcsr_invert_block_diag; kernels of dbcsr_amd/csrc/mm_block_inverse.h) on
1424 diagonal blocks of 23 x 23 (the diagonal of config 2's product shape), 32, 64 and 96, float64, alternating: get_block_diag of a matrix with eight more
blocks per block row, invert_block_diag without and with the check, dbcsr_scale of the block diagonal as the fixed cost of one launch, the device path
get_block_diag + invert_block_diag(check=True), the host round trip it replaces (to_host, numpy.linalg.inv of the stack of diagonal blocks, upload,
synchronise) and torch.linalg.inv on the (1424, n, n) device stack.  These rows are wall-clock times around a device synchronisation (the calls that
answer on the host synchronise themselves), --reps calls per sample.  The condition: at 23 x 23 the device path is not slower than the host round trip in
any alternation:

    python tools/ops_bench.py --block-inverse --alternations 7 --warmup 2 --out profiles/block_inverse.txt

With --dense only the dense conversion is timed (dbcsr_to_dense, dbcsr_from_dense, dbcsr_create_from_dense; kernels of dbcsr_amd/csrc/mm_dense.h) on a
float64 matrix of 504 x 504 blocks of 23 x 23 (n = 11592: a dense matrix of 1.07 GB), once with every block stored and once with one block in ten,
alternating: to_dense into a row-by-row and into a column-by-column tensor, from_dense out of both, create_from_dense(eps) (a wall-clock row: it answers on
the host), and the yardsticks out.copy_(src) and out.copy_(src.T) of a dense tensor of that size (the vendor's straight and transposing copies),
torch.zeros of that size, and the host round trip the feature replaces (to_host, the block loop of oracle.Bcsr.to_dense, upload, synchronise; wall clock,
one call per sample) against dbcsr_to_dense timed the same way.  The condition: the device path is faster than the host round trip in every alternation:

    python tools/ops_bench.py --dense --alternations 7 --warmup 2 --out profiles/dense_conversion.txt

With --csr only the element CSR form is timed (dbcsr_to_csr, dbcsr_from_csr, dbcsr_create_from_csr; kernels of dbcsr_amd/csrc/mm_csr.h) on the matrix of
--dense (float64, 504 x 504 blocks of 23 x 23, every block stored and one block in ten), alternating: to_csr without eps and with an eps that drops about
half of the elements (a wall-clock row: it answers on the host), from_csr onto the same pattern, create_from_csr (wall clock, one call per sample), and the
yardsticks copy_ of the data area, dbcsr_to_dense of the same matrix, dbcsr_to_dense(...).to_sparse_csr() on the device where torch offers it (said
otherwise), and the host round trip the feature replaces (to_host, a numpy loop over the blocks, upload, synchronise; wall clock, one call per sample)
against dbcsr_to_csr timed the same way.  The condition: the device path is faster than the host round trip in every alternation:

    python tools/ops_bench.py --csr --alternations 7 --warmup 2 --out profiles/csr_conversion.txt

With --submatrix only the submatrix method's two copies are timed (dbcsr_submatrix_gather, dbcsr_submatrix_scatter; kernels of
dbcsr_amd/csrc/mm_submatrix.h) on the matrix of --dense at one block in ten: with one submatrix per block column, gather into the whole batch padded to
the largest side, scatter out of it, and zero_() of the batch as the floor of writing it; and the full-set gather (one submatrix holding every block
row) against dbcsr_to_dense of the same matrix, which moves the same bytes with the same moves, alternating in one process.  No condition: the ratio and
its spread are the result:

    python tools/ops_bench.py --submatrix --alternations 7 --warmup 2 --out profiles/submatrix.txt

With --elementwise only the element-wise operations on two patterns are timed (dbcsr_hadamard_product, dbcsr_copy with keep_sparsity,
dbcsr_function_of_elements; kernels of dbcsr_amd/csrc/mm_elementwise.h), alternating with their yardsticks: had.flat (the whole in-place call on the same
pattern: index comparison, one synchronisation, elementwise_mul_flat) against the flat dbcsr_add and torch.mul on the data areas; had.general
(dbcsr_amd_bcsr_hadamard_count + _apply at 50 % overlap, dst allocated once; had.count: the count with its synchronisation alone) against the union add
of the same pair (general / count of the standard report); copy_onto (B onto A's equal pattern) against A.data.copy_(B.data); function (tanh, in
place) against torch.tanh_ on the data area.  No condition: times, ratios and their spread are the result:

    python tools/ops_bench.py --elementwise --alternations 7 --warmup 2 --out profiles/elementwise.txt

With --blocks only the block lists are timed (dbcsr_reserve_blocks, dbcsr_put_blocks, dbcsr_get_blocks; kernels of dbcsr_amd/csrc/mm_blocklist.h),
alternating with their yardsticks, on the full pattern unless said otherwise and through the C entries: put.over (every block overwritten from a list in
random order, the source packed in list order: locate, group, apply) and get (every block into windows in list order) against copy_onto
(dbcsr_copy(keep_sparsity=True) between two matrices of that pattern) and torch.copy_ of the data area; put.sum (summation) against the flat dbcsr_add;
put.python: the whole dbcsr_put_blocks(keep_sparsity=True) call with the window checks torch does in front of it; reserve.general (count + apply of a
list that is the general pair's B pattern onto the general pair's A: half of it new) and reserve.count against add.general and add.count of that pair;
reserve.none (a count over the whole pattern in random order that finds nothing to create) against add.count of two matrices of the same pattern;
create (dbcsr_create_from_blocks from that list and source, one call per sample, by the host's clock) against from_host of the same matrix from
pageable numpy arrays, its host-to-device copy included.  No condition: times, ratios and their spread are the result:

    python tools/ops_bench.py --blocks --alternations 7 --warmup 2 --out profiles/block_lists.txt

A sample is `--reps` calls back to back between two device events, divided by reps.  Bytes are counted from the shapes: 8 * (elements read + elements
written) of the data areas, index arrays left out.  Spread = (max - min) / median over the samples."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dbcsr_amd import lib as L  # noqa: E402
from dbcsr_amd.matrix import DbcsrMatrix, StreamHandle  # noqa: E402
from dbcsr_amd.multiply import MultiplyEngine, dbcsr_multiply  # noqa: E402
from dbcsr_amd.operations import dbcsr_add, dbcsr_get_block_diag, dbcsr_invert_block_diag, dbcsr_scale, dbcsr_scale_by_block_diag  # noqa: E402
from dbcsr_amd.operations import dbcsr_create_from_dense, dbcsr_from_dense, dbcsr_to_dense  # noqa: E402
from dbcsr_amd.operations import dbcsr_func_tanh, dbcsr_hadamard_product  # noqa: E402
from dbcsr_amd.operations import dbcsr_create_from_blocks, dbcsr_put_blocks  # noqa: E402
from dbcsr_amd.submatrix import dbcsr_submatrix_gather, dbcsr_submatrix_plan, dbcsr_submatrix_scatter  # noqa: E402


def matrix_of(mask, b, seed):
    """uniform b x b blocks on the pattern `mask` (block rows x block columns), packed, uniform(-0.5, 0.5) values made on the device"""
    nb = mask.shape[0]
    rows, cols = np.nonzero(mask)
    row_p = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=nb))]).astype(np.int32)
    sizes = torch.full((nb,), b, dtype=torch.int32, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(seed)
    data = torch.rand(len(rows) * b * b, dtype=torch.float64, device="cuda", generator=g) - 0.5
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda()
    return DbcsrMatrix(sizes, sizes, t(row_p, torch.int32), t(cols, torch.int32), t(np.arange(len(rows), dtype=np.int64) * b * b, torch.int64), data)


def sample(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def colsums(args, say, lines, rng, b, nb, st):
    assert L.want_lab(), "--colsums needs the lab build (DBCSR_AMD_LAB=1)"
    A = matrix_of(rng.random((nb, nb)) < args.fill_flat, b, 1)
    a = A.desc()
    f64 = L.dbcsr_type_real_8
    out2 = (C.c_double * 2)()
    colv = torch.empty(nb * b, dtype=torch.float64, device="cuda")
    engines = {}
    for v in range(5):
        os.environ["DBCSR_AMD_ALG_COLSUMS"] = str(v)
        engines[v] = MultiplyEngine(lab=True)
    del os.environ["DBCSR_AMD_ALG_COLSUMS"]
    check = lambda rc: rc == 0 or sys.exit("a library call failed (%d)" % rc)
    run = {"norm": lambda: check(engines[0].L.dbcsr_amd_bcsr_norm2(engines[0].h, f64, C.byref(a), 0, out2, st.ptr))}
    for v in range(5):
        run["col.%d" % v] = (lambda e: lambda: check(e.L.dbcsr_amd_bcsr_col_sums(e.h, f64, C.byref(a), 1, 0, colv.data_ptr(), colv.numel(), st.ptr)))(engines[v])
    check(engines[0].L.dbcsr_amd_bcsr_col_sums(engines[0].h, f64, C.byref(a), 1, 0, colv.data_ptr(), colv.numel(), st.ptr))
    ref = colv.clone()
    check(engines[4].L.dbcsr_amd_bcsr_col_sums(engines[4].h, f64, C.byref(a), 1, 0, colv.data_ptr(), colv.numel(), st.ptr))
    torch.cuda.synchronize()
    say("col.4 against col.0: largest relative difference of a column sum %.2e" % float(((colv - ref).abs() / ref).max()))
    times = {k: [] for k in run}
    for step in range(args.warmup + args.alternations):
        for k in run:
            t = sample(run[k], args.reps)
            if step >= args.warmup:
                times[k].append(t)
    say("")
    say("forms of algebra_col_sums, %d blocks, %.1f MB" % (A.nblks, 8e-6 * A.nze))
    med = {}
    for k in run:
        v = sorted(times[k])
        med[k] = v[len(v) // 2]
        say("  %-6s  median %8.4f ms  min %8.4f  max %8.4f  spread %5.1f %%  %.2f of norm   samples: %s"
            % (k, med[k], v[0], v[-1], 100 * (v[-1] - v[0]) / med[k], med[k] / med["norm"], " ".join("%.4f" % x for x in times[k])))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def multivec(args, say, lines, rng, b, nb, st):
    lab = L.want_lab()
    E = MultiplyEngine(lab=True) if lab else MultiplyEngine()
    mask = rng.random((nb, nb)) < args.fill_flat
    A, T = matrix_of(mask, b, 1), matrix_of(np.triu(mask), b, 5)
    a, t_ = A.desc(), T.desc()
    f64 = L.dbcsr_type_real_8
    n = nb * b
    one, zero = (C.c_double * 2)(1.0, 0.0), (C.c_double * 2)(0.0, 0.0)
    out2 = (C.c_double * 2)()
    ones = torch.ones(n, dtype=torch.float64, device="cuda")
    colv = torch.empty(n, dtype=torch.float64, device="cuda")
    kmax = 64
    X = torch.ones(n * kmax, dtype=torch.float64, device="cuda")
    Y = torch.empty(n * kmax, dtype=torch.float64, device="cuda")
    check = lambda rc: rc == 0 or sys.exit("a library call failed (%d)" % rc)

    def mv(e, trans, d, kind, k):
        return lambda: check(e.L.dbcsr_amd_bcsr_multivec(e.h, f64, trans, one, C.byref(d), kind, k, X.data_ptr(), n, k, zero, Y.data_ptr(), n, k, st.ptr))

    run = {
        "norm": lambda: check(E.L.dbcsr_amd_bcsr_norm2(E.h, f64, C.byref(a), 0, out2, st.ptr)),
        "norm.T": lambda: check(E.L.dbcsr_amd_bcsr_norm2(E.h, f64, C.byref(t_), 1, out2, st.ptr)),
        "matvec.N": lambda: check(E.L.dbcsr_amd_bcsr_matvec(E.h, f64, b"N", one, C.byref(a), -1, ones.data_ptr(), n, zero, colv.data_ptr(), n, st.ptr)),
        "matvec.T": lambda: check(E.L.dbcsr_amd_bcsr_matvec(E.h, f64, b"T", one, C.byref(a), -1, ones.data_ptr(), n, zero, colv.data_ptr(), n, st.ptr)),
    }
    width = {}
    for k in (1, 4, 8, 16, 32, 64):
        run["multivec.N.%d" % k] = mv(E, b"N", a, -1, k)
        width["multivec.N.%d" % k] = k
    for k in (8, 16):
        run["multivec.T.%d" % k] = mv(E, b"T", a, -1, k)
        width["multivec.T.%d" % k] = k
    run["multivec.S.16"] = mv(E, b"N", t_, 0, 16)
    width["multivec.S.16"] = 16
    if lab:
        os.environ["DBCSR_AMD_MULTIVEC_WAVES"] = "1"
        E1 = MultiplyEngine(lab=True)
        del os.environ["DBCSR_AMD_MULTIVEC_WAVES"]
        for k in (32, 64):
            run["ind.N.%d" % k] = mv(E1, b"N", a, -1, k)
            width["ind.N.%d" % k] = k
    # the product of ones: every row of A x, in every column, is the row sum; the multivec and the matvec must agree on it to rounding
    run["matvec.N"]()
    run["multivec.N.64"]()
    torch.cuda.synchronize()
    worst = float((Y.view(n, kmax) - colv[:, None]).abs().max() / colv.abs().max())
    say("multivec.N.64 against matvec.N on vectors of ones: largest difference %.2e of the largest row sum" % worst)
    times = {k: [] for k in run}
    for step in range(args.warmup + args.alternations):
        for k in run:
            t = sample(run[k], args.reps)
            if step >= args.warmup:
                times[k].append(t)
    say("")
    say("A: %d blocks, %.1f MB; T (stored triangle): %d blocks, %.1f MB" % (A.nblks, 8e-6 * A.nze, T.nblks, 8e-6 * T.nze))
    med = {}
    for k in run:
        v = sorted(times[k])
        med[k] = v[len(v) // 2]
        nbytes = (16 if k.endswith(".S.16") else 8) * (T.nze if (k == "norm.T" or ".S." in k) else A.nze)
        say("  %-14s  median %8.4f ms  min %8.4f  max %8.4f  spread %5.1f %%  %8.1f GB/s   samples: %s"
            % (k, med[k], v[0], v[-1], 100 * (v[-1] - v[0]) / med[k], 1e-6 * nbytes / med[k], " ".join("%.4f" % x for x in times[k])))
    say("")
    say("time against one read of the matrix (median / median; the ratio per alternation, sample by sample), and per right-hand side")
    for k in run:
        if k not in width:
            continue
        y = "norm.T" if ".S." in k else "norm"
        r = sorted(x / z for x, z in zip(times[k], times[y]))
        say("  %-14s / %-6s  %5.2f   (per alternation %.2f ... %.2f)   %8.4f ms per column" % (k, y, med[k] / med[y], r[0], r[-1], med[k] / width[k]))
    say("")
    say("condition: multivec(k) below k * matvec in every alternation, k >= 4")
    ok = True
    for k in run:
        if k not in width or width[k] < 4 or ".S." in k or k.startswith("ind."):
            continue
        y = "matvec.T" if ".T." in k else "matvec.N"
        r = sorted(x / (width[k] * z) for x, z in zip(times[k], times[y]))
        ok = ok and r[-1] < 1.0
        say("  %-14s / (%2d * %s)  %.3f ... %.3f   %s" % (k, width[k], y, r[0], r[-1], "holds" if r[-1] < 1.0 else "FAILS"))
    say("  the condition %s" % ("holds" if ok else "FAILS"))
    say("")
    say("split S (waves per block row / column and tile; as dbcsr_amd/csrc/mm_engine_algebra.h: multivec_split) and the volume of the partial matrices")
    row_split = max(1, min(-(-65536 // nb), A.nblks // nb, 64))
    for k in (1, 4, 8, 16, 32, 64):
        tiles = -(-k // 16)
        S = max(1, -(-row_split // tiles))
        vol = 8.0 * S * n * k
        say("  nrhs %2d: %d tile(s), S = %2d, %7.1f MB written and read once = %.2f %% of A" % (k, tiles, S, 1e-6 * vol, 100.0 * vol / (8.0 * A.nze)))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def rank_update(args, say, lines, rng, b, nb, st):
    E = MultiplyEngine()
    A = matrix_of(rng.random((nb, nb)) < args.fill_flat, b, 1)
    a = A.desc()
    f64 = L.dbcsr_type_real_8
    n = nb * b
    kmax = 256
    alpha, beta, zero, one = (C.c_double * 2)(1e-3, 0.0), (C.c_double * 2)(0.5, 0.0), (C.c_double * 2)(0.0, 0.0), (C.c_double * 2)(1.0, 0.0)
    out2 = (C.c_double * 2)()
    X = torch.ones(n * kmax, dtype=torch.float64, device="cuda")
    Y = torch.ones(n * kmax, dtype=torch.float64, device="cuda")
    check = lambda rc: rc == 0 or sys.exit("a library call failed (%d)" % rc)

    def ru(k, y, al=alpha, be=beta):
        # (the first n k elements of the tensors of ones as a contiguous (n, k) tensor: ld = k)
        return lambda: check(E.L.dbcsr_amd_bcsr_rank_update(E.h, f64, b"T", al, k, X.data_ptr(), n, k, y.data_ptr(), n, k, be, C.byref(a), st.ptr))

    run = {
        "scale": lambda: check(E.L.dbcsr_amd_bcsr_scale_window(E.h, f64, C.byref(a), 0.9999, -1, -1, -1, -1, st.ptr)),
        "norm": lambda: check(E.L.dbcsr_amd_bcsr_norm2(E.h, f64, C.byref(a), 0, out2, st.ptr)),
    }
    width = {}
    for k in (1, 4, 16, 64, 256):
        run["rank.%d" % k] = ru(k, Y)
        width["rank.%d" % k] = k
    run["rank.xx.64"] = ru(64, X)
    width["rank.xx.64"] = 64
    # X and Y of ones, beta = 0, alpha = 1: every stored element is nrhs
    keep = A.data.clone()
    ru(64, Y, one, zero)()
    torch.cuda.synchronize()
    right = bool((A.data == 64.0).all().item())
    say("rank.64 with alpha = 1, beta = 0 on tensors of ones: every element of A is 64: %s" % right)
    if not right:
        sys.exit("the rank-k update is wrong: nothing is timed")
    A.data.copy_(keep)
    del keep
    times = {k: [] for k in run}
    for step in range(args.warmup + args.alternations):
        for k in run:
            t = sample(run[k], args.reps)
            if step >= args.warmup:
                times[k].append(t)
    say("")
    say("A: %d blocks, %.1f MB" % (A.nblks, 8e-6 * A.nze))
    med = {}
    for k in run:
        v = sorted(times[k])
        med[k] = v[len(v) // 2]
        nbytes = (8 if k == "norm" else 16) * A.nze
        say("  %-11s  median %8.4f ms  min %8.4f  max %8.4f  spread %5.1f %%  %8.1f GB/s of A   samples: %s"
            % (k, med[k], v[0], v[-1], 100 * (v[-1] - v[0]) / med[k], 1e-6 * nbytes / med[k], " ".join("%.4f" % x for x in times[k])))
    say("")
    say("time against dbcsr_scale (median / median; the ratio per alternation, sample by sample), and 2 nze nrhs / time"
        + (" against %.1f TFLOP/s" % args.mfma_tflops if args.mfma_tflops else ""))
    for k in width:
        r = sorted(x / z for x, z in zip(times[k], times["scale"]))
        tf = 2e-9 * A.nze * width[k] / med[k]
        say("  %-11s / scale  %6.2f   (per alternation %.2f ... %.2f)   %7.2f TFLOP/s%s"
            % (k, med[k] / med["scale"], r[0], r[-1], tf, "   %.3f of the measured MFMA figure" % (tf / args.mfma_tflops) if args.mfma_tflops else ""))
    say("")
    say("condition: rank(k) below k * rank(1) in every alternation, k = 4, 16, 64")
    ok = True
    for k in (4, 16, 64):
        r = sorted(x / (k * z) for x, z in zip(times["rank.%d" % k], times["rank.1"]))
        ok = ok and r[-1] < 1.0
        say("  rank.%-3d / (%2d * rank.1)  %.3f ... %.3f   %s" % (k, k, r[0], r[-1], "holds" if r[-1] < 1.0 else "FAILS"))
    say("  the condition %s" % ("holds" if ok else "FAILS"))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def sample_wall(fn, reps):
    """ms per call by the host's clock, the device idle before and after (for calls that answer on the host)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / reps


def block_inverse(args, say, lines, rng):
    E = MultiplyEngine()
    nb, extra = 1424, 8
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda()
    results = {}
    for b in (23, 32, 64, 96):
        # S: the diagonal blocks (uniform(-0.5, 0.5) + b / 2 on the diagonal: condition numbers of a few units, so that inverting the inverse again and
        # again stays where it is) and `extra` blocks per block row off the diagonal
        mask = np.zeros((nb, nb), bool)
        mask[np.arange(nb), np.arange(nb)] = True
        for r in range(nb):
            mask[r, rng.choice(nb, extra, replace=False)] = True
        S = matrix_of(mask, b, 10 + b)
        rows, cols = np.nonzero(mask)
        diag_at = np.flatnonzero(rows == cols)
        view, at = S.data.view(-1, b, b), torch.as_tensor(diag_at, device="cuda")
        view[at] = view[at] + 0.5 * b * torch.eye(b, dtype=torch.float64, device="cuda")
        D = dbcsr_get_block_diag(S, engine=E)
        keep = D.data.clone()
        # the inverse is one: against torch on the host, block by block
        assert dbcsr_invert_block_diag(D, engine=E) == (0, -1)
        ref = np.linalg.inv(keep.view(nb, b, b).cpu().numpy())
        err = float(np.max(np.abs(D.data.view(nb, b, b).cpu().numpy() - ref)) / np.max(np.abs(ref)))
        say("%d blocks of %d x %d: max |device - numpy.linalg.inv| / max |inverse| = %.2e" % (nb, b, b, err))
        if not err < 1e-12:
            sys.exit("the block inverse is wrong: nothing is timed")
        D.data.copy_(keep)

        def host_round_trip():
            rs, cs, row_p, col_i, blk_p, data = S.to_host()
            r_of = np.repeat(np.arange(len(rs)), np.diff(row_p))
            at = np.flatnonzero(r_of == col_i)
            blocks = np.stack([data[blk_p[i]:blk_p[i] + b * b].reshape(b, b) for i in at])
            inv = np.linalg.inv(blocks)
            X = DbcsrMatrix(S.row_blk_size, S.col_blk_size, t(np.arange(nb + 1), torch.int32), t(np.arange(nb), torch.int32),
                            t(np.arange(nb, dtype=np.int64) * b * b, torch.int64), torch.as_tensor(inv.reshape(-1)).cuda())
            torch.cuda.synchronize()
            return X

        def device_path():
            X = dbcsr_get_block_diag(S, engine=E)
            dbcsr_invert_block_diag(X, check=True, engine=E)
            return X

        stack = keep.view(nb, b, b).clone()
        run = {
            "scale": lambda: dbcsr_scale(D, 0.9999, engine=E),
            "get_block_diag": lambda: dbcsr_get_block_diag(S, engine=E),
            "invert": lambda: dbcsr_invert_block_diag(D, check=False, engine=E),
            "invert.check": lambda: dbcsr_invert_block_diag(D, check=True, engine=E),
            "device path": device_path,
        }
        if b == 23:
            run["host path"] = host_round_trip
        try:
            torch.linalg.inv(stack)
            torch.cuda.synchronize()
            run["torch.inv"] = lambda: torch.linalg.inv(stack)
        except Exception as e:   # (recorded: the yardstick is optional)
            say("torch.linalg.inv on the (%d, %d, %d) device stack does not work here: %s" % (nb, b, b, str(e).splitlines()[0][:120]))
        times = {k: [] for k in run}
        for step in range(args.warmup + args.alternations):
            for k in run:
                x = sample_wall(run[k], 1 if k == "host path" else args.reps)
                if step >= args.warmup:
                    times[k].append(x)
        say("")
        say("%d blocks of %d x %d (%.1f MB of diagonal blocks; S has %d blocks)" % (nb, b, b, 8e-6 * nb * b * b, S.nblks))
        for k in run:
            v = sorted(times[k])
            med = v[len(v) // 2]
            say("  %-15s median %8.4f ms  min %8.4f  max %8.4f  spread %5.1f %%   samples: %s"
                % (k, med, v[0], v[-1], 100 * (v[-1] - v[0]) / med, " ".join("%.4f" % x for x in times[k])))
        results[b] = times
        del S, D, keep, stack
    say("")
    say("condition: at 23 x 23 the device path (get_block_diag + invert_block_diag(check=True)) is not slower than the host round trip in any alternation")
    r = sorted(x / z for x, z in zip(results[23]["device path"], results[23]["host path"]))
    say("  device path / host path  %.4f ... %.4f   the condition %s" % (r[0], r[-1], "holds" if r[-1] <= 1.0 else "FAILS"))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def block_scale(args, say, lines, rng):
    E = MultiplyEngine()
    plan_env = os.environ.get("DBCSR_AMD_MM_PLAN")
    os.environ["DBCSR_AMD_MM_PLAN"] = "0"
    E_cold = MultiplyEngine()
    if plan_env is None:
        os.environ.pop("DBCSR_AMD_MM_PLAN", None)
    else:
        os.environ["DBCSR_AMD_MM_PLAN"] = plan_env
    results = {}
    for b in (args.block, 32):
        nb = args.n // b
        A = matrix_of(rng.random((nb, nb)) < args.fill_flat, b, 1)
        # D: I + uniform(-0.5, 0.5) / (10 b) per diagonal block -- a norm near one, so that applying it again and again stays where it is
        D = matrix_of(np.eye(nb, dtype=bool), b, 50 + b)
        D.data.mul_(0.1 / b)
        D.data.view(nb, b, b).add_(torch.eye(b, dtype=torch.float64, device="cuda"))
        Cm = matrix_of(np.zeros((nb, nb), bool), b, 3)
        # what is timed is right: the blocks of the first block row against torch (a column-major block read row by row is its transpose)
        head = int(A.row_p[1].item())
        before = A.data[:head * b * b].view(head, b, b).clone()
        dbcsr_scale_by_block_diag(A, D, "left", engine=E)
        want = before @ D.data[:b * b].view(b, b)
        err = float(((A.data[:head * b * b].view(head, b, b) - want).abs().max() / want.abs().max()).item())
        say("%d x %d blocks of %d x %d: left pass on the first block row against torch: max difference / max element = %.2e" % (nb, nb, b, b, err))
        if not err < 1e-13:
            sys.exit("the block scaling is wrong: nothing is timed")
        run = {
            "scale": lambda: dbcsr_scale(A, 0.9999, engine=E),
            "left": lambda: dbcsr_scale_by_block_diag(A, D, "left", engine=E),
            "right": lambda: dbcsr_scale_by_block_diag(A, D, "right", engine=E),
            "both": lambda: dbcsr_scale_by_block_diag(A, D, "both", engine=E),
            "multiply.warm": lambda: dbcsr_multiply("N", "N", 1.0, D, A, 0.0, Cm, engine=E),
            "multiply.cold": lambda: dbcsr_multiply("N", "N", 1.0, D, A, 0.0, Cm, engine=E_cold),
        }
        run["multiply.warm"]()
        torch.cuda.synchronize()
        times = {k: [] for k in run}
        for step in range(args.warmup + args.alternations):
            for k in run:
                x = sample(run[k], args.reps)
                if step >= args.warmup:
                    times[k].append(x)
        say("")
        say("A: %d blocks of %d x %d, %.1f MB; D: %d blocks" % (A.nblks, b, b, 8e-6 * A.nze, D.nblks))
        med = {}
        for k in run:
            v = sorted(times[k])
            med[k] = v[len(v) // 2]
            say("  %-14s median %9.4f ms  min %9.4f  max %9.4f  spread %5.1f %%  %8.1f GB/s of A   samples: %s"
                % (k, med[k], v[0], v[-1], 100 * (v[-1] - v[0]) / med[k], 1e-6 * 16 * A.nze / med[k], " ".join("%.4f" % x for x in times[k])))
        say("")
        say("time against dbcsr_scale and against the warm multiply (median / median; per alternation, sample by sample), and 2 nze b / time per pass"
            + (" against %.1f TFLOP/s" % args.mfma_tflops if args.mfma_tflops else ""))
        for k in ("left", "right", "both"):
            r = sorted(x / z for x, z in zip(times[k], times["scale"]))
            q = sorted(x / z for x, z in zip(times[k], times["multiply.warm"]))
            tf = 2e-9 * A.nze * b * (2 if k == "both" else 1) / med[k]
            say("  %-6s / scale %6.2f (%.2f ... %.2f)   / multiply.warm %6.3f (%.3f ... %.3f)   / multiply.cold %6.3f   %7.2f TFLOP/s%s"
                % (k, med[k] / med["scale"], r[0], r[-1], med[k] / med["multiply.warm"], q[0], q[-1], med[k] / med["multiply.cold"], tf,
                   "   %.3f of the measured MFMA figure" % (tf / args.mfma_tflops) if args.mfma_tflops else ""))
        results[b] = med
        del A, D, Cm, before, want
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def dense_conversion(args, say, lines, rng):
    from oracle import oracle as O
    E = MultiplyEngine()
    b, nb = 23, 504
    n = b * nb
    results = {}
    src = torch.rand((n, n), dtype=torch.float64, device="cuda") - 0.5
    out_r = torch.empty((n, n), dtype=torch.float64, device="cuda")
    out_c = torch.empty((n, n), dtype=torch.float64, device="cuda").T
    for fill in (1.0, 0.1):
        M = matrix_of(rng.random((nb, nb)) < fill, b, 40)
        # what is timed is right: against the host helper, bit for bit, on the first block rows (the whole comparison is the tests' business)
        rs, cs, row_p, col_i, blk_p, data = M.to_host()
        head = 8
        H = O.Bcsr(rs[:head], cs, row_p[:head + 1], col_i[:row_p[head]], blk_p[:row_p[head]], data).to_dense()
        for out in (out_r, out_c):
            out.fill_(float("nan"))
            dbcsr_to_dense(M, out=out, engine=E)
            if out[:head * b].cpu().numpy().tobytes() != H.tobytes() or bool(torch.isnan(out).any()):
                sys.exit("dbcsr_to_dense is wrong: nothing is timed")
        del rs, cs, row_p, col_i, blk_p, data, H
        X = M.copy()
        eps = 1e-3

        def host_round_trip():
            rs, cs, row_p, col_i, blk_p, data = M.to_host()
            D = torch.as_tensor(O.Bcsr(rs, cs, row_p, col_i, blk_p, data).to_dense()).cuda()
            torch.cuda.synchronize()
            return D

        run = {
            "copy": lambda: out_r.copy_(src),
            "copy.T": lambda: out_r.copy_(src.T),
            "zeros": lambda: torch.zeros((n, n), dtype=torch.float64, device="cuda"),
            "to_dense.rows": lambda: dbcsr_to_dense(M, out=out_r, engine=E),
            "to_dense.cols": lambda: dbcsr_to_dense(M, out=out_c, engine=E),
            "from_dense.rows": lambda: dbcsr_from_dense(out_r, X, engine=E),
            "from_dense.cols": lambda: dbcsr_from_dense(out_c, X, engine=E),
            "create(eps)": lambda: dbcsr_create_from_dense(out_r, M.row_blk_size, M.col_blk_size, eps=eps, engine=E),
            "device path": lambda: dbcsr_to_dense(M, engine=E),
            "host path": host_round_trip,
        }
        wall = ("create(eps)", "device path", "host path")
        dbcsr_to_dense(M, out=out_r, engine=E)
        dbcsr_to_dense(M, out=out_c, engine=E)
        times = {k: [] for k in run}
        for step in range(args.warmup + args.alternations):
            for k in run:
                x = sample_wall(run[k], 1 if k == "host path" else args.reps) if k in wall else sample(run[k], args.reps)
                if step >= args.warmup:
                    times[k].append(x)
        say("")
        say("%d x %d blocks of %d x %d, fill %.2f: %d blocks, %.1f MB of blocks, a dense matrix of %.1f MB" % (nb, nb, b, b, fill, M.nblks, 8e-6 * M.nze, 8e-6 * n * n))
        med = {}
        for k in run:
            v = sorted(times[k])
            med[k] = v[len(v) // 2]
            moved = {"copy": 2 * n * n, "copy.T": 2 * n * n, "zeros": n * n, "to_dense.rows": n * n + M.nze, "to_dense.cols": n * n + M.nze,
                     "from_dense.rows": 2 * M.nze, "from_dense.cols": 2 * M.nze}.get(k)
            say("  %-16s median %9.4f ms  min %9.4f  max %9.4f  spread %5.1f %%  %s   samples: %s"
                % (k, med[k], v[0], v[-1], 100 * (v[-1] - v[0]) / med[k], "%8.1f GB/s" % (8e-6 * moved / med[k]) if moved else " " * 13,
                   " ".join("%.4f" % x for x in times[k])))
        say("  ratios (median / median): to_dense.rows / copy.T %.2f, to_dense.cols / copy %.2f, from_dense.rows / copy.T %.2f, from_dense.cols / copy %.2f, "
            "to_dense.rows / zeros %.2f" % (med["to_dense.rows"] / med["copy.T"], med["to_dense.cols"] / med["copy"], med["from_dense.rows"] / med["copy.T"],
                                            med["from_dense.cols"] / med["copy"], med["to_dense.rows"] / med["zeros"]))
        results[fill] = times
        del M, X
    say("")
    say("condition: the device path (dbcsr_to_dense, allocation included, synchronised) is faster than the host round trip in every alternation")
    ok = True
    for fill, times in results.items():
        r = sorted(x / z for x, z in zip(times["device path"], times["host path"]))
        ok = ok and r[-1] < 1.0
        say("  fill %.2f: device path / host path  %.6f ... %.6f   %s" % (fill, r[0], r[-1], "holds" if r[-1] < 1.0 else "FAILS"))
    say("  the condition %s" % ("holds" if ok else "FAILS"))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def host_csr(rs, cs, row_p, col_i, blk_p, data):
    """the element CSR of a host matrix by a loop over its blocks (numpy per block: the transposed block into the rows of its block row)"""
    ro, co = np.concatenate([[0], np.cumsum(rs, dtype=np.int64)]), np.concatenate([[0], np.cumsum(cs, dtype=np.int64)])
    crow = np.zeros(int(ro[-1]) + 1, np.int64)
    cols, vals = [], []
    for r in range(len(rs)):
        m, blocks = int(rs[r]), range(int(row_p[r]), int(row_p[r + 1]))
        if not len(blocks):
            continue
        tiles = [data[blk_p[b]:blk_p[b] + m * int(cs[col_i[b]])].reshape(int(cs[col_i[b]]), m).T for b in blocks]
        line = np.concatenate([np.arange(co[col_i[b]], co[col_i[b] + 1], dtype=np.int32) for b in blocks])
        vals.append(np.concatenate(tiles, axis=1).reshape(-1))
        cols.append(np.tile(line, m))
        crow[ro[r] + 1:ro[r + 1] + 1] = line.size
    crow = np.cumsum(crow)
    return crow, (np.concatenate(cols) if cols else np.zeros(0, np.int32)), (np.concatenate(vals) if vals else np.zeros(0, data.dtype))


def csr_conversion(args, say, lines, rng):
    from dbcsr_amd.csr import dbcsr_create_from_csr, dbcsr_from_csr, dbcsr_to_csr
    E = MultiplyEngine()
    b, nb = 23, 504
    n = b * nb
    results = {}
    out_r = torch.empty((n, n), dtype=torch.float64, device="cuda")
    eps = 0.25   # (uniform(-0.5, 0.5) values: about half of them are dropped)
    for fill in (1.0, 0.1):
        M = matrix_of(rng.random((nb, nb)) < fill, b, 40)
        X = M.copy()
        # what is timed is right: against the host's block loop, bit for bit (the whole comparison is the tests' business)
        ref = host_csr(*M.to_host())
        got = dbcsr_to_csr(M, engine=E)
        if any(g.cpu().numpy().tobytes() != r.tobytes() for g, r in zip(got, ref)):
            sys.exit("dbcsr_to_csr is wrong: nothing is timed")
        X.data.fill_(float("nan"))
        dbcsr_from_csr(*got, X, engine=E)
        if X.data.cpu().numpy().tobytes() != M.data.cpu().numpy().tobytes():
            sys.exit("dbcsr_from_csr is wrong: nothing is timed")
        half = dbcsr_to_csr(M, eps=eps, engine=E)
        keep = np.abs(ref[2]) > eps
        if half[2].cpu().numpy().tobytes() != ref[2][keep].tobytes() or half[1].cpu().numpy().tobytes() != ref[1][keep].tobytes():
            sys.exit("dbcsr_to_csr(eps) is wrong: nothing is timed")
        kept = float(keep.mean())
        del ref, half, keep
        crow, col, values = got

        def host_round_trip():
            out = [torch.as_tensor(a).cuda() for a in host_csr(*M.to_host())]
            torch.cuda.synchronize()
            return out

        def torch_csr():
            return dbcsr_to_dense(M, out=out_r, engine=E).to_sparse_csr()

        run = {
            "copy": lambda: X.data.copy_(M.data),
            "to_dense": lambda: dbcsr_to_dense(M, out=out_r, engine=E),
            "to_csr": lambda: dbcsr_to_csr(M, engine=E),
            "to_csr(eps)": lambda: dbcsr_to_csr(M, eps=eps, engine=E),
            "from_csr": lambda: dbcsr_from_csr(crow, col, values, X, engine=E),
            "create": lambda: dbcsr_create_from_csr(crow, col, values, M.row_blk_size, M.col_blk_size, engine=E),
            "torch.csr": torch_csr,
            "device path": lambda: dbcsr_to_csr(M, engine=E),
            "host path": host_round_trip,
        }
        try:
            torch_csr()
            torch.cuda.synchronize()
            torch_note = None
        except Exception as e:   # (what torch-ROCm does not offer is reported, not timed)
            torch_note = "%s: %s" % (type(e).__name__, str(e).splitlines()[0] if str(e) else "")
            del run["torch.csr"]
        wall = ("to_csr(eps)", "create", "torch.csr", "device path", "host path")
        times = {k: [] for k in run}
        for step in range(args.warmup + args.alternations):
            for k in run:
                x = sample_wall(run[k], 1 if k in ("host path", "create", "torch.csr") else args.reps) if k in wall else sample(run[k], args.reps)
                if step >= args.warmup:
                    times[k].append(x)
        say("")
        say("%d x %d blocks of %d x %d, fill %.2f: %d blocks, %.1f MB of blocks = nnz %d; eps = %.2f keeps %.1f %% of the elements"
            % (nb, nb, b, b, fill, M.nblks, 8e-6 * M.nze, M.nze, eps, 100 * kept))
        if torch_note:
            say("  torch.csr (dbcsr_to_dense(...).to_sparse_csr() on the device) is not offered here: %s" % torch_note)
        med = {}
        for k in run:
            v = sorted(times[k])
            med[k] = v[len(v) // 2]
            # elements of 8 bytes read + written: the data area and values; col counts half an element per entry
            moved = {"copy": 2 * M.nze, "to_dense": n * n + M.nze, "to_csr": 2.5 * M.nze, "from_csr": 2.5 * M.nze}.get(k)
            say("  %-16s median %10.4f ms  min %10.4f  max %10.4f  spread %5.1f %%  %s   samples: %s"
                % (k, med[k], v[0], v[-1], 100 * (v[-1] - v[0]) / med[k], "%8.1f GB/s" % (8e-6 * moved / med[k]) if moved else " " * 13,
                   " ".join("%.4f" % x for x in times[k])))
        say("  ratios (median / median): to_csr / copy %.2f, to_csr / to_dense %.2f, to_csr(eps) / to_csr %.2f, from_csr / copy %.2f, create / from_csr %.2f%s"
            % (med["to_csr"] / med["copy"], med["to_csr"] / med["to_dense"], med["to_csr(eps)"] / med["to_csr"], med["from_csr"] / med["copy"],
               med["create"] / med["from_csr"], ", to_csr / torch.csr %.3f" % (med["to_csr"] / med["torch.csr"]) if "torch.csr" in med else ""))
        results[fill] = times
        del M, X, got, crow, col, values
    say("")
    say("condition: the device path (dbcsr_to_csr, allocation included, synchronised) is faster than the host round trip in every alternation")
    ok = True
    for fill, times in results.items():
        r = sorted(x / z for x, z in zip(times["device path"], times["host path"]))
        ok = ok and r[-1] < 1.0
        say("  fill %.2f: device path / host path  %.6f ... %.6f   %s" % (fill, r[0], r[-1], "holds" if r[-1] < 1.0 else "FAILS"))
    say("  the condition %s" % ("holds" if ok else "FAILS"))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def submatrix(args, say, lines, rng):
    """the submatrix method's two copies on the matrix of the dense conversion, and the full-set gather against dbcsr_to_dense"""
    E = MultiplyEngine()
    b, nb = 23, 504
    n_full = b * nb
    M = matrix_of(rng.random((nb, nb)) < 0.1, b, 40)
    # one submatrix per block column
    plan = dbcsr_submatrix_plan(M)
    n = plan.max_dim
    batch = torch.full((plan.nsub, n, n), float("nan"), dtype=torch.float64, device="cuda")
    dbcsr_submatrix_gather(M, plan, pad_diag=1.0, out=batch, engine=E)
    D = dbcsr_to_dense(M, engine=E)
    # what is timed is right: some windows against index_select of the whole dense matrix, bit for bit (the whole comparison is the tests' business)
    set_ptr, set_idx = plan.set_ptr.cpu().numpy(), plan.set_idx.cpu().numpy()
    for g in (0, nb // 2, nb - 1):
        S = set_idx[set_ptr[g]:set_ptr[g + 1]]
        e = torch.as_tensor((S[:, None].astype(np.int64) * b + np.arange(b)).reshape(-1)).cuda()
        ng = int(e.numel())
        if ng != int(plan.sub_dim_host[g]) or not torch.equal(batch[g, :ng, :ng], D[e][:, e]) or bool(torch.isnan(batch[g]).any()):
            sys.exit("dbcsr_submatrix_gather is wrong: nothing is timed")
    X = M.copy()
    dbcsr_submatrix_scatter(batch, X, plan, engine=E)
    if not torch.equal(X.data, M.data):
        sys.exit("dbcsr_submatrix_scatter is wrong: nothing is timed")
    filled = int((plan.sub_dim_host ** 2).sum())
    say("")
    say("%d x %d blocks of %d x %d, fill 0.10: %d blocks, %.1f MB of blocks; one submatrix per block column: %d windows, sides %d ... %d, %d members at most"
        % (nb, nb, b, b, M.nblks, 8e-6 * M.nze, plan.nsub, int(plan.sub_dim_host.min()), n, plan.max_members))
    say("the batch (%d, %d, %d): %.1f MB, of which %.1f MB inside the submatrices (%.1f %% padding)"
        % (plan.nsub, n, n, 8e-6 * plan.nsub * n * n, 8e-6 * filled, 100.0 * (1 - filled / (plan.nsub * n * n))))
    # the full set: one submatrix holding every block row, against dbcsr_to_dense of the same matrix
    whole = dbcsr_submatrix_plan(M, [0] * nb)
    out_s = torch.full((1, n_full, n_full), float("nan"), dtype=torch.float64, device="cuda")
    dbcsr_submatrix_gather(M, whole, out=out_s, engine=E)
    if not torch.equal(out_s[0], D):
        sys.exit("the full-set gather is not dbcsr_to_dense: nothing is timed")
    run = {
        "gather": lambda: dbcsr_submatrix_gather(M, plan, pad_diag=1.0, out=batch, engine=E),
        "scatter": lambda: dbcsr_submatrix_scatter(batch, X, plan, engine=E),
        "zeros(batch)": lambda: batch.zero_(),
        "full-set gather": lambda: dbcsr_submatrix_gather(M, whole, out=out_s, engine=E),
        "to_dense": lambda: dbcsr_to_dense(M, out=D, engine=E),
    }
    moved = {"gather": plan.nsub * n * n, "scatter": 2 * M.nze, "zeros(batch)": plan.nsub * n * n, "full-set gather": n_full * n_full + M.nze,
             "to_dense": n_full * n_full + M.nze}
    times = {k: [] for k in run}
    for step in range(args.warmup + args.alternations):
        for k in run:
            x = sample(run[k], args.reps)
            if step >= args.warmup:
                times[k].append(x)
    dbcsr_submatrix_gather(M, plan, pad_diag=1.0, out=batch, engine=E)   # (zeros(batch) ran last on it)
    med = {}
    for k in run:
        v = sorted(times[k])
        med[k] = v[len(v) // 2]
        say("  %-16s median %9.4f ms  min %9.4f  max %9.4f  spread %5.1f %%  %8.1f GB/s   samples: %s"
            % (k, med[k], v[0], v[-1], 100 * (v[-1] - v[0]) / med[k], 8e-6 * moved[k] / med[k], " ".join("%.4f" % x for x in times[k])))
    say("  (GB/s: gather and zeros by the batch's bytes written, scatter by the blocks read and written, the two full matrices by window + blocks)")
    r = sorted(x / z for x, z in zip(times["full-set gather"], times["to_dense"]))
    say("  full-set gather / to_dense: median of medians %.3f; per alternation %.3f ... %.3f (median %.3f, spread %.1f %%)"
        % (med["full-set gather"] / med["to_dense"], r[0], r[-1], r[len(r) // 2], 100 * (r[-1] - r[0]) / r[len(r) // 2]))
    say("  gather / zeros(batch): %.2f" % (med["gather"] / med["zeros(batch)"]))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def elementwise(args, say, lines, rng, b, nb, st):
    E = MultiplyEngine()
    f64 = L.dbcsr_type_real_8
    mask = rng.random((nb, nb)) < args.fill_flat
    A, B = matrix_of(mask, b, 1), matrix_of(mask, b, 2)
    a, b_ = A.desc(), B.desc()
    # the general pair of the standard report: three disjoint random sets of blocks S, SA, SB of equal size; A = S + SA, B = S + SB
    u = rng.random((nb, nb))
    q = args.fill_general / 2
    GA, GB = matrix_of((u < 2 * q), b, 3), matrix_of((u < q) | ((u >= 2 * q) & (u < 3 * q)), b, 4)
    ga, gb = GA.desc(), GB.desc()
    check = lambda rc: rc == 0 or sys.exit("a library call failed (%d)" % rc)
    one, beta = (C.c_double * 2)(1.0, 0.0), (C.c_double * 2)(1e-3, 0.0)
    nblk, nze, same = C.c_int64(), C.c_int64(), C.c_int32()

    def counted(entry, flag):
        row_p = torch.empty(nb + 1, dtype=torch.int32, device="cuda")
        count = lambda: check(entry(E.h, C.byref(ga), C.byref(gb), flag, row_p.data_ptr(), C.byref(nblk), C.byref(nze), C.byref(same), st.ptr))
        count()
        assert same.value == 0
        D = DbcsrMatrix(GA.row_blk_size, GA.col_blk_size, row_p, torch.empty(nblk.value, dtype=torch.int32, device="cuda"),
                        torch.empty(nblk.value, dtype=torch.int64, device="cuda"), torch.empty(nze.value, dtype=torch.float64, device="cuda"))
        return count, D, D.desc(out=True)

    had_count, HD, hd = counted(E.L.dbcsr_amd_bcsr_hadamard_count, 0)
    add_count, AD, ad = counted(E.L.dbcsr_amd_bcsr_add_count, 0)

    def had_general():
        had_count()
        check(E.L.dbcsr_amd_bcsr_hadamard_apply(E.h, f64, C.byref(ga), C.byref(gb), None, C.byref(hd), st.ptr))

    def add_general():
        add_count()
        check(E.L.dbcsr_amd_bcsr_add_apply(E.h, f64, one, C.byref(ga), beta, C.byref(gb), C.byref(ad), st.ptr))

    def had_flat():
        assert dbcsr_hadamard_product(A, B, A, engine=E) is True

    def add_flat():
        assert dbcsr_add(A, B, 1.0, 1e-3, engine=E) is True

    # what is timed is right: the first blocks of each result against torch (the whole comparison is the tests' business)
    head = 4096 * b * b
    keep = A.data[:head].clone()
    had_flat()
    had_general()
    torch.cuda.synchronize()
    if not torch.equal(A.data[:head], keep * B.data[:head]):
        sys.exit("the flat hadamard product is wrong: nothing is timed")
    shared = torch.as_tensor(np.flatnonzero((u < q)[u < 2 * q])[:64]).cuda()    # positions in GA of blocks both have ...
    theirs = torch.as_tensor(np.flatnonzero((u < q)[(u < q) | ((u >= 2 * q) & (u < 3 * q))])[:64]).cuda()   # ... and in GB, in the same order
    want = GA.data.view(-1, b * b)[shared] * GB.data.view(-1, b * b)[theirs]
    if HD.nblks != int(np.count_nonzero(u < q)) or not torch.equal(HD.data.view(-1, b * b)[:64], want):
        sys.exit("the general hadamard product is wrong: nothing is timed")
    check(E.L.dbcsr_amd_bcsr_copy_onto(E.h, f64, C.byref(b_), C.byref(a), st.ptr))
    if not torch.equal(A.data[:head], B.data[:head]):
        sys.exit("copy_onto is wrong: nothing is timed")
    keep = A.data[:head].clone()
    check(E.L.dbcsr_amd_bcsr_function_of_elements(E.h, f64, C.byref(a), dbcsr_func_tanh, 0.0, 1.0, st.ptr))
    if not float((A.data[:head] - torch.tanh(keep)).abs().max()) < 1e-15:
        sys.exit("function_of_elements is wrong: nothing is timed")
    del keep, want
    run = {
        "had.flat": had_flat,
        "add.flat": add_flat,
        "torch.mul": lambda: torch.mul(A.data, B.data, out=A.data),
        "had.general": had_general,
        "had.count": had_count,
        "add.general": add_general,
        "add.count": add_count,
        "copy_onto": lambda: check(E.L.dbcsr_amd_bcsr_copy_onto(E.h, f64, C.byref(b_), C.byref(a), st.ptr)),
        "torch.copy_": lambda: A.data.copy_(B.data),
        "function": lambda: check(E.L.dbcsr_amd_bcsr_function_of_elements(E.h, f64, C.byref(a), dbcsr_func_tanh, 0.0, 1.0, st.ptr)),
        "torch.tanh_": lambda: A.data.tanh_(),
    }
    nbytes = {"had.flat": 24 * A.nze, "add.flat": 24 * A.nze, "torch.mul": 24 * A.nze, "had.general": 8 * 3 * HD.nze, "had.count": 0,
              "add.general": 8 * (GA.nze + GB.nze + AD.nze), "add.count": 0, "copy_onto": 16 * A.nze, "torch.copy_": 16 * A.nze, "function": 16 * A.nze,
              "torch.tanh_": 16 * A.nze}
    times = {k: [] for k in run}
    for step in range(args.warmup + args.alternations):
        for k in run:
            if k in ("copy_onto", "function"):
                A.data.copy_(B.data)   # (values of the usual size for what follows: the products before shrank them)
            t = sample(run[k], args.reps)
            if step >= args.warmup:
                times[k].append(t)
    say("")
    say("same pattern: %d blocks, %.1f MB per matrix; general: %d and %d blocks (%.1f MB each), %d shared (%.1f MB): the product; %d in the union (%.1f MB): the sum"
        % (A.nblks, 8e-6 * A.nze, GA.nblks, GB.nblks, 8e-6 * GA.nze, HD.nblks, 8e-6 * HD.nze, AD.nblks, 8e-6 * AD.nze))
    med = {}
    for k in run:
        v = sorted(times[k])
        med[k] = v[len(v) // 2]
        rate = ("%8.1f GB/s" % (1e-6 * nbytes[k] / med[k])) if nbytes[k] else "   (no data moved)"
        say("  %-12s  median %8.4f ms  min %8.4f  max %8.4f  spread %5.1f %%  %s   samples: %s"
            % (k, med[k], v[0], v[-1], 100 * (v[-1] - v[0]) / med[k], rate, " ".join("%.4f" % x for x in times[k])))
    say("  (GB/s of had.general: the shared blocks read from both operands and written once; the blocks only one operand has are not touched)")
    say("")
    say("time against the yardstick of the same run (median / median; the ratio per alternation, sample by sample)")
    for k, y in (("had.flat", "add.flat"), ("had.flat", "torch.mul"), ("had.general", "add.general"), ("had.count", "add.count"), ("copy_onto", "torch.copy_"),
                 ("function", "torch.tanh_")):
        r = sorted(x / z for x, z in zip(times[k], times[y]))
        say("  %-12s / %-12s  %.2f   (per alternation %.2f ... %.2f)" % (k, y, med[k] / med[y], r[0], r[-1]))
    had_apply, add_apply = med["had.general"] - med["had.count"], med["add.general"] - med["add.count"]
    say("  apply = general - count: hadamard %.4f ms (%.1f GB/s), add %.4f ms (%.1f GB/s); per byte moved the hadamard apply runs at %.2f of the add's rate"
        % (had_apply, 1e-6 * nbytes["had.general"] / had_apply, add_apply, 1e-6 * nbytes["add.general"] / add_apply,
           (nbytes["had.general"] / had_apply) / (nbytes["add.general"] / add_apply)))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def blocks(args, say, lines, rng, b, nb, st):
    E = MultiplyEngine()
    f64 = L.dbcsr_type_real_8
    mask = rng.random((nb, nb)) < args.fill_flat
    A, B = matrix_of(mask, b, 1), matrix_of(mask, b, 2)
    a, b_ = A.desc(), B.desc()
    u = rng.random((nb, nb))
    q = args.fill_general / 2
    mask_b = (u < q) | ((u >= 2 * q) & (u < 3 * q))
    GA, GB = matrix_of((u < 2 * q), b, 3), matrix_of(mask_b, b, 4)
    ga, gb = GA.desc(), GB.desc()
    check = lambda rc: rc == 0 or sys.exit("a library call failed (%d)" % rc)
    one, small = (C.c_double * 2)(1.0, 0.0), (C.c_double * 2)(1e-3, 0.0)
    t32 = lambda x: torch.as_tensor(np.ascontiguousarray(x, np.int32)).cuda()
    # the whole pattern in random order; entry i's window is block i of a packed source
    rr, cc = np.nonzero(mask)
    perm = rng.permutation(len(rr))
    rows, cols, n = t32(rr[perm]), t32(cc[perm]), len(rr)
    off = torch.arange(n, dtype=torch.int64, device="cuda") * (b * b)
    src = torch.rand(n * b * b, dtype=torch.float64, device="cuda") - 0.5
    out = torch.empty(n * b * b, dtype=torch.float64, device="cuda")
    found = torch.empty(n, dtype=torch.int32, device="cuda")
    put = lambda alpha, summation: check(E.L.dbcsr_amd_bcsr_put_blocks(E.h, f64, C.byref(a), n, rows.data_ptr(), cols.data_ptr(), off.data_ptr(),
                                                                       src.data_ptr(), alpha, summation, st.ptr))
    get = lambda: check(E.L.dbcsr_amd_bcsr_get_blocks(E.h, f64, C.byref(a), n, rows.data_ptr(), cols.data_ptr(), off.data_ptr(), out.data_ptr(),
                                                      found.data_ptr(), st.ptr))
    # the general pair: B's pattern as a list in random order, reserved on A
    gr, gc = np.nonzero(mask_b)
    gperm = rng.permutation(len(gr))
    g_rows, g_cols, g_n = t32(gr[gperm]), t32(gc[gperm]), len(gr)
    nblk, nze, same, new, bad = C.c_int64(), C.c_int64(), C.c_int32(), C.c_int64(), C.c_int64()
    r_row_p, a_row_p, s_row_p, n_row_p = (torch.empty(nb + 1, dtype=torch.int32, device="cuda") for _ in range(4))
    reserve_count = lambda: check(E.L.dbcsr_amd_bcsr_reserve_count(E.h, C.byref(ga), g_n, g_rows.data_ptr(), g_cols.data_ptr(), 0, r_row_p.data_ptr(),
                                                                   C.byref(nblk), C.byref(nze), C.byref(new), C.byref(bad), st.ptr))
    add_count = lambda: check(E.L.dbcsr_amd_bcsr_add_count(E.h, C.byref(ga), C.byref(gb), 0, a_row_p.data_ptr(), C.byref(nblk), C.byref(nze), C.byref(same),
                                                           st.ptr))
    result = lambda row_p: DbcsrMatrix(GA.row_blk_size, GA.col_blk_size, row_p, torch.empty(nblk.value, dtype=torch.int32, device="cuda"),
                                       torch.empty(nblk.value, dtype=torch.int64, device="cuda"), torch.empty(nze.value, dtype=torch.float64, device="cuda"))
    reserve_count()
    union = int(np.count_nonzero((u < 2 * q) | mask_b))
    if (new.value, bad.value, nblk.value) != (union - GA.nblks, 0, union):
        sys.exit("the reserve count is wrong: nothing is timed")
    RD = result(r_row_p)
    rd = RD.desc(out=True)
    add_count()
    AD = result(a_row_p)
    ad = AD.desc(out=True)

    def reserve_general():
        reserve_count()
        check(E.L.dbcsr_amd_bcsr_reserve_apply(E.h, f64, C.byref(ga), C.byref(rd), st.ptr))

    def add_general():
        add_count()
        check(E.L.dbcsr_amd_bcsr_add_apply(E.h, f64, one, C.byref(ga), small, C.byref(gb), C.byref(ad), st.ptr))

    def reserve_none():
        check(E.L.dbcsr_amd_bcsr_reserve_count(E.h, C.byref(a), n, rows.data_ptr(), cols.data_ptr(), 0, n_row_p.data_ptr(), C.byref(nblk), C.byref(nze),
                                               C.byref(new), C.byref(bad), st.ptr))
        assert new.value == 0 and bad.value == 0

    def add_count_same():
        check(E.L.dbcsr_amd_bcsr_add_count(E.h, C.byref(a), C.byref(b_), 0, s_row_p.data_ptr(), C.byref(nblk), C.byref(nze), C.byref(same), st.ptr))
        assert same.value == 1

    def add_flat():
        assert dbcsr_add(A, B, 1.0, 1e-3, engine=E) is True

    # what is timed is right: a sample of the blocks of each result against torch (the whole comparison is the tests' business)
    pick = torch.as_tensor(rng.permutation(n)[:4096]).cuda()
    where = torch.as_tensor(perm).cuda()[pick]   # (entry i names block perm[i] of the index: np.nonzero lists the pattern in index order)
    put(one, 0)
    get()
    torch.cuda.synchronize()
    if not torch.equal(A.data.view(-1, b * b)[where], src.view(-1, b * b)[pick]) or not torch.equal(out, src) or not bool(found.all()):
        sys.exit("put or get is wrong: nothing is timed")
    keep = A.data.view(-1, b * b)[where].clone()
    put(one, 1)
    torch.cuda.synchronize()
    if not torch.equal(A.data.view(-1, b * b)[where], keep + src.view(-1, b * b)[pick]):
        sys.exit("put with summation is wrong: nothing is timed")
    del keep
    reserve_general()
    add_general()
    torch.cuda.synchronize()
    if not (torch.equal(RD.row_p, AD.row_p) and torch.equal(RD.col_i, AD.col_i) and torch.equal(RD.blk_p, AD.blk_p)):
        sys.exit("the reserved pattern is not the union the add forms: nothing is timed")
    run = {
        "put.over": lambda: put(one, 0),
        "get": get,
        "copy_onto": lambda: check(E.L.dbcsr_amd_bcsr_copy_onto(E.h, f64, C.byref(b_), C.byref(a), st.ptr)),
        "torch.copy_": lambda: A.data.copy_(B.data),
        "put.sum": lambda: put(one, 1),
        "add.flat": add_flat,
        "put.python": lambda: dbcsr_put_blocks(A, rows, cols, src, off, keep_sparsity=True, engine=E),
        "reserve.general": reserve_general,
        "reserve.count": reserve_count,
        "add.general": add_general,
        "add.count": add_count,
        "reserve.none": reserve_none,
        "add.count.same": add_count_same,
    }
    nbytes = {"put.over": 16 * A.nze, "get": 16 * A.nze, "copy_onto": 16 * A.nze, "torch.copy_": 16 * A.nze, "put.sum": 24 * A.nze, "add.flat": 24 * A.nze,
              "put.python": 16 * A.nze, "reserve.general": 8 * (GA.nze + RD.nze), "reserve.count": 0, "add.general": 8 * (GA.nze + GB.nze + AD.nze),
              "add.count": 0, "reserve.none": 0, "add.count.same": 0}
    times = {k: [] for k in run}
    for step in range(args.warmup + args.alternations):
        for k in run:
            if k in ("put.sum", "add.flat"):
                A.data.copy_(B.data)   # (values of the usual size for what follows: the sums before grew them)
            t = sample(run[k], args.reps)
            if step >= args.warmup:
                times[k].append(t)
    # a whole matrix from the list, against from_host of the same matrix: one call per sample, by the host's clock
    sizes = A.row_blk_size
    host = [x.cpu().numpy() for x in (sizes, sizes, A.row_p, A.col_i, A.blk_p, A.data)]
    made = {"create": lambda: dbcsr_create_from_blocks(sizes, sizes, rows, cols, src, off, summation=True, engine=E),
            "from_host": lambda: DbcsrMatrix.from_host(*host)}
    M = made["create"]()
    torch.cuda.synchronize()
    if M.nblks != n or not torch.equal(M.col_i, A.col_i) or not torch.equal(M.data.view(-1, b * b)[where], src.view(-1, b * b)[pick]):
        sys.exit("create_from_blocks is wrong: nothing is timed")
    del M
    for k in made:
        times[k] = []
    for step in range(args.warmup + args.alternations):
        for k in made:
            t = sample_wall(made[k], 1)
            if step >= args.warmup:
                times[k].append(t)
    nbytes.update({"create": 16 * A.nze, "from_host": 8 * A.nze})
    say("")
    say("full pattern: %d blocks in a list in random order, %.1f MB per matrix and source; general: %d blocks, a list of %d, %d of them new (%.1f MB in, %.1f MB out)"
        % (n, 8e-6 * A.nze, GA.nblks, g_n, RD.nblks - GA.nblks, 8e-6 * GA.nze, 8e-6 * RD.nze))
    med = {}
    for k in times:
        v = sorted(times[k])
        med[k] = v[len(v) // 2]
        rate = ("%8.1f GB/s" % (1e-6 * nbytes[k] / med[k])) if nbytes[k] else "   (no data moved)"
        say("  %-15s  median %9.4f ms  min %9.4f  max %9.4f  spread %5.1f %%  %s   samples: %s"
            % (k, med[k], v[0], v[-1], 100 * (v[-1] - v[0]) / med[k], rate, " ".join("%.4f" % x for x in times[k])))
    say("  (GB/s of reserve.general: A's blocks read and the result written; of create: the source read and the matrix written -- its zeros are written first;")
    say("   of from_host: the data area copied once; create and from_host by the host's clock, one call per sample)")
    say("")
    say("time against the yardstick of the same run (median / median; the ratio per alternation, sample by sample)")
    for k, y in (("put.over", "copy_onto"), ("put.over", "torch.copy_"), ("put.python", "put.over"), ("put.sum", "add.flat"), ("get", "copy_onto"),
                 ("get", "torch.copy_"), ("reserve.general", "add.general"), ("reserve.count", "add.count"), ("reserve.none", "add.count.same"),
                 ("create", "from_host")):
        r = sorted(x / z for x, z in zip(times[k], times[y]))
        say("  %-15s / %-14s  %.2f   (per alternation %.2f ... %.2f)" % (k, y, med[k] / med[y], r[0], r[-1]))
    r_apply, a_apply = med["reserve.general"] - med["reserve.count"], med["add.general"] - med["add.count"]
    say("  apply = general - count: reserve %.4f ms (%.1f GB/s), add %.4f ms (%.1f GB/s)"
        % (r_apply, 1e-6 * nbytes["reserve.general"] / r_apply, a_apply, 1e-6 * nbytes["add.general"] / a_apply))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--block", type=int, default=23)
    ap.add_argument("--fill-flat", type=float, default=1.0, help="pattern fill of the same-pattern add and the norm (config 2's product is full)")
    ap.add_argument("--fill-general", type=float, default=0.5, help="pattern fill of each operand of the general add (at most 2/3)")
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--colsums", action="store_true", help="the forms of algebra_col_sums against each other (lab build)")
    ap.add_argument("--matvec", action="store_true", help="only the matrix-vector product, its yardsticks and the sums its passes are made from")
    ap.add_argument("--multivec", action="store_true", help="only the matrix times several dense vectors and its yardsticks")
    ap.add_argument("--rank-update", action="store_true", help="only the rank-k update on the stored pattern and its yardsticks")
    ap.add_argument("--block-inverse", action="store_true", help="only the block diagonal: get_block_diag, invert_block_diag and what they replace")
    ap.add_argument("--block-scale", action="store_true", help="only the block diagonal applied to a matrix: left, right, both, dbcsr_scale and the multiply it replaces")
    ap.add_argument("--dense", action="store_true", help="only the dense conversion: to_dense, from_dense, create_from_dense and what they replace")
    ap.add_argument("--csr", action="store_true", help="only the element CSR form: to_csr, from_csr, create_from_csr and what they replace")
    ap.add_argument("--submatrix", action="store_true", help="only the submatrix method: gather, scatter, and the full-set gather against to_dense")
    ap.add_argument("--elementwise", action="store_true", help="only the element-wise operations on two patterns and their yardsticks")
    ap.add_argument("--blocks", action="store_true", help="only the block lists: reserve, put, get, create_from_blocks and their yardsticks")
    ap.add_argument("--mfma-tflops", type=float, default=None, help="with --rank-update / --block-scale: the fp64 MFMA figure bench.py --full measured in the same session")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ops_bench.py measures on the GPU"
    assert 0 < args.fill_general <= 2.0 / 3
    b, nb = args.block, args.n // args.block
    lines = []
    say = lambda s: (print(s, flush=True), lines.append(s))
    say("matrix algebra between multiplies, float64, %d x %d block rows / columns of %d x %d blocks (n = %d); %s" % (nb, nb, b, b, args.n, torch.cuda.get_device_name(0)))
    say("%d alternations after %d warm-up rounds, %d calls per sample; ms per call; GB/s = 8 * (elements read + written) / time" % (args.alternations, args.warmup, args.reps))
    E, st = MultiplyEngine(), StreamHandle()
    rng = np.random.default_rng(2)
    if args.colsums:
        return colsums(args, say, lines, rng, b, nb, st)
    if args.multivec:
        return multivec(args, say, lines, rng, b, nb, st)
    if args.rank_update:
        return rank_update(args, say, lines, rng, b, nb, st)
    if args.block_inverse:
        return block_inverse(args, say, lines, rng)
    if args.block_scale:
        return block_scale(args, say, lines, rng)
    if args.dense:
        return dense_conversion(args, say, lines, rng)
    if args.csr:
        return csr_conversion(args, say, lines, rng)
    if args.submatrix:
        return submatrix(args, say, lines, rng)
    if args.elementwise:
        return elementwise(args, say, lines, rng, b, nb, st)
    if args.blocks:
        return blocks(args, say, lines, rng, b, nb, st)
    only =("norm", "norm.T", "matvec.N", "matvec.T", "matvec.S", "gersh.N", "colnorm", "gersh.S") if args.matvec else None
    # the same-pattern pair
    mask = rng.random((nb, nb)) < args.fill_flat
    A, B = matrix_of(mask, b, 1), matrix_of(mask, b, 2)
    beta = 1e-3
    # the general pair: three disjoint random sets of blocks S, SA, SB of equal size; A = S + SA, B = S + SB
    u = rng.random((nb, nb))
    q = args.fill_general / 2
    GA, GB = matrix_of((u < 2 * q), b, 3), matrix_of((u < q) | ((u >= 2 * q) & (u < 3 * q)), b, 4)
    ga, gb = GA.desc(), GB.desc()
    row_p = torch.empty(nb + 1, dtype=torch.int32, device="cuda")
    nblk, nze, same = C.c_int64(), C.c_int64(), C.c_int32()
    count = lambda: E.L.dbcsr_amd_bcsr_add_count(E.h, C.byref(ga), C.byref(gb), 0, row_p.data_ptr(), C.byref(nblk), C.byref(nze), C.byref(same), st.ptr)
    assert count() == 0 and same.value == 0
    D = DbcsrMatrix(GA.row_blk_size, GA.col_blk_size, row_p, torch.empty(nblk.value, dtype=torch.int32, device="cuda"),
                    torch.empty(nblk.value, dtype=torch.int64, device="cuda"), torch.empty(nze.value, dtype=torch.float64, device="cuda"))
    gd = D.desc(out=True)
    one, two, zero = (C.c_double * 2)(1.0, 0.0), (C.c_double * 2)(beta, 0.0), (C.c_double * 2)(0.0, 0.0)
    shared = int(np.count_nonzero(u < q))
    out2 = (C.c_double * 2)()
    a = A.desc()

    b_ = B.desc()
    row_p_same = torch.empty(nb + 1, dtype=torch.int32, device="cuda")
    nblk_s, nze_s, same_s = C.c_int64(), C.c_int64(), C.c_int32()
    count_same = lambda: E.L.dbcsr_amd_bcsr_add_count(E.h, C.byref(a), C.byref(b_), 0, row_p_same.data_ptr(), C.byref(nblk_s), C.byref(nze_s), C.byref(same_s), st.ptr)

    # norms and vectors: A (full), the stored upper triangle T of a symmetric matrix of the same shape
    T = matrix_of(np.triu(mask), b, 5)
    t_ = T.desc()
    f64 = L.dbcsr_type_real_8
    ones = torch.ones(nb * b, dtype=torch.float64, device="cuda")
    colv = torch.empty(nb * b, dtype=torch.float64, device="cuda")
    check = lambda rc: rc == 0 or sys.exit("a library call failed (%d)" % rc)

    def general():
        assert count() == 0
        assert E.L.dbcsr_amd_bcsr_add_apply(E.h, L.dbcsr_type_real_8, one, C.byref(ga), two, C.byref(gb), C.byref(gd), st.ptr) == 0

    def flat():
        assert dbcsr_add(A, B, 1.0, beta, engine=E) is True

    run = {
        "flat": flat,
        "torch.add": lambda: torch.add(A.data, B.data, alpha=beta, out=A.data),
        "flat.count": lambda: count_same(),
        "general": general,
        "count": lambda: count(),
        "norm": lambda: E.L.dbcsr_amd_bcsr_norm2(E.h, L.dbcsr_type_real_8, C.byref(a), 0, out2, st.ptr),
        "torch.norm": lambda: torch.linalg.vector_norm(A.data),
        "gersh.N": lambda: check(E.L.dbcsr_amd_bcsr_gershgorin(E.h, f64, C.byref(a), 0, out2, st.ptr)),
        "norm.T": lambda: check(E.L.dbcsr_amd_bcsr_norm2(E.h, f64, C.byref(t_), 1, out2, st.ptr)),
        "gersh.S": lambda: check(E.L.dbcsr_amd_bcsr_gershgorin(E.h, f64, C.byref(t_), 1, out2, st.ptr)),
        "colnorm": lambda: check(E.L.dbcsr_amd_bcsr_col_sums(E.h, f64, C.byref(a), 1, 0, colv.data_ptr(), colv.numel(), st.ptr)),
        "maxabs": lambda: check(E.L.dbcsr_amd_bcsr_maxabs(E.h, f64, C.byref(a), out2, st.ptr)),
        "scale.R": lambda: check(E.L.dbcsr_amd_bcsr_scale_by_vector(E.h, f64, C.byref(a), ones.data_ptr(), ones.numel(), 1, st.ptr)),
        "scale.L": lambda: check(E.L.dbcsr_amd_bcsr_scale_by_vector(E.h, f64, C.byref(a), ones.data_ptr(), ones.numel(), 0, st.ptr)),
        "torch.mul": lambda: torch.mul(A.data, 1.0, out=A.data),
        "matvec.N": lambda: check(E.L.dbcsr_amd_bcsr_matvec(E.h, f64, b"N", one, C.byref(a), -1, ones.data_ptr(), ones.numel(), zero, colv.data_ptr(), colv.numel(), st.ptr)),
        "matvec.T": lambda: check(E.L.dbcsr_amd_bcsr_matvec(E.h, f64, b"T", one, C.byref(a), -1, ones.data_ptr(), ones.numel(), zero, colv.data_ptr(), colv.numel(), st.ptr)),
        "matvec.S": lambda: check(E.L.dbcsr_amd_bcsr_matvec(E.h, f64, b"N", one, C.byref(t_), 0, ones.data_ptr(), ones.numel(), zero, colv.data_ptr(), colv.numel(), st.ptr)),
    }
    if only:
        run = {k: run[k] for k in only}
    nbytes = {"flat": 24 * A.nze, "torch.add": 24 * A.nze, "flat.count": 0, "general": 8 * (GA.nze + GB.nze + nze.value), "count": 0, "norm": 8 * A.nze, "torch.norm": 8 * A.nze,
              "gersh.N": 8 * A.nze, "norm.T": 8 * T.nze, "gersh.S": 16 * T.nze, "colnorm": 8 * A.nze, "maxabs": 8 * A.nze, "scale.R": 16 * A.nze, "scale.L": 16 * A.nze,
              "torch.mul": 16 * A.nze, "matvec.N": 8 * A.nze, "matvec.T": 8 * A.nze, "matvec.S": 16 * T.nze}
    times = {k: [] for k in run}
    for step in range(args.warmup + args.alternations):
        for k in run:
            t = sample(run[k], args.reps)
            if step >= args.warmup:
                times[k].append(t)
    say("")
    say("same pattern: %d blocks, %.1f MB per matrix; general: %d and %d blocks (%.1f MB each), %d shared (%.0f %% of each), %d in the union (%.1f MB)"
        % (A.nblks, 8e-6 * A.nze, GA.nblks, GB.nblks, 8e-6 * GA.nze, shared, 100.0 * shared / max(1, GA.nblks), nblk.value, 8e-6 * nze.value))
    med = {}
    for k in run:
        v = sorted(times[k])
        med[k] = v[len(v) // 2]
        rate = ("%8.1f GB/s" % (1e-6 * nbytes[k] / med[k])) if nbytes[k] else "   (no data moved)"
        say("  %-10s  median %8.4f ms  min %8.4f  max %8.4f  spread %5.1f %%  %s   samples: %s"
            % (k, med[k], v[0], v[-1], 100 * (v[-1] - v[0]) / med[k], rate, " ".join("%.4f" % x for x in times[k])))
    matvec_rows = (("matvec.N", "norm"), ("matvec.T", "norm"), ("matvec.S", "norm.T"))
    if only:
        say("")
        say("matrix-vector product: time against the yardstick of the same run (median / median; spread of the ratio over the alternations, sample by sample);")
        say("below them the sums whose walks the passes are, without the reads of x")
        for k, y in matvec_rows + (("gersh.N", "norm"), ("colnorm", "norm"), ("gersh.S", "norm.T")):
            r = sorted(x / z for x, z in zip(times[k], times[y]))
            say("  %-8s / %-9s  %.2f   (per alternation %.2f ... %.2f)" % (k, y, med[k] / med[y], r[0], r[-1]))
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    flat_ms = med["flat"] - med["flat.count"]
    say("  flat kernel = flat - flat.count: %.4f ms, %.1f GB/s, %.2f of torch.add's rate" % (flat_ms, 1e-6 * nbytes["flat"] / flat_ms, med["torch.add"] / flat_ms))
    apply_ms = med["general"] - med["count"]
    say("  apply = general - count: %.4f ms, %.1f GB/s" % (apply_ms, 1e-6 * nbytes["general"] / apply_ms))
    flat_rate, torch_rate = nbytes["flat"] / med["flat"], nbytes["torch.add"] / med["torch.add"]
    say("  flat against torch.add: %.2f of its rate; general (count + apply) against torch.add: %.2f; apply alone: %.2f; norm against torch.norm: %.2f"
        % (flat_rate / torch_rate, nbytes["general"] / med["general"] / torch_rate, nbytes["general"] / apply_ms / torch_rate, med["torch.norm"] / med["norm"]))
    say("")
    say("norms and vectors: time against the yardstick of the same run (median / median; spread of the ratio over the alternations, sample by sample)")
    for k, y in (("gersh.N", "norm"), ("colnorm", "norm"), ("maxabs", "norm"), ("gersh.S", "norm.T"), ("scale.R", "torch.mul"), ("scale.L", "torch.mul")) + matvec_rows:
        r = sorted(x / z for x, z in zip(times[k], times[y]))
        say("  %-8s / %-9s  %.2f   (per alternation %.2f ... %.2f)" % (k, y, med[k] / med[y], r[0], r[-1]))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
