#!/usr/bin/env python
"""Times re-blocking on the device (dbcsr_amd/reblock.py; kernels of dbcsr_amd/csrc/mm_reblock.h) and writes profiles/reblock.txt.  One process; every
variant is warmed, then the variants of a group alternate round by round; reported are median, min, max and spread = (max - min) / median over the
samples.  A sample of an asynchronous call is the mean of `calls` calls between two device events; a sample of a call that synchronises by itself
(dbcsr_reblock, the CSR and dense routes, a multiply) is a host clock around it, ended by a device synchronise.  GB/s = bytes read + written / time.

Workload: float64, 504 x 504 blocks of 23 x 23 (n = 11592), full and at one block in ten, re-blocked to
    u32      uniform blocks of 32 (a tail of 8): no boundary but every 736th element is one of the source's -- consecutive 23s cannot be merged to 32
    m46      dbcsr_merged_block_sizes(., 64): consecutive pairs, blocks of 46
    s12      dbcsr_split_block_sizes(., 12): every block cut into 12 + 11
  1. dbcsr_reblock and dbcsr_reblock_into (there, onto the pattern dbcsr_reblock made, and back, onto the source's pattern) against copy_ of the data
     area (the floor), dbcsr_to_csr -> dbcsr_create_from_csr and dbcsr_to_dense -> dbcsr_create_from_dense;
  2. the steps of dbcsr_reblock one by one, each ended by a synchronise: name the pieces (count and list), the reserve's count, the index apply, the gather;
  3. the point of it all: a warm dbcsr_multiply A A in 23-blocks against the same product in 46-blocks with both conversions included -- the operands
     brought over with dbcsr_reblock_into onto resident merged matrices (their index stays, so the merged multiply reuses its plan too) and the
     product brought back onto the pattern of the 23-block product."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dbcsr_amd.csr import dbcsr_create_from_csr, dbcsr_to_csr  # noqa: E402
from dbcsr_amd.matrix import DbcsrMatrix, StreamHandle  # noqa: E402
from dbcsr_amd.multiply import MultiplyEngine, dbcsr_multiply  # noqa: E402
from dbcsr_amd.operations import dbcsr_create_from_dense, dbcsr_to_dense  # noqa: E402
from dbcsr_amd.reblock import dbcsr_merged_block_sizes, dbcsr_reblock, dbcsr_reblock_into, dbcsr_split_block_sizes  # noqa: E402

LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def stat_line(name, samples, nbytes=None):
    med = float(np.median(samples))
    rate = "  %8.1f GB/s" % (nbytes / med / 1e6) if nbytes else " " * 15
    say("  %-24s median %9.4f ms  min %9.4f  max %9.4f  spread %5.1f %%%s   samples: %s"
        % (name, med, min(samples), max(samples), 100.0 * (max(samples) - min(samples)) / med, rate, " ".join("%.4f" % s for s in samples)))
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


def matrix(nb, bs, fill, seed):
    """nb x nb blocks of bs x bs, about `fill` of them stored, random float64 values; built on the device, packed"""
    dev = torch.device("cuda")
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    sizes = torch.full((nb,), bs, dtype=torch.int32, device=dev)
    keep = torch.ones(nb * nb, dtype=torch.bool, device=dev) if fill >= 1.0 else torch.rand(nb * nb, device=dev, generator=g) < fill
    idx = torch.nonzero(keep).flatten()
    rows, cols = idx // nb, idx % nb
    row_p = torch.zeros(nb + 1, dtype=torch.int32, device=dev)
    row_p[1:] = torch.cumsum(torch.bincount(rows, minlength=nb), 0).to(torch.int32)
    blk_p = torch.arange(idx.numel(), dtype=torch.int64, device=dev) * (bs * bs)
    data = torch.randn(idx.numel() * bs * bs, dtype=torch.float64, device=dev, generator=g)
    return DbcsrMatrix(sizes, sizes, row_p, cols.to(torch.int32).contiguous(), blk_p, data)


def steps_of_reblock(E, A, rs, cs):
    """the C calls of dbcsr_reblock one by one, a synchronise and a host clock after each: (name, reserve count, index apply, gather) in ms"""
    st = StreamHandle()
    dev = A.row_p.device
    nbr, nbc = int(rs.numel()), int(cs.numel())
    out = []

    def lap(t0):
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
        return time.perf_counter()
    torch.cuda.synchronize()
    t = time.perf_counter()
    src, total = A.desc(), C.c_int64()
    assert E.L.dbcsr_amd_bcsr_reblock_name_blocks(E.h, C.byref(src), rs.data_ptr(), cs.data_ptr(), nbr, nbc, C.byref(total), None, None, st.ptr) == 0
    n = total.value
    rows, cols = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    assert E.L.dbcsr_amd_bcsr_reblock_name_blocks(E.h, C.byref(src), rs.data_ptr(), cs.data_ptr(), nbr, nbc, C.byref(total), rows.data_ptr(),
                                                  cols.data_ptr(), st.ptr) == 0
    t = lap(t)
    M = DbcsrMatrix.empty_like_pattern(rs, cs, A.dtype, device=dev)
    m = M.desc()
    row_p = torch.empty(nbr + 1, dtype=torch.int32, device=dev)
    nb, nz, new, bad = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
    assert E.L.dbcsr_amd_bcsr_reserve_count(E.h, C.byref(m), n, rows.data_ptr(), cols.data_ptr(), 0, row_p.data_ptr(), C.byref(nb), C.byref(nz),
                                            C.byref(new), C.byref(bad), st.ptr) == 0 and bad.value == 0
    t = lap(t)
    res = DbcsrMatrix(rs, cs, row_p, torch.empty(nb.value, dtype=torch.int32, device=dev), torch.empty(nb.value, dtype=torch.int64, device=dev),
                      torch.empty(nz.value, dtype=A.dtype, device=dev))
    dst = res.desc(out=True)
    assert E.L.dbcsr_amd_bcsr_reserve_apply_index(E.h, C.byref(m), C.byref(dst), st.ptr) == 0
    t = lap(t)
    d = res.desc()
    assert E.L.dbcsr_amd_bcsr_reblock_gather(E.h, A.dtype_code, C.byref(src), C.byref(d), st.ptr) == 0
    lap(t)
    return out, n


def conversions(E, A, label, structures, rounds, warm, calls, dense_fits):
    dev = A.row_p.device
    item = A.data.element_size()
    say("%s: %d blocks, %.1f MB of blocks" % (label, A.nblks, A.data.numel() * item / 1e6))
    scratch = torch.empty_like(A.data)
    back = A.copy()
    for tag, (rs, cs) in structures.items():
        rs_d, cs_d = (torch.as_tensor(np.asarray(x, np.int32)).to(dev) for x in (rs, cs))
        Y = dbcsr_reblock(A, rs_d, cs_d, engine=E)
        moved = (A.data.numel() + Y.data.numel()) * item
        say(" to %s: %d x %d blocks, %d stored, %.1f MB" % (tag, len(rs), len(cs), Y.nblks, Y.data.numel() * item / 1e6))

        def csr_route():
            return dbcsr_create_from_csr(*dbcsr_to_csr(A, engine=E), rs_d, cs_d, engine=E)

        def dense_route():
            return dbcsr_create_from_dense(dbcsr_to_dense(A, engine=E), rs_d, cs_d, engine=E)
        variants = [("copy_ (floor)", lambda: scratch.copy_(A.data), device_sample, calls),
                    ("dbcsr_reblock", lambda: dbcsr_reblock(A, rs_d, cs_d, engine=E), host_sample, 1),
                    ("reblock_into (there)", lambda: dbcsr_reblock_into(A, Y, engine=E), device_sample, calls),
                    ("reblock_into (back)", lambda: dbcsr_reblock_into(Y, back, engine=E), device_sample, calls),
                    ("to_csr -> from_csr", csr_route, host_sample, 1)]
        if dense_fits:
            variants.append(("to_dense -> from_dense", dense_route, host_sample, 1))
        got = alternate(variants, rounds, warm)
        med = {}
        for name, _, _, _ in variants:
            med[name] = stat_line(name, got[name], 2 * A.data.numel() * item if name.startswith("copy_") else (moved if "reblock" in name else None))
        assert torch.equal(back.data.view(torch.int64), A.data.view(torch.int64)), "the way back must give the source bit for bit"
        floor = med["copy_ (floor)"]
        say("  ratios (median / median): reblock / copy %.2f, into (there) / copy %.2f, into (back) / copy %.2f, csr route / reblock %.1f%s"
            % (med["dbcsr_reblock"] / floor, med["reblock_into (there)"] / floor, med["reblock_into (back)"] / floor,
               med["to_csr -> from_csr"] / med["dbcsr_reblock"],
               ", dense route / reblock %.1f" % (med["to_dense -> from_dense"] / med["dbcsr_reblock"]) if dense_fits else ""))
        laps = []
        for r in range(warm + rounds):
            one, n = steps_of_reblock(E, A, rs_d, cs_d)
            if r >= warm:
                laps.append(one)
        laps = np.median(np.asarray(laps), axis=0)
        say("  steps of dbcsr_reblock, each ended by a synchronise (medians): name %d pieces %.4f ms, reserve count %.4f, index apply %.4f, gather %.4f: "
            "the index step is %.0f %% of the four" % (n, laps[0], laps[1], laps[2], laps[3], 100.0 * laps[:3].sum() / laps.sum()))
        del Y
    say()


def the_point(E, A, rounds, warm):
    """C = A A warm in 23-blocks, against the product in 46-blocks with the conversions included"""
    dev = A.row_p.device
    merged = dbcsr_merged_block_sizes([23] * A.nblkrows, 64)
    m_d = torch.as_tensor(np.asarray(merged, np.int32)).to(dev)
    Cm = DbcsrMatrix.empty_like_pattern(A.row_blk_size, A.col_blk_size, A.dtype, device=dev)
    dbcsr_multiply("N", "N", 1.0, A, A, 0.0, Cm, engine=E)
    mA = dbcsr_reblock(A, m_d, m_d, engine=E)
    mC = DbcsrMatrix.empty_like_pattern(m_d, m_d, A.dtype, device=dev)
    dbcsr_multiply("N", "N", 1.0, mA, mA, 0.0, mC, engine=E)
    back = Cm.copy()
    E2 = MultiplyEngine()   # (an engine per blocking: each keeps the plan of its multiply)

    def plain():
        dbcsr_multiply("N", "N", 1.0, A, A, 0.0, Cm, engine=E)

    def in_merged():
        dbcsr_reblock_into(A, mA, engine=E2)
        dbcsr_multiply("N", "N", 1.0, mA, mA, 0.0, mC, engine=E2)
        dbcsr_reblock_into(mC, back, engine=E2)

    def merged_alone():
        dbcsr_multiply("N", "N", 1.0, mA, mA, 0.0, mC, engine=E2)
    got = alternate([("multiply in 23-blocks", plain, host_sample, 1), ("in 46-blocks, converted", in_merged, host_sample, 1),
                     ("in 46-blocks, multiply", merged_alone, host_sample, 1)], rounds, warm + 1)
    med = {k: stat_line(k, v) for k, v in got.items()}
    torch.cuda.synchronize()
    err = float((back.data - Cm.data).abs().max() / Cm.data.abs().max())
    say("  product in 46-blocks brought back against the product in 23-blocks: max |difference| / max |C| = %.2e (the sums run in another order)" % err)
    say("  plans reused / symbolic phases: 23-blocks %s, 46-blocks %s" % (E.plan_stats(), E2.plan_stats()))
    say("  ratio (median / median): in 46-blocks with both conversions / in 23-blocks %.3f" % (med["in 46-blocks, converted"] / med["multiply in 23-blocks"]))
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nb", type=int, default=504)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "reblock.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU: there is no fallback"
    E = MultiplyEngine()
    n = 23 * a.nb
    sizes = [23] * a.nb
    u32 = [32] * (n // 32) + ([n % 32] if n % 32 else [])
    structures = {"u32": (u32, u32), "m46": (dbcsr_merged_block_sizes(sizes, 64),) * 2, "s12": (dbcsr_split_block_sizes(sizes, 12),) * 2}
    say("re-blocking, float64, %d x %d blocks of 23 x 23 (n = %d); %s" % (a.nb, a.nb, n, torch.cuda.get_device_name(0)))
    say("%d alternations after %d warm-up round(s), %d calls per device-event sample, 1 call per host-clock sample; ms per call; GB/s = 8 * (elements read + "
        "written) / time" % (a.rounds, a.warm, a.calls))
    say()
    for fill, seed in ((1.0, 1), (0.1, 2)):
        A = matrix(a.nb, 23, fill, seed)
        conversions(E, A, "%d x %d blocks of 23 x 23, fill %.2f" % (a.nb, a.nb, fill), structures, a.rounds, a.warm, a.calls, dense_fits=True)
        say("the point, fill %.2f: C = A A" % fill)
        the_point(E, A, a.rounds, a.warm)
        del A
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
