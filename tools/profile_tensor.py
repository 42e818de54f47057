#!/usr/bin/env python
"""Times the re-folding of block-sparse tensors on the device (dbcsr_amd/tensor.py; kernel tensor_permute_blocks of dbcsr_amd/csrc/mm_tensor.h) and writes
profiles/tensor.txt.  One process; every variant is warmed, then the variants of a group alternate round by round; a sample is the mean of `calls` calls
between two device events; reported are median, min, max and spread = (max - min) / median over the samples.  GB/s = bytes read + written / time.

  1. one permute launch over a rank-3 tensor of about 1 GB of 23^3-element float64 blocks, for the identity and the five other permutations, against
     copy_ of the same bytes and against torch.permute(...).contiguous() of the uniform (nblk, 23, 23, 23) tensor that holds the same blocks;
  2. the same for 32^3 blocks, and float32 / complex128 at one permutation each;
  3. a contraction T3[i,j,l] = T1[i,j,k] T2[k,l]: with compatible mappings, and with T1 and T3 in foreign ones, split into remap in, multiply, remap out
     (host clock around a device synchronise: the multiply synchronises by itself);
  4. once: the host path that the remap replaces -- to_host(), a numpy loop over the blocks, from_host()."""
import argparse
import ctypes as C
import itertools
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dbcsr_amd.tensor as T  # noqa: E402
from dbcsr_amd.matrix import DbcsrMatrix, StreamHandle, _dtype_code  # noqa: E402
from dbcsr_amd.multiply import default_engine  # noqa: E402

LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def stat_line(name, samples, nbytes=None):
    med = float(np.median(samples))
    rate = "  %8.1f GB/s" % (nbytes / med / 1e6) if nbytes else ""
    say("  %-26s median %9.4f ms  min %9.4f  max %9.4f  spread %5.1f %%%s   samples: %s"
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


def alternate(variants, rounds, warm, calls, sample=device_sample):
    """{name: samples}: the variants take turns, round by round"""
    out = {name: [] for name, _ in variants}
    for r in range(warm + rounds):
        for name, fn in variants:
            s = sample(fn, calls)
            if r >= warm:
                out[name].append(s)
    return out


def full_tensor(nb, bs, mapping, dtype, fill=1.0, seed=0):
    """a tensor of nb blocks per dimension, all of size bs, about `fill` of them stored, random values; built on the device"""
    dev = torch.device("cuda")
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    sizes = [torch.full((n,), bs, dtype=torch.int32, device=dev) for n in nb]
    idx = torch.cartesian_prod(*[torch.arange(n, device=dev) for n in nb])
    if fill < 1.0:
        idx = idx[torch.rand(idx.shape[0], device=dev, generator=g) < fill]
    t = T.dbcsr_t_create(sizes, mapping[0], mapping[1], dtype)
    _, row_p, col_i, blk_p, nze = T.fold_index(idx, t.blk_sizes, t.map1, t.map2)
    if dtype.is_complex:
        data = torch.view_as_complex(torch.randn((int(nze), 2), dtype=torch.float64, device=dev, generator=g))
    else:
        data = torch.randn(int(nze), dtype=dtype, device=dev, generator=g)
    t.matrix.adopt(DbcsrMatrix(t.matrix.row_blk_size, t.matrix.col_blk_size, row_p, col_i, blk_p, data))
    return t


def permute_group(bs, dtype, perms, target_bytes, rounds, warm, calls, with_torch=True):
    item = torch.empty(0, dtype=dtype).element_size()
    n = bs ** 3
    nblk = max(1, int(target_bytes // (n * item)))
    dev = torch.device("cuda")
    src = torch.randn(nblk * n * (2 if dtype.is_complex else 1), dtype=torch.float64 if dtype.is_complex else dtype, device=dev)
    src = torch.view_as_complex(src.view(-1, 2)) if dtype.is_complex else src
    dst = torch.empty_like(src)
    ext = torch.ones((nblk, 4), dtype=torch.int32, device=dev)
    ext[:, :3] = bs
    off = torch.arange(nblk, dtype=torch.int64, device=dev) * n
    E, st, code = default_engine(), StreamHandle(), _dtype_code(dtype)
    nbytes = 2 * nblk * n * item
    say("%d blocks of %d^3 %s elements: %.1f MB read and as much written per launch" % (nblk, bs, str(dtype).replace("torch.", ""), nbytes / 2e6))

    def launch(perm):
        p = (C.c_int * 3)(*perm)

        def fn():
            rc = E.L.dbcsr_amd_tensor_permute_blocks(E.h, code, nblk, 3, p, ext.data_ptr(), off.data_ptr(), off.data_ptr(), src.data_ptr(), src.numel(),
                                                     dst.data_ptr(), dst.numel(), st.ptr)
            assert rc == 0
        return fn

    variants = [("copy_", lambda: dst.copy_(src))]
    uniform = src.view(nblk, bs, bs, bs)
    for perm in perms:
        variants.append(("permute %s" % (perm,), launch(perm)))
        if with_torch and perm != (0, 1, 2):
            order = [0] + [3 - perm[3 - t] for t in (1, 2, 3)]
            variants.append(("torch %s" % (perm,), lambda order=order: uniform.permute(order).contiguous()))
    # what is timed is what is tested: one check per permutation against torch
    for perm in perms:
        launch(perm)()
        order = [0] + [3 - perm[3 - t] for t in (1, 2, 3)]
        assert torch.equal(torch.view_as_real(dst) if dtype.is_complex else dst,
                           torch.view_as_real(uniform.permute(order).contiguous().view(-1)) if dtype.is_complex else uniform.permute(order).contiguous().view(-1))
    res = alternate(variants, rounds, warm, calls)
    med = {name: stat_line(name, s, nbytes) for name, s in res.items()}
    for perm in perms:
        k = "permute %s" % (perm,)
        line = "  %s / copy_: %.2f" % (k, med[k] / med["copy_"])
        if "torch %s" % (perm,) in med:
            line += "   / torch.permute().contiguous(): %.2f" % (med[k] / med["torch %s" % (perm,)])
        say(line)
    say()


def contraction_group(rounds, warm, calls):
    nb, bs = 20, 23
    dt = torch.float64
    compatible, foreign_1, foreign_3 = ((0, 1), (2,)), ((0,), (1, 2)), ((2, 0), (1,))
    t1c = full_tensor((nb, nb, nb), bs, compatible, dt, fill=0.3, seed=1)
    t2 = full_tensor((nb, nb), bs, ((0,), (1,)), dt, fill=0.5, seed=2)
    t1f = T._like(t1c, *foreign_1)
    T.dbcsr_t_copy(t1c, t1f)
    t3c = T._like(t1c, *compatible)
    t3f = T._like(t1c, *foreign_3)
    args = dict(contract_1=(2,), notcontract_1=(0, 1), contract_2=(0,), notcontract_2=(1,), map_1=(0, 1), map_2=(2,))
    flop = T.dbcsr_t_contract(1.0, t1c, t2, 0.0, t3c, **args)
    say("T3[i,j,l] = T1[i,j,k] T2[k,l], float64, %d blocks of %d per dimension: T1 %d blocks (%.1f MB), T2 %d blocks, T3 %d blocks (%.1f MB), %.2f GFLOP"
        % (nb, bs, t1c.nblks, t1c.matrix.nze * 8 / 1e6, t2.nblks, t3c.nblks, t3c.matrix.nze * 8 / 1e6, flop / 1e9))
    scratch_1, scratch_3 = T._like(t1c, *compatible), T._like(t1c, *foreign_3)
    variants = [
        ("contract, compatible", lambda: T.dbcsr_t_contract(1.0, t1c, t2, 0.0, t3c, **args)),
        ("contract, foreign T1 + T3", lambda: T.dbcsr_t_contract(1.0, t1f, t2, 0.0, t3f, **args)),
        ("remap in (T1)", lambda: T.dbcsr_t_copy(t1f, scratch_1)),
        ("remap out (T3)", lambda: T.dbcsr_t_copy(t3c, scratch_3)),
    ]
    T.reset_stats()
    T.dbcsr_t_contract(1.0, t1f, t2, 0.0, t3f, **args)
    say("  permute launches of the foreign contraction: %d (%d elements)" % (T.stats()["permute_launches"], T.stats()["permuted_elements"]))
    res = alternate(variants, rounds, warm, calls, sample=host_sample)
    med = {name: stat_line(name, s) for name, s in res.items()}
    say("  foreign / compatible: %.2f; remap in + remap out = %.4f ms, %.2f of the compatible contraction (index work by torch included)"
        % (med["contract, foreign T1 + T3"] / med["contract, compatible"], med["remap in (T1)"] + med["remap out (T3)"],
           (med["remap in (T1)"] + med["remap out (T3)"]) / med["contract, compatible"]))
    say()
    return t1f, compatible


def host_path(t_in, mapping_out):
    """to_host(), numpy per block, from_host(): what a caller had to do before"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rs, cs, row_p, col_i, blk_p, data = t_in.matrix.to_host()
    t1 = time.perf_counter()
    nb = t_in.nblks_per_dim
    sizes = [h for h in t_in._host_sizes]
    s_in, s_out = t_in.stored_order, mapping_out[0] + mapping_out[1]
    perm = [s_in.index(d) for d in s_out]
    rows = np.repeat(np.arange(len(rs)), np.diff(row_p))
    idx = np.zeros((len(col_i), len(nb)), np.int64)
    for lin, dims in ((rows.copy(), t_in.map1), (col_i.astype(np.int64), t_in.map2)):
        for d in dims:
            idx[:, d] = lin % nb[d]
            lin //= nb[d]
    key = np.zeros(len(col_i), np.int64)
    nbc = int(np.prod([nb[d] for d in mapping_out[1]]))
    for dims, scale in ((mapping_out[0], nbc), (mapping_out[1], 1)):
        lin, stride = np.zeros(len(col_i), np.int64), 1
        for d in dims:
            lin += idx[:, d] * stride
            stride *= nb[d]
        key += lin * scale
    order = np.argsort(key, kind="stable")
    out = np.empty_like(data)
    at = 0
    new_blk_p = np.zeros(len(order), np.int64)
    for k, b in enumerate(order):
        e = [int(sizes[d][idx[b, d]]) for d in s_in]
        n = int(np.prod(e))
        out[at:at + n] = np.transpose(data[blk_p[b]:blk_p[b] + n].reshape(e, order="F"), perm).reshape(-1, order="F")
        new_blk_p[k] = at
        at += n
    t2 = time.perf_counter()
    dev = torch.as_tensor(out).cuda()
    torch.as_tensor(new_blk_p).cuda()
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    say("the host path, once, for T1 of the contraction (%d blocks, %.1f MB): to_host %.1f ms, numpy loop over the blocks %.1f ms, back to the device %.1f ms, "
        "together %.1f ms" % (len(order), data.nbytes / 1e6, 1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t3 - t2), 1e3 * (t3 - t0)))
    return dev


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "tensor.txt"))
    ap.add_argument("--bytes", type=float, default=1.0e9, help="bytes of blocks per launch in the permute groups")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--calls", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("profile_tensor.py measures on the GPU; none is available")
    say("re-folding of block-sparse tensors; %s" % torch.cuda.get_device_name(0))
    say("%d alternations after %d warm-up rounds, %d calls per sample; ms per call; GB/s = (bytes read + written) / time" % (a.rounds, a.warm, a.calls))
    say()
    perms = list(itertools.permutations(range(3)))
    permute_group(23, torch.float64, perms, a.bytes, a.rounds, a.warm, a.calls)
    permute_group(32, torch.float64, perms, a.bytes, a.rounds, a.warm, a.calls)
    permute_group(23, torch.float32, [(2, 1, 0)], a.bytes, a.rounds, a.warm, a.calls)
    permute_group(23, torch.complex128, [(2, 1, 0)], a.bytes, a.rounds, a.warm, a.calls)
    t1f, compatible = contraction_group(a.rounds, a.warm, a.calls)
    host_path(t1f, compatible)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
