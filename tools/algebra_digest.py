#!/usr/bin/env python3
"""The bits of the matrix algebra between multiplies (dbcsr_amd/operations.py; kernels of dbcsr_amd/csrc/mm_algebra.h, mm_multivec.h, mm_rank_update.h,
mm_block_inverse.h over the block walk of mm_block_walk.h): one line per case with the case's name and the SHA-256 of every output -- the index arrays and the whole
data area (holes included) of a matrix, a vector, the 8 or 16 bytes of a scalar.

    python tools/algebra_digest.py --out digest.txt

These kernels promise the same bits on every call (no atomics, fixed summation orders), so the files that two builds of the library write must be EQUAL
byte for byte: a change that is meant to keep the kernels' results is checked by running this file, unchanged, in the checkout of either commit.  It
uses only dbcsr_amd's Python interface and the C-ABI entries behind it.

The matrix: 12 block rows and columns with the sizes 1, 2, 3, 5, 8, 13, 23, 32, 67, 70 (and 1 and 23 once more) in a seeded order, about half of the
blocks present, for float64, float32 and complex128.  Before any launch the host checks that it has what the walks branch on (check_shapes).  It is used
as built (packed), after an in-place filter (holes between the blocks), as the stored triangle of an 'S' / 'A' (complex: 'H' / 'K') matrix, and with a
data area that is not 16-byte aligned."""
import argparse
import ctypes as C
import hashlib
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dbcsr_amd import operations as ops  # noqa: E402
from dbcsr_amd.matrix import DbcsrMatrix, StreamHandle  # noqa: E402
from dbcsr_amd.multiply import MultiplyEngine  # noqa: E402

SIZES = [1, 2, 3, 5, 8, 13, 23, 32, 67, 70, 1, 23]
DTYPES = {"fp64": np.float64, "fp32": np.float32, "z64": np.complex128}
SCALARS = [(1.0, 1.0), (0.5, 1.0), (1.0, -2.5), (0.75, 1.5)]   # exactly 1 and not 1, on either side


def values(rng, shape, dtype):
    x = rng.uniform(-1.0, 1.0, shape)
    if np.dtype(dtype).kind == "c":
        x = x + 1j * rng.uniform(-1.0, 1.0, shape)
    return x.astype(dtype)


def host_matrix(sizes, mask, dtype, seed, triangle=False):
    """(row_p, col_i, blk_p, data) of the packed matrix with a column-major block wherever mask is set (ascending columns); triangle: the blocks on and
    above the diagonal, the diagonal blocks made symmetric / hermitian"""
    rng = np.random.default_rng(seed)
    nb = len(sizes)
    row_p, col_i, blk_p, data, at = [0], [], [], [], 0
    for r in range(nb):
        for c in range(nb):
            blk = values(rng, (sizes[r], sizes[c]), dtype)   # (drawn for every position: a block's values do not depend on the pattern)
            if not mask[r, c] or (triangle and c < r):
                continue
            if triangle and r == c:
                blk = (blk + blk.conj().T).astype(dtype)
            col_i.append(c)
            blk_p.append(at)
            data.append(blk.reshape(-1, order="F"))
            at += blk.size
        row_p.append(len(col_i))
    return (np.array(row_p, np.int32), np.array(col_i, np.int32), np.array(blk_p, np.int64),
            np.concatenate(data) if data else np.zeros(0, dtype))


def check_shapes(sizes, row_p, col_i, blk_p, dtype, what):
    """the matrix has every shape the walks take another path at (host only)"""
    V = 16 // np.dtype(dtype).itemsize
    rows = np.repeat(np.arange(len(sizes)), np.diff(row_p))
    m, n = np.array(sizes)[rows], np.array(sizes)[col_i]
    ne, head = m * n, (V - blk_p % V) % V
    need = {
        "every residue of blk_p modulo V": set(blk_p % V) == set(range(V)),
        "a block no longer than its head": bool(np.any((head > 0) & (ne <= head))) or V == 1,
        "a block shorter than its head": bool(np.any(ne < head)) or V < 4,
        "a block with no whole pack": bool(np.any((ne - np.minimum(head, ne)) // V == 0)) or V == 1,
        "a block with more than 64 V elements": bool(np.any(ne > 64 * V)),
        "a block row with m / gcd(V, m) > 64": bool(np.any(m // np.gcd(V, m) > 64)),
        "a block wider than 64 columns": bool(np.any(n > 64)),
        "a 64-column part above 1024 elements": bool(np.any(np.minimum(n, 64) * m > 1024)),
    }
    missing = [k for k, ok in need.items() if not ok]
    if missing:
        sys.exit("%s lacks: %s" % (what, "; ".join(missing)))


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def scalar_sha(x):
    return hashlib.sha256(np.asarray(x, dtype=np.complex128 if isinstance(x, complex) else np.float64).tobytes()).hexdigest()


def matrix_sha(M):
    return sha(M.row_p, M.col_i, M.blk_p, M.data)


class Cases:
    def __init__(self, eng, out):
        self.eng, self.out, self.count = eng, out, 0

    def add(self, name, digest):
        torch.cuda.synchronize()
        self.out.write("%s %s\n" % (name, digest))
        self.count += 1


def run_type(cases, tname, dtype):
    eng = cases.eng
    rng = np.random.default_rng(20240607)
    sizes = [SIZES[i] for i in rng.permutation(len(SIZES))]
    nb = len(sizes)
    mask = rng.random((nb, nb)) < 0.5
    mask[np.arange(nb), np.arange(nb)] = rng.random(nb) < 0.7              # (some block rows lack their diagonal block)
    other = (mask & (rng.random((nb, nb)) < 0.5)) | (~mask & (rng.random((nb, nb)) < 0.5))   # about half of its blocks shared with mask
    n = sum(sizes)
    st = StreamHandle()
    sz = torch.tensor(sizes, dtype=torch.int32, device="cuda")
    is_z = np.dtype(dtype).kind == "c"
    for tri in (False, True):
        check_shapes(sizes, *host_matrix(sizes, mask, dtype, 1, tri)[:3], dtype, "%s%s" % (tname, " (triangle)" if tri else ""))

    def dev(parts, symmetry="N"):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        return DbcsrMatrix(sz, sz, t(parts[0]), t(parts[1]), t(parts[2]), t(parts[3]), symmetry=symmetry)

    def with_holes():
        """the matrix' blocks where an in-place filter leaves them: between blocks that were there and fell below the threshold"""
        rp, ci, bp, full = host_matrix(sizes, mask | other, dtype, 1)
        rows = np.repeat(np.arange(nb), np.diff(rp))
        for b in range(len(ci)):
            if not mask[rows[b], ci[b]]:
                full[bp[b]:bp[b] + sizes[rows[b]] * sizes[ci[b]]] *= 1e-9
        out = eng.filtered(dev((rp, ci, bp, full)), 1e-6, in_place=True)
        torch.cuda.synchronize()
        assert not out.packed and out.nblks == int(mask.sum())
        return out

    def misaligned(M):
        big = torch.zeros(M.data.numel() + 3, dtype=M.data.dtype, device="cuda")
        view = big[1:1 + M.data.numel()]
        view.copy_(M.data)
        assert is_z or view.data_ptr() % 16 != 0
        return DbcsrMatrix(M.row_blk_size, M.col_blk_size, M.row_p, M.col_i, M.blk_p, view, symmetry=M.symmetry, nze=M.nze)

    sym1, sym2 = ("H", "K") if is_z else ("S", "A")

    def maker(vname):
        """make(): the matrix in this variant, afresh; make(pat, seed): another operand for it (packed), make(s=...): with another symmetry"""
        def make(pat=mask, seed=1, s=None):
            tri = vname == "triangle"
            if vname == "holes" and pat is mask and seed == 1:
                return with_holes()
            M = dev(host_matrix(sizes, pat, dtype, seed, tri), s or (sym1 if tri else "N"))
            return misaligned(M) if vname == "misaligned" else M
        return make

    vec = lambda seed, *shape: torch.from_numpy(values(np.random.default_rng(seed), shape, dtype)).cuda()
    za = (0.3 + 0.2j) if is_z else 0.3

    def padded(seed, nrhs):
        """an (n, nrhs) slice of a wider tensor: the padding columns belong to the digest (they are never written)"""
        big = vec(seed, n, nrhs + 3)
        return big, big[:, :nrhs]

    for vname in ("built", "holes", "triangle", "misaligned"):
        make = maker(vname)
        tag = "%s.%s" % (tname, vname)
        sym = make().symmetry
        # add: the same pattern, a union pattern with about half of the blocks shared, beta == 0
        for alpha, beta in SCALARS:
            A = make()
            ops.dbcsr_add(A, make(seed=2), alpha, beta, engine=eng)
            cases.add("%s add.same(%g,%g)" % (tag, alpha, beta), matrix_sha(A))
            A = make()
            ops.dbcsr_add(A, make(pat=other, seed=3), alpha, beta, engine=eng)
            cases.add("%s add.union(%g,%g)" % (tag, alpha, beta), matrix_sha(A))
        for alpha in (1.0, 0.5):
            A = make()
            ops.dbcsr_add(A, make(pat=other, seed=3), alpha, 0.0, engine=eng)
            cases.add("%s add.beta0(%g)" % (tag, alpha), matrix_sha(A))
        A = make()
        ops.dbcsr_scale(A, za, engine=eng)
        cases.add("%s scale" % tag, matrix_sha(A))
        A = make()
        ops.dbcsr_add_on_diag(A, za if sym == "N" else 0.3, engine=eng)
        cases.add("%s add_on_diag" % tag, matrix_sha(A))
        # reductions
        A = make()
        cases.add("%s trace" % tag, scalar_sha(ops.dbcsr_trace(A, engine=eng)))
        if not is_z:
            cases.add("%s dot.same" % tag, scalar_sha(ops.dbcsr_dot(A, make(seed=2), engine=eng)))
            cases.add("%s dot.union" % tag, scalar_sha(ops.dbcsr_dot(A, make(pat=other, seed=3), engine=eng)))
        cases.add("%s frobenius" % tag, scalar_sha(ops.dbcsr_frobenius_norm(A, engine=eng)))
        cases.add("%s maxabs" % tag, scalar_sha(ops.dbcsr_maxabs_norm(A, engine=eng)))
        cases.add("%s gershgorin" % tag, scalar_sha(ops.dbcsr_gershgorin_norm(A, engine=eng)))
        # sums of |x| and |x|^2 per full row and column, with and without the diagonal blocks (the C-ABI entries: the stored blocks as they are)
        a = A.desc()
        for what in (0, 1):
            out = torch.full((n,), -1.0, dtype=torch.float64, device="cuda")
            rc = eng.L.dbcsr_amd_bcsr_row_sums(eng.h, A.dtype_code, C.byref(a), what, out.data_ptr(), n, st.ptr)
            assert rc == 0, rc
            cases.add("%s row_sums(%d)" % (tag, what), sha(out))
            for skip in (0, 1):
                out = torch.full((n,), -1.0, dtype=torch.float64, device="cuda")
                rc = eng.L.dbcsr_amd_bcsr_col_sums(eng.h, A.dtype_code, C.byref(a), what, skip, out.data_ptr(), n, st.ptr)
                assert rc == 0, rc
                cases.add("%s col_sums(%d,skip=%d)" % (tag, what, skip), sha(out))
        if sym == "N":
            cases.add("%s norm.column" % tag, sha(ops.dbcsr_norm(A, ops.dbcsr_norm_column, engine=eng)))
        # the diagonal as a vector, scale by vector
        cases.add("%s get_diag" % tag, sha(ops.dbcsr_get_diag(A, engine=eng)))
        A = make()
        ops.dbcsr_set_diag(A, vec(5, n), engine=eng)
        cases.add("%s set_diag" % tag, matrix_sha(A))
        if sym == "N":
            for side in ("left", "right"):
                A = make()
                ops.dbcsr_scale_by_vector(A, vec(6, n), side, engine=eng)
                cases.add("%s scale_by_vector.%s" % (tag, side), matrix_sha(A))
        # matvec and multivec: every operation, every symmetry kind the type has
        for s in ((sym1, sym2) if sym != "N" else ("N",)):
            A = make(s=s)
            for trans in "NTC":
                for alpha, beta in ((1.0, 0.0), (1.25, -0.5)):
                    y = vec(8, n)
                    ops.dbcsr_matvec(A, vec(7, n), y, alpha, beta, trans, engine=eng)
                    cases.add("%s matvec.%s.%s(%g,%g)" % (tag, s, trans, alpha, beta), sha(y))
                for nrhs in (1, 16, 17, 64):
                    xbig, x = padded(9, nrhs)
                    ybig, y = padded(10, nrhs)
                    ops.dbcsr_multivec(A, x, y, 1.25, -0.5, trans, engine=eng)
                    cases.add("%s multivec.%s.%s(%d)" % (tag, s, trans, nrhs), sha(ybig))
        # one rank update: the header of its kernels includes the walk
        A = make()
        xbig, x = padded(11, 5)
        if sym == "N":
            ops.dbcsr_rank_update(A, x, padded(12, 5)[1], za, 0.5, "C" if is_z else "T", engine=eng)
        else:
            ops.dbcsr_rank_update(A, x, None, 0.3, 0.5, "C" if is_z else "T", engine=eng)
        cases.add("%s rank_update" % tag, matrix_sha(A))
        # the block diagonal: its copy, and every stored diagonal block inverted in place (blocks of 1 ... 70: the wave and the workgroup kernel)
        A = make()
        cases.add("%s get_block_diag" % tag, matrix_sha(ops.dbcsr_get_block_diag(A, engine=eng)))
        singular = ops.dbcsr_invert_block_diag(A, engine=eng)
        assert singular == (0, -1), singular
        cases.add("%s invert_block_diag" % tag, matrix_sha(A))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    t0 = time.time()
    with open(args.out, "w") as f:
        cases = Cases(MultiplyEngine(), f)
        for tname, dtype in DTYPES.items():
            run_type(cases, tname, dtype)
    print("%d cases in %.1f s -> %s" % (cases.count, time.time() - t0, args.out))


if __name__ == "__main__":
    main()
