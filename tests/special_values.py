"""Inf, NaN and extreme magnitudes in the operands of the device kernels: the helpers of tests/test_special_values_cpu.py (the conditions on the
inputs, oracle only) and tests/test_gpu_special_values.py (the device against the oracle).  Nothing here touches a GPU.

The class rule.  The class of a sum does not depend on the order of its terms as long as no finite partial sum overflows: NaN if a term is NaN or if
Inf of both signs occurs, otherwise +-Inf if a term is Inf, otherwise finite.  A product of two operands has one class as long as no operand is exactly
zero (0 x Inf would be NaN) and no finite product overflows.  So with operands that hold no zero and whose finite values are at most 10 in magnitude
the oracle's classes are the reference for every summation order a kernel uses -- element by element, no tolerance.  A kernel that pads a block to its
tile and multiplies the padding of one operand (zeros) by whatever the other operand's lanes read there breaks exactly this: 0 x Inf = NaN.

seed() puts the non-finite values where such reads happen: element (0, c) of a B block (the tail k step of the exact-size kernels reads it for the
lanes past the end), the last element of a block (the neighbour of the next block's first), the first and the last block of a data area."""
import functools

import numpy as np

from oracle import oracle as O

FINITE, PINF, NINF, NAN = 0, 1, 2, 3
F64, F32, Z64 = np.float64, np.float32, np.complex128
TOL = {np.dtype(F64): 1e-10, np.dtype(F32): 1e-5, np.dtype(Z64): 1e-10}
ALPHA, BETA = 0.7, 1.3


def bcsr(M, data):
    return O.Bcsr(M.row_sizes, M.col_sizes, M.row_p, M.col_i, M.blk_p, data)


def classes(x):
    """0 finite, 1 +Inf, 2 -Inf, 3 NaN per element; complex data: per component, shape (..., 2)"""
    x = np.asarray(x)
    if x.dtype.kind == "c":
        return np.stack([classes(x.real), classes(x.imag)], axis=-1)
    c = np.zeros(x.shape, np.int8)
    c[np.isposinf(x)] = PINF
    c[np.isneginf(x)] = NINF
    c[np.isnan(x)] = NAN
    return c


def block_sizes(M):
    return M.row_sizes[M.rows()].astype(np.int64) * M.col_sizes[M.col_i]


def gathered(M):
    """the blocks of M in index order, one after the other (the packed form of an unpacked matrix)"""
    if M.nblks == 0:
        return M.data[:0]
    return np.concatenate([M.data[p:p + n] for p, n in zip(M.blk_p, block_sizes(M))])


def packed(M):
    size = block_sizes(M)
    blk_p = np.concatenate([[0], np.cumsum(size)[:-1]]).astype(np.int64) if len(size) else np.zeros(0, np.int64)
    if np.array_equal(blk_p, M.blk_p) and M.data.size == int(size.sum()):
        return M
    return O.Bcsr(M.row_sizes, M.col_sizes, M.row_p, M.col_i, blk_p, gathered(M))


def where_is(M, e):
    """(block, block row, block column, row, column) of element e of M's packed data area"""
    b = int(np.searchsorted(M.blk_p, e, side="right")) - 1
    r, c = int(M.rows()[b]), int(M.col_i[b])
    t = int(e - M.blk_p[b])
    m = int(M.row_sizes[r])
    return b, r, c, t % m, t // m


def column_mask(M, columns):
    """True on the elements of M's data area that lie in column c of a block of block column nb, for every (nb, c) of columns"""
    mask = np.zeros(M.data.size, bool)
    rows = M.rows()
    for b in range(M.nblks):
        m = int(M.row_sizes[rows[b]])
        for nb, c in columns:
            if int(M.col_i[b]) == nb:
                mask[M.blk_p[b] + m * c:M.blk_p[b] + m * (c + 1)] = True
    return mask


def tail_columns(placed):
    """the (C block column, column) pairs that element (0, c) of a B block with +Inf there feeds: what the lanes past the end of K read in the last k
    step of the exact-size fp64 kernel.  Every block row counts, whether A has the block that meets the B block or not."""
    return sorted({(p["block_col"], p["col"]) for p in placed if p["matrix"] == "B" and p["row"] == 0 and np.isposinf(np.real(p["value"]))})


def assert_same(out, ref, tol, kernel="", blk_p=True, only=None, columns=()):
    """out (device) against ref (oracle): the same index arrays, the same class in every element, and on the finite elements the elementwise relative
    error of the neighbouring files (complex: modulus of the difference over the modulus of the reference, on the elements finite in both components).
    blk_p=False: an unpacked result (the in-place filter) -- its blocks are compared in index order.  only="outside" / "inside" with columns (see
    column_mask): the elements outside / inside those columns of C alone are compared."""
    assert np.array_equal(out.row_p, ref.row_p) and np.array_equal(out.col_i, ref.col_i), "%s: the block index differs from the oracle's" % kernel
    if blk_p:
        assert np.array_equal(out.blk_p, ref.blk_p), "%s: blk_p differs from the oracle's" % kernel
    else:
        out, ref = packed(out), packed(ref)
    assert out.data.size == ref.data.size
    if only is not None:
        sel = column_mask(ref, columns)
        sel = sel if only == "inside" else ~sel
        assert np.any(sel), "nothing to compare %s the columns" % only
        keep = np.flatnonzero(sel)
        full_out, full_ref = out, ref
        # (the comparison below on the selected elements; positions are reported in the whole data area)
        out, ref = bcsr(full_out, full_out.data[sel]), bcsr(full_ref, full_ref.data[sel])
        where = lambda e: where_is(full_ref, int(keep[e]))
    else:
        where = lambda e: where_is(ref, e)
    co, cr = classes(out.data), classes(ref.data)
    describe = lambda e: "C block %d (%d, %d) element (%d, %d)" % where(e) + ", kernel %s: device %r, oracle %r" % (kernel, out.data[e], ref.data[e])
    bad = np.flatnonzero((co != cr).reshape(co.shape[0], -1).any(axis=1)) if co.size else np.zeros(0, np.int64)
    if bad.size:
        print("%d of %d elements differ in class; the first:" % (bad.size, ref.data.size))
        for e in bad[:8]:
            print("  " + describe(int(e)))
    assert bad.size == 0, "%d elements differ in class, first: %s" % (bad.size, describe(int(bad[0])))
    fin = (cr == FINITE).reshape(cr.shape[0], -1).all(axis=1) if cr.size else np.zeros(0, bool)
    o, r = out.data[fin], ref.data[fin]
    if r.size == 0:
        return 0.0
    wide = np.complex128 if r.dtype.kind == "c" else np.float64
    err = np.abs(o.astype(wide) - r.astype(wide)) / np.maximum(np.abs(r.astype(wide)), 1e-300)
    w = int(np.argmax(err))
    if err[w] > tol:
        print("relative error %.3e above %.1e: %s" % (err[w], tol, describe(int(np.flatnonzero(fin)[w]))))
    assert err[w] <= tol, "relative error %.3e above %.1e: %s" % (err[w], tol, describe(int(np.flatnonzero(fin)[w])))
    return float(err[w])


# ---- seeding --------------------------------------------------------------------------------------------------------------------------------------------
def _pattern(M):
    P = np.zeros((M.nbr, M.nbc), bool)
    P[M.rows(), M.col_i] = True
    return P


def _dominant(M):
    """the most frequent (rows, columns) of M's blocks"""
    m, n = M.row_sizes[M.rows()], M.col_sizes[M.col_i]
    pairs, counts = np.unique(np.stack([m, n], 1), axis=0, return_counts=True)
    return tuple(int(v) for v in pairs[np.argmax(counts)])


def tail_flags(M):
    """per block: in the last block row or column, with a size there that is not the dominant one"""
    r, c = M.rows(), M.col_i
    dm, dn = _dominant(M)
    return ((r == M.nbr - 1) & (M.row_sizes[r] != dm)) | ((c == M.nbc - 1) & (M.col_sizes[c] != dn))


def _complex(re, im, dtype=np.complex128):
    """re + i im without a product by i (i x Inf would put a NaN into the real part)"""
    z = np.empty(np.shape(re), dtype)
    z.real, z.imag = re, im
    return z


class _Seeder:
    def __init__(self, M, name, rng):
        self.M, self.name, self.rng = M, name, rng
        self.order = np.argsort(M.blk_p, kind="stable")   # blocks in the order of the data area
        self.used, self.inf_blocks, self.placed = set(), set(), []
        self.rows = M.rows()
        self.dom = _dominant(M)
        self.tail = tail_flags(M)
        self.pos = np.empty(M.nblks, np.int64)
        self.pos[self.order] = np.arange(M.nblks)

    def dims(self, b):
        return int(self.M.row_sizes[self.rows[b]]), int(self.M.col_sizes[self.M.col_i[b]])

    def put(self, b, r, c, value, role):
        M = self.M
        m, n = self.dims(b)
        r, c = (m - 1 if r < 0 else r), (n - 1 if c < 0 else c)
        e = int(M.blk_p[b]) + r + m * c
        if M.data.dtype.kind == "c":
            if np.isnan(value):   # NaN in either component
                value = complex(np.nan, M.data[e].imag) if self.rng.integers(2) else complex(M.data[e].real, np.nan)
            else:                 # Inf in the real part only; the imaginary part stays finite and non-zero
                value = complex(value, M.data[e].imag)
        M.data[e] = value
        self.used.add(int(b))
        if not np.isnan(value):
            self.inf_blocks.add(int(b))
        pos = int(self.pos[b])
        self.placed.append(dict(matrix=self.name, block=int(b), block_row=int(self.rows[b]), block_col=int(M.col_i[b]), row=r, col=c, value=value, role=role,
                                first=pos == 0, last=pos == M.nblks - 1, dominant=self.dims(b) == self.dom, tail=bool(self.tail[b])))

    def free(self, cand):
        return [int(b) for b in cand if int(b) not in self.used]

    def pick(self, want=None, near=None):
        """an unused block: the one nearest (in the data area) to position near that satisfies want; without near: drawn by the generator"""
        cand = self.free(self.order)
        good = [b for b in cand if want is None or want(b)] or cand
        if not good:
            return None
        if near is None:
            return good[int(self.rng.integers(len(good)))]
        return min(good, key=lambda b: abs(int(self.pos[b]) - near))


def seed(A, B, Cm, rng, beta=1.0, transa="N", transb="N", rounds=1, retain=False):
    """Copies of the operands with a few elements replaced by non-finite values, and the list of what was put where (positions in terms of op(A) and
    op(B); a transposed operand is seeded in its op() form and stored back).  Per round, in B: +Inf at element (0, c) of three blocks -- the first
    and the last of the data area and a block of the dominant size in the middle --, -Inf at the last element of a tail-size block, one NaN; in A:
    -Inf at (r, 0) of the first block, +Inf at the last element of the last block, one NaN in a block that shares no product with an Inf-seeded
    block and reaches at least five C blocks free of Inf where the structure allows; in C when beta != 0: one +Inf.  Rounds after the first draw their
    blocks with the generator (more seeds for a case with many blocks).  retain: only the blocks C already has count as reached."""
    opA = O.transposed(A) if transa != "N" else A
    opB = O.transposed(B) if transb != "N" else B
    opA, opB, Cs = bcsr(opA, opA.data.copy()), bcsr(opB, opB.data.copy()), bcsr(Cm, Cm.data.copy())
    sa, sb, sc = _Seeder(opA, "A", rng), _Seeder(opB, "B", rng), _Seeder(Cs, "C", rng)
    PA, PB = _pattern(opA), _pattern(opB)
    PC = _pattern(Cs) if retain else np.ones((opA.nbr, opB.nbc), bool)
    for rnd in range(rounds):
        first = rnd == 0
        # B: the tail read of the exact-size kernels, both ends of the data area, a NaN
        for role, near, want in (("first", 0, None), ("last", opB.nblks - 1, None), ("middle", opB.nblks // 2, lambda b: sb.dims(b) == sb.dom)):
            b = sb.pick(want, near if first else None)
            if b is not None:
                sb.put(b, 0, int(rng.integers(sb.dims(b)[1])), np.inf, "B +Inf at (0, c), " + role)
        b = sb.pick(lambda b: sb.tail[b], opB.nblks - 1 if first else None)
        if b is not None:
            sb.put(b, -1, -1, -np.inf, "B -Inf at (k-1, n-1)")
        # A: both ends of the data area
        b = sa.pick(None, 0 if first else None)
        if b is not None:
            sa.put(b, int(rng.integers(sa.dims(b)[0])), 0, -np.inf, "A -Inf at (r, 0)")
        b = sa.pick(lambda b: sa.tail[b] or first, opA.nblks - 1 if first else None)
        if b is not None:
            sa.put(b, -1, -1, np.inf, "A +Inf at (m-1, k-1)")
    # which C blocks receive an Inf, from the block structure
    SA, SB = np.zeros_like(PA), np.zeros_like(PB)
    for b in sa.inf_blocks:
        SA[sa.rows[b], opA.col_i[b]] = True
    for b in sb.inf_blocks:
        SB[sb.rows[b], opB.col_i[b]] = True
    inf_c = (SA.astype(np.int32) @ PB.astype(np.int32) + PA.astype(np.int32) @ SB.astype(np.int32)) > 0
    for rnd in range(rounds):
        # B's NaN: any unused block
        b = sb.pick(None, None)
        if b is not None:
            m, n = sb.dims(b)
            sb.put(b, int(rng.integers(m)), int(rng.integers(n)), np.nan, "B NaN")
        # A's NaN: no product with an Inf-seeded block of B, and as many Inf-free C blocks as the structure gives (five are enough)
        def clean_targets(b):
            i, kb = int(sa.rows[b]), int(opA.col_i[b])
            return 0 if SB[kb].any() else int(np.count_nonzero(PB[kb] & PC[i] & ~inf_c[i]))
        cand = sa.free(sa.order)
        if cand:
            mid = opA.nblks // 2
            cand.sort(key=lambda b: abs(int(sa.pos[b]) - mid))
            enough = [b for b in cand if clean_targets(b) >= 5]
            if not any(p["dominant"] for p in sa.placed):   # a block of the dominant size among A's seeded blocks
                enough = [b for b in enough if sa.dims(b) == sa.dom] or enough
            b = enough[0] if enough else max(cand, key=clean_targets)
            m, n = sa.dims(b)
            sa.put(b, int(rng.integers(m)), int(rng.integers(n)), np.nan, "A NaN")
    if beta != 0 and Cs.nblks:
        b = sc.pick(None, Cs.nblks // 2)
        m, n = sc.dims(b)
        sc.put(b, int(rng.integers(m)), int(rng.integers(n)), np.inf, "C +Inf")
    outA = O.transposed(opA) if transa != "N" else opA
    outB = O.transposed(opB) if transb != "N" else opB
    return outA, outB, Cs, sa.placed + sb.placed + sc.placed


# ---- references ---------------------------------------------------------------------------------------------------------------------------------------
def typed(M, dtype, seed_):
    """the oracle's float64 matrix in the case's data type; complex: uniform(0.1, 1) imaginary parts laid over it (no zero component)"""
    if np.dtype(dtype).kind == "c":
        return bcsr(M, _complex(M.data, np.random.default_rng(seed_).uniform(0.1, 1.0, M.data.size), dtype))
    return bcsr(M, M.data.astype(dtype))


def on_pattern(M, ref):
    """M's elements in ref's layout (ref's pattern holds M's), zeros in the blocks M does not have"""
    out = np.zeros(ref.data.size, M.data.dtype)
    where = {rc: b for b, rc in enumerate(zip(ref.rows().tolist(), ref.col_i.tolist()))}
    size = block_sizes(M)
    for b, rc in enumerate(zip(M.rows().tolist(), M.col_i.tolist())):
        t = where[rc]
        out[ref.blk_p[t]:ref.blk_p[t] + size[b]] = M.data[M.blk_p[b]:M.blk_p[b] + size[b]]
    return out


def oracle_multiply(ta, tb, alpha, A, B, beta, Cm, **kw):
    """the oracle's multiply in float64.  Complex data: P = op(A) op(B) from the oracle's four real multiplies (on C's pattern, the old C zeroed),
    then alpha P + beta C written out on the real parts, every product of two components on its own -- complex arithmetic as the kernels and the
    reference's Fortran do it.  (A scalar with a zero component multiplies an Inf of the other operand's by it: 0.7 + 0 i times Inf is NaN + NaN i in
    that arithmetic.  The cases give complex data scalars without a zero component.)"""
    if A.data.dtype.kind != "c":
        w = lambda M: bcsr(M, M.data.astype(np.float64))
        return O.multiply(ta, tb, alpha, w(A), w(B), beta, w(Cm), **kw)
    assert beta != 0, "complex cases run with beta != 0"
    re, im = (lambda M: bcsr(M, np.ascontiguousarray(M.data.real))), (lambda M: bcsr(M, np.ascontiguousarray(M.data.imag)))
    zero = bcsr(Cm, np.zeros(Cm.data.size))
    rr, info = O.multiply(ta, tb, 1.0, re(A), re(B), 1.0, zero, **kw)
    ii, _ = O.multiply(ta, tb, 1.0, im(A), im(B), 1.0, zero, **kw)
    ri, _ = O.multiply(ta, tb, 1.0, re(A), im(B), 1.0, zero, **kw)
    ir, _ = O.multiply(ta, tb, 1.0, im(A), re(B), 1.0, zero, **kw)
    assert all(np.array_equal(x.col_i, rr.col_i) and np.array_equal(x.blk_p, rr.blk_p) for x in (ii, ri, ir))
    a, b = complex(alpha), complex(beta)
    c = on_pattern(Cm, rr)
    with np.errstate(invalid="ignore"):
        pr, pi = rr.data - ii.data, ri.data + ir.data
        return bcsr(rr, _complex(a.real * pr - a.imag * pi + (b.real * c.real - b.imag * c.imag),
                                 a.real * pi + a.imag * pr + (b.real * c.imag + b.imag * c.real))), info


def block_class_summary(Cref):
    """per C block: holds a non-finite element, holds NaN, holds Inf; and whether some block has a column that is Inf in every element (and NaN in none)"""
    cl = classes(Cref.data)
    if cl.ndim == 2:   # complex: the worse of the two components (NaN over Inf over finite) for the block statistics
        cl = cl.max(axis=1)
    size = block_sizes(Cref)
    rows = Cref.rows()
    nonfinite, has_nan, has_inf, inf_column = [], [], [], False
    for b in range(Cref.nblks):
        blk = cl[Cref.blk_p[b]:Cref.blk_p[b] + size[b]]
        nonfinite.append(bool(np.any(blk != FINITE)))
        has_nan.append(bool(np.any(blk == NAN)))
        has_inf.append(bool(np.any((blk == PINF) | (blk == NINF))))
        m = int(Cref.row_sizes[rows[b]])
        cols = blk.reshape(-1, m)   # [column][row]
        inf_column = inf_column or bool(np.any(np.all((cols == PINF) | (cols == NINF), axis=1)))
    return np.array(nonfinite), np.array(has_nan), np.array(has_inf), inf_column


# ---- the multiply cases of part A: (switches, case, data type, expected kernel-name prefix, lab build, options) ---------------------------------------------
def _uniform_cube(k, nb=(20, 18, 22), tails=(3, 2, 1)):
    """blocks of k x k x k with a tail block of another size in every dimension"""
    return (k * nb[0] + tails[0], k * nb[1] + tails[1], k * nb[2] + tails[2], 0.6, 0.6, 0.7, [1, k], [1, k], [1, k])


def _uniform_inner(k, s=13, nb=(20, 18, 22), tails=(3, 2, 1)):
    """blocks of s x s x k (C blocks above the one-tile kernel's 8 x 8 whatever k is), with tails"""
    return (s * nb[0] + tails[0], s * nb[1] + tails[1], k * nb[2] + tails[2], 0.6, 0.6, 0.7, [1, s], [1, s], [1, k])


def multiply_entries():
    """every kernel family tests/test_gpu_far_offsets.py reaches, on each family's smallest case, + the class kernels on every forced case, + the inner
    extents with K % 4 in {1, 2, 3} (fp32: odd K), + transposes, beta == 0, retain_sparsity and an in-place second product.  The entries on CONFIG3_37
    and SPARSE (the largest cases) are not taken over: their kernels run here on other cases, and the two switch combinations only they carried --
    the product-driven symbolic phase with the class kernels, and all classes through the run-time compiled kernels (MID=0, with the 32 x 32
    class) -- run on CONFIG3."""
    from tests import test_gpu_far_offsets as FO
    from tests import test_gpu_kernel_variants as KV
    out = []
    for env, case, dtype, expect, lab in FO.ENTRIES:
        if case in (KV.CONFIG3_37, KV.SPARSE):
            continue
        # (complex data: scalars without a zero component, see oracle_multiply)
        out.append((dict(env), case, dtype, expect, lab, dict(alpha=ALPHA + 0.2j, beta=BETA - 0.4j) if np.dtype(dtype).kind == "c" else {}))
    cls = {"DBCSR_AMD_MM_CLASSES": "2"}
    for case in (KV.H2O, KV.CONFIG3, KV.POW2):
        out.append((dict(cls), case, F64, "mm_numeric_f64_class[", False, {}))
    out.append(({"DBCSR_AMD_MM_SYMBOLIC": "rows", "DBCSR_AMD_MM_CLASSES": "2"}, KV.CONFIG3, F64, "mm_numeric_f64_class[", False, {}))
    out.append(({"DBCSR_AMD_MM_CLASSES": "2", "DBCSR_AMD_MM_MID": "0"}, KV.CONFIG3, F64, "mm_numeric_f64_class[", False, {}))
    out.append(({}, KV.CONFIG3, F64, "mm_numeric_f64", False, {}))
    out.append(({}, KV.POW2, F64, "mm_numeric_f64", False, {}))
    out.append(({}, KV.TINY_K, F64, "mm_numeric_f64_tiny", False, {}))
    # inner extents: the exact-size kernel and the class kernels, K % 4 = 1, 2, 3 (23: the kernel of the headline case); fp32: the odd-k tail
    for k in (5, 6, 7, 13, 23):
        cube = _uniform_cube(k)
        if k >= 9:   # (cubes below 9 have the one-tile kernel by default: test_gpu_class_mode.py)
            out.append(({}, cube, F64, "mm_numeric_f64_hot<%d,%d,%d>" % (k, k, k), False, {}))
        else:
            out.append(({"DBCSR_AMD_MM_SMALL": "0"}, cube, F64, "mm_numeric_f64_", False, {}))
        # (a cube below 9 has the one-tile kernel even with the classes forced: the class kernels get 13 x 13 x k there)
        out.append((dict(cls), cube if k >= 9 else _uniform_inner(k), F64, "mm_numeric_f64_class[", False, {}))
    # the exact-size kernel with K % 4 == 2 (13 and 23: K % 4 == 1 and 3).  That kernel is unchanged: the class comparison inside the columns its tail
    # k step spoils is an expected failure by the tail rule (tests/test_gpu_special_values.py: TAIL_RULE)
    for k in (10, 14, 30):
        out.append(({}, _uniform_cube(k), F64, "mm_numeric_f64_hot<%d,%d,%d>" % (k, k, k), False, {}))
    for k in (7, 23):
        out.append(({}, _uniform_cube(k), F32, "mm_numeric_f32", False, {}))
    # transposes, beta == 0 over a C full of NaN, retain_sparsity, the in-place second product
    out.append(({}, KV.H2O, F64, "mm_numeric_f64_hot<23,23,23>", False, dict(ta="T", tb="T")))
    out.append(({}, KV.MIXED, F64, "mm_numeric_f64", False, dict(ta="N", tb="T")))
    out.append(({}, KV.H2O, F64, "mm_numeric_f64_hot<23,23,23>", False, dict(beta=0.0)))
    out.append(({}, KV.MIXED, F64, "mm_numeric_f64", False, dict(beta=0.0)))
    out.append(({}, KV.H2O, F64, "mm_numeric_f64_hot<23,23,23>", False, dict(retain=True)))
    out.append(({}, KV.H2O, F64, "mm_numeric_f64_hot<23,23,23>", False, dict(alpha=1.0, beta=1.0, retain=True, twice=True)))
    out.append((dict(cls), KV.MIXED, F64, "mm_numeric_f64_class[", False, dict(alpha=1.0, beta=1.0, retain=True, twice=True)))
    return out


ENTRIES = None


def entries():
    global ENTRIES
    if ENTRIES is None:
        ENTRIES = multiply_entries()
    return ENTRIES


def entry_id(i):
    env, case, dtype, expect, lab, opt = entries()[i]
    sw = "-".join("%s=%s" % (k[13:], v) for k, v in sorted(env.items())) or "default"
    op = "-".join("%s=%s" % kv for kv in sorted(opt.items()))
    return "%02d-%s-%s%s" % (i, np.dtype(dtype).name, sw, "-" + op if op else "")


def rounds_of(case):
    """seeding rounds: one per 150 C blocks the case can have (a case with thousands of blocks gets more seeds, so that at least 5 % of them are reached)"""
    M, N, K, sa, sb, sc, bm, bn, bk = case
    nbr, nbc = len(O.make_block_sizes(M, bm)), len(O.make_block_sizes(N, bn))
    return max(1, int(round(nbr * nbc / 400.0)))


@functools.lru_cache(maxsize=None)
def clean_operands(i):
    """(A, B, C_in) of entry i on the host, in its data type and storage form: computed once, never written"""
    env, case, dtype, expect, lab, opt = entries()[i]
    A, B, Cm = O.perf_case(*case, transa=opt.get("ta", "N"), transb=opt.get("tb", "N"))
    return typed(A, dtype, 1), typed(B, dtype, 2), typed(Cm, dtype, 3)


@functools.lru_cache(maxsize=None)
def seeded_operands(i):
    env, case, dtype, expect, lab, opt = entries()[i]
    A, B, Cm = clean_operands(i)
    beta = opt.get("beta", BETA)
    if beta == 0:   # the old C is full of NaN: none of it may come out
        Cm = bcsr(Cm, np.full(Cm.data.size, np.nan, Cm.data.dtype))
    return seed(A, B, Cm, np.random.default_rng(1000 + i), beta=beta, transa=opt.get("ta", "N"), transb=opt.get("tb", "N"), rounds=rounds_of(case),
                retain=opt.get("retain", False))


@functools.lru_cache(maxsize=None)
def seeded_reference(i):
    """(the oracle's product of the seeded operands, its info; with twice: also the second product accumulated into the first)"""
    env, case, dtype, expect, lab, opt = entries()[i]
    A, B, Cm, _ = seeded_operands(i)
    alpha, beta = opt.get("alpha", ALPHA), opt.get("beta", BETA)
    ta, tb = opt.get("ta", "N"), opt.get("tb", "N")
    ref, info = oracle_multiply(ta, tb, alpha, A, B, beta, Cm, retain_sparsity=opt.get("retain", False))
    ref2 = None
    if opt.get("twice"):
        ref2, _ = oracle_multiply(ta, tb, alpha, A, B, 1.0, ref, retain_sparsity=True)
    return ref, info, ref2


@functools.lru_cache(maxsize=None)
def clean_reference(i):
    env, case, dtype, expect, lab, opt = entries()[i]
    A, B, Cm = clean_operands(i)
    return oracle_multiply(opt.get("ta", "N"), opt.get("tb", "N"), opt.get("alpha", ALPHA), A, B, opt.get("beta", BETA), Cm, retain_sparsity=opt.get("retain", False))


# ---- part C: power-of-two scaling ------------------------------------------------------------------------------------------------------------------------
PAIRS = {np.dtype(F64): [(300, -300), (-300, 300), (400, 300), (-400, -300)], np.dtype(Z64): [(300, -300), (-300, 300), (400, 300), (-400, -300)],
         np.dtype(F32): [(60, -60), (30, 20), (-30, -20)]}


def scaled(M, p):
    """M * 2^p: the same mantissas"""
    if M.data.dtype.kind == "c":
        return bcsr(M, _complex(np.ldexp(M.data.real, p), np.ldexp(M.data.imag, p), M.data.dtype))
    return bcsr(M, np.ldexp(M.data, p).astype(M.data.dtype))


def ldexp(x, p):
    if x.dtype.kind == "c":
        return _complex(np.ldexp(x.real, p), np.ldexp(x.imag, p), x.dtype)
    return np.ldexp(x, p).astype(x.dtype)


def scaling_entries():
    """the entries of part A with plain options (N / N, the common alpha and beta), each with one (p, q) of its data type: the pairs rotate per kernel
    family (the name up to its first bracket), so that every pair meets every family that has at least as many entries as there are pairs"""
    out, turn = [], {}
    for i, (env, case, dtype, expect, lab, opt) in enumerate(entries()):
        if set(opt) - {"alpha", "beta"} or opt.get("beta", BETA) == 0:
            continue
        family = (np.dtype(dtype).name, expect.split("<")[0].split("[")[0])
        pairs = PAIRS[np.dtype(dtype)]
        t = turn.get(family, len(turn))   # (a family with one entry: the pair by the family's number, so that all pairs occur among them)
        turn[family] = t + 1
        out.append((i, pairs[t % len(pairs)]))
    return out


def same_bits(x, y):
    return x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


# ---- part B: the filter cases (tests/test_gpu_filter_in_place.py: spread() inputs, eps at the median of the clean product's block norms) --------------------
def filter_cases():
    from tests import test_gpu_filter_in_place as FIP
    return list(FIP.CASES)


@functools.lru_cache(maxsize=None)
def filter_operands(case):
    """(clean A, B, C_in), (seeded A, B, C_in, placed), eps"""
    from tests import test_gpu_filter_in_place as FIP
    clean = FIP.inputs(case)
    eps = FIP.quantile_eps(case, 0.5)
    k = filter_cases().index(case)
    return clean, seed(*clean, np.random.default_rng(2000 + k), beta=1.0, rounds=rounds_of(FIP.CASES[case])), eps


@functools.lru_cache(maxsize=None)
def filter_reference(case):
    """the oracle's filtered product of the seeded operands, its info, and its unfiltered product"""
    _, (A, B, Cm, _), eps = filter_operands(case)
    ref, info = O.multiply("N", "N", 1.0, A, B, 1.0, Cm, filter_eps=eps)
    full, _ = O.multiply("N", "N", 1.0, A, B, 1.0, Cm)
    return ref, info, full


def block_sq_norms(M):
    """sum of squares of the moduli per block, float64"""
    sq = np.abs(np.asarray(M.data).astype(np.complex128 if M.data.dtype.kind == "c" else np.float64)) ** 2
    return np.array([sq[p:p + n].sum() for p, n in zip(M.blk_p, block_sizes(M))])


def coordinates(M):
    return set(zip(M.rows().tolist(), M.col_i.tolist()))
