"""The submatrix method on the device: a dense function of a large sparse matrix, one small dense principal submatrix at a time.

    dbcsr_submatrix_plan(matrix, groups)                        the index sets: which block rows each block column (or group of them) touches
    dbcsr_submatrix_gather(matrix, plan, subs, n, pad_diag, out)   a batch (nslot, n, n) of the dense principal submatrices A[S_g, S_g]
    dbcsr_submatrix_scatter(dense, matrix, plan, subs)          the block columns each submatrix owns <- the columns of its window, on the matrix' pattern
    dbcsr_submatrix_apply(matrix, fn, plan, out, pad_diag, max_waste)   gather -> fn(batch) -> scatter, bucket by bucket

Not a mirror of a routine of the reference (the method of Lass, Mohr, Wiebeler, Kuehne and Plessl; in CP2K the submatrix sign method of dm_ls_scf).  For
every block column j -- or every group of block columns -- the block rows S that the column(s) touch are taken, the dense principal submatrix A[S, S] is
assembled from the blocks the matrix stores (zeros elsewhere), a dense function is applied to the batch of these small matrices, and the columns that
belong to j are copied out of each result into block column j of the result, on the pattern of A.  The index sets are built here with torch operations
(the plumbing, which also runs on host tensors); the two copies are HIP kernels behind the C-ABI entries dbcsr_amd_bcsr_submatrix_gather / _scatter
(include/dbcsr_amd_mm.h, "Submatrix method"; kernels of dbcsr_amd/csrc/mm_submatrix.h); the dense function is the caller's, torch.linalg on the batch.
float64, float32 and complex128 data; one rank / one device."""
import ctypes as C
import math

import numpy as np
import torch

from .matrix import DbcsrMatrix, StreamHandle
from .multiply import default_engine
from .operations import _check_symmetry, _data_overlap, _same_blk_sizes

__all__ = ["SubmatrixPlan", "dbcsr_submatrix_plan", "dbcsr_submatrix_gather", "dbcsr_submatrix_scatter", "dbcsr_submatrix_apply"]


class SubmatrixPlan:
    """The index sets of the submatrix method for one block structure and pattern (dbcsr_submatrix_plan makes it).  Device tensors, int32: set_ptr
    [nsub + 1]; set_idx [nmem], the member block rows, ascending inside a set; set_off [nmem], the element offset of each member inside its submatrix;
    sub_dim [nsub], the side of each submatrix; owner [nblkcols], the submatrix of each block column, -1 for none.  Host integers: nsub, nmem,
    max_members, max_dim.  It keeps the matrix' index_stamp() and its block-size tensors: gather and scatter refuse a matrix with another block
    structure.  The sides and member counts are also held on the host (sub_dim_host, members_host: what buckets() works on), fetched in the one
    synchronisation of the constructor."""

    def __init__(self, matrix, owner, set_ptr, set_idx, set_off, sub_dim, nmem, max_members, max_dim, sub_dim_host, members_host):
        self.row_blk_size, self.col_blk_size = matrix.row_blk_size, matrix.col_blk_size
        self.nblkcols = matrix.nblkcols
        self.stamp = matrix.index_stamp()
        self.symmetry = getattr(matrix, "symmetry", "N")
        self.owner, self.set_ptr, self.set_idx, self.set_off, self.sub_dim = owner, set_ptr, set_idx, set_off, sub_dim
        self.nsub, self.nmem, self.max_members, self.max_dim = int(sub_dim_host.size), int(nmem), int(max_members), int(max_dim)
        self.sub_dim_host, self.members_host = sub_dim_host, members_host
        self._all_slots = None

    @property
    def device(self):
        return self.owner.device

    def all_slots(self):
        """sub_slot of a batch that holds every submatrix in its order: 0 ... nsub - 1"""
        if self._all_slots is None:
            self._all_slots = torch.arange(self.nsub, dtype=torch.int32, device=self.device)
        return self._all_slots

    def buckets(self, max_waste=0.5):
        """Lists of submatrix ids grouped by side, every submatrix in exactly one: a batch of a bucket is padded to the bucket's largest side n, and the
        share of its count * n^2 elements that is padding is at most max_waste (0: only equal sides share a bucket).  The buckets come with descending
        side, the ids inside one ascend.  A plain host helper on sub_dim_host."""
        max_waste = float(max_waste)
        if not 0.0 <= max_waste <= 1.0:
            raise ValueError("SubmatrixPlan.buckets: max_waste must be in [0, 1], got %r" % max_waste)
        dims = self.sub_dim_host
        out, cur, filled, side = [], [], 0, 0
        for g in sorted(range(self.nsub), key=lambda g: (-int(dims[g]), g)):
            d = int(dims[g])
            total = (len(cur) + 1) * side * side
            if cur and total - (filled + d * d) <= max_waste * total:
                cur.append(g)
                filled += d * d
                continue
            if cur:
                out.append(sorted(cur))
            cur, filled, side = [g], d * d, d
        if cur:
            out.append(sorted(cur))
        return out


def _groups(name, groups, nb, device):
    if groups is None:
        return torch.arange(nb, dtype=torch.int64, device=device)
    t = groups if isinstance(groups, torch.Tensor) else torch.as_tensor(np.asarray(groups))
    if t.dim() != 1 or t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
        raise TypeError("%s: groups must be a 1-D sequence of integers" % name)
    if t.numel() != nb:
        raise ValueError("%s: groups has %d entries, the matrix has %d block columns" % (name, t.numel(), nb))
    return t.to(device=device, dtype=torch.int64)


def dbcsr_submatrix_plan(matrix, groups=None):
    """The index sets of the submatrix method.  The matrix is square in its block structure with row block sizes equal to its column block sizes; any
    symmetry ('N' 'S' 'A' 'H' 'K').  groups=None: one submatrix per block column.  Otherwise a sequence or tensor of nblkcols integers: group[j] = g >= 0
    puts block column j into submatrix g -- the ids are 0 ... nsub - 1 with none unused (ValueError) -- and -1 leaves block column j out of every
    submatrix.  The set of submatrix g is the union over its block columns j of {j} and {i : (i, j) stored}; of a stored triangle also {i : (j, i)
    stored}, the column pattern of the desymmetrized matrix.  j itself is always a member, whether the diagonal block is stored or not.  Members ascend.
    Everything is built with torch operations on the device of the index arrays (host tensors serve as well), at the full length the pattern allows, so
    that one transfer at the end -- the one synchronisation -- brings the counts, the sides and the verdict on the arguments.  Zero-size blocks and a
    matrix without block columns are legal."""
    name = "dbcsr_submatrix_plan"
    sym = _check_symmetry(name, matrix)
    matrix.dtype_code
    if sym != "N":
        matrix.symmetry_kind()
    nb = matrix.nblkcols
    if matrix.nblkrows != nb:
        raise ValueError("%s: the matrix is not square in its block structure (%d x %d blocks)" % (name, matrix.nblkrows, nb))
    dev = matrix.row_p.device
    own = _groups(name, groups, nb, dev)
    i32 = lambda t: t.to(torch.int32).contiguous()
    if nb == 0:
        z = torch.zeros(0, dtype=torch.int32, device=dev)
        return SubmatrixPlan(matrix, z, torch.zeros(1, dtype=torch.int32, device=dev), z, z, z, 0, 0, 0, np.zeros(0, np.int64), np.zeros(0, np.int64))
    bs = matrix.row_blk_size.to(torch.int64)
    same_sizes = torch.ones((), dtype=torch.bool, device=dev) if matrix.col_blk_size is matrix.row_blk_size else \
        (matrix.col_blk_size.to(torch.int64) == bs).all()
    every = torch.arange(nb, dtype=torch.int64, device=dev)
    nblks = matrix.nblks
    rows = torch.searchsorted(matrix.row_p[1:].to(torch.int64).contiguous(), torch.arange(nblks, dtype=torch.int64, device=dev), right=True)
    cols = matrix.col_i.to(torch.int64)
    mem, col = [every, rows], [every, cols]   # (member, the block column that brings it in)
    if sym != "N":
        mem.append(cols)
        col.append(rows)
    mem, col = torch.cat(mem), torch.cat(col)
    # the arguments' verdict: ids in -1 ... nb - 1 (a submatrix has at least one block column), none unused below the largest
    in_range = ((own >= -1) & (own < nb)).all()
    present = torch.zeros(nb + 1, dtype=torch.int64, device=dev).scatter_(0, own.clamp(-1, nb - 1) + 1, torch.ones_like(own))
    nsub_t = (own.max() + 1).clamp(0, nb)
    ok = in_range & ((present[1:] > 0).sum() == nsub_t) & same_sizes
    # one key per (submatrix, member), sorted; the pairs of block columns without a submatrix sort behind all of them
    big = nb * nb
    g = own[col]
    key = torch.where((g >= 0) & (g < nb), g * nb + mem, torch.full_like(g, big))
    key, _ = torch.sort(key)
    K = int(key.numel())
    first = torch.ones(K, dtype=torch.bool, device=dev)
    first[1:] = key[1:] != key[:-1]
    first &= key < big
    pos = torch.cumsum(first.to(torch.int64), 0) - 1
    nmem_t = pos[-1] + 1
    skey = torch.full((K + 1,), big, dtype=torch.int64, device=dev)
    skey.scatter_(0, torch.where(first, pos, torch.full_like(pos, K)), key)   # (repeats and the unowned go to entry K, which is reset)
    skey[K] = big
    set_g, idx = torch.div(skey, nb, rounding_mode="floor"), skey % nb   # (behind the members: set_g = nb)
    sizes = torch.where(skey < big, bs[idx], torch.zeros_like(idx))
    csum = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(sizes, 0)])   # csum[p]: the sizes of the entries before p
    ptr = torch.searchsorted(set_g.contiguous(), torch.arange(nb + 1, dtype=torch.int64, device=dev))   # [nb + 1]; from nsub on: nmem
    off = csum[:-1] - csum[ptr[set_g]]
    dims = csum[ptr[1:]] - csum[ptr[:-1]]
    members = ptr[1:] - ptr[:-1]
    head = torch.stack([nsub_t, nmem_t, members.max(), dims.max(), ok.to(torch.int64)])
    host = torch.cat([head, dims, members]).cpu().numpy()   # the one synchronisation
    nsub, nmem, max_members, max_dim, fine = (int(x) for x in host[:5])
    if not fine:
        raise ValueError("%s: groups must hold -1 or the ids 0 ... nsub - 1 with none unused, and the row block sizes must be the column block sizes" % name)
    if max_dim > 2 ** 31 - 1:
        raise ValueError("%s: a submatrix of side %d" % (name, max_dim))
    return SubmatrixPlan(matrix, i32(own), i32(ptr[:nsub + 1]), i32(idx[:nmem]), i32(off[:nmem]), i32(dims[:nsub]), nmem, max_members, max_dim,
                         host[5:5 + nsub].astype(np.int64), host[5 + nb:5 + nb + nsub].astype(np.int64))


# ---- checks that come before any call of the library ------------------------------------------------------------------------------------------------------
def _check_plan(name, matrix, plan):
    if not isinstance(plan, SubmatrixPlan):
        raise TypeError("%s: plan must be a SubmatrixPlan" % name)
    sym = _check_symmetry(name, matrix)
    matrix.dtype_code
    kind = matrix.symmetry_kind() if sym != "N" else -1
    if matrix.row_p.device != plan.device:
        raise ValueError("%s: the plan is not on the matrix' device" % name)
    if matrix.nblkrows != plan.nblkcols or matrix.nblkcols != plan.nblkcols:
        raise ValueError("%s: the plan was made for %d block columns, the matrix has %d x %d blocks" % (name, plan.nblkcols, matrix.nblkrows, matrix.nblkcols))
    if matrix.index_stamp() != plan.stamp and not (_same_blk_sizes(matrix.row_blk_size, plan.row_blk_size) and
                                                  _same_blk_sizes(matrix.col_blk_size, plan.col_blk_size)):
        raise ValueError("%s: the plan was made for another block structure" % name)
    return kind


def _check_subs(name, plan, subs):
    """the submatrices of the slots as a list, None for all of them in their order"""
    if subs is None:
        return None
    ids = subs.tolist() if isinstance(subs, (torch.Tensor, np.ndarray)) else list(subs)
    if any(isinstance(g, (float, complex, bool)) or int(g) != g for g in ids):
        raise TypeError("%s: subs must be integers" % name)
    ids = [int(g) for g in ids]
    if any(g < 0 or g >= plan.nsub for g in ids):
        raise ValueError("%s: subs outside 0 ... %d" % (name, plan.nsub - 1))
    if len(set(ids)) != len(ids):
        raise ValueError("%s: subs names a submatrix twice" % name)
    return ids


def _largest(values, ids):
    if ids is None:
        return int(values.max()) if values.size else 0
    return max((int(values[g]) for g in ids), default=0)


def _check_batch(name, matrix, t, nslot, n, what):
    """a 3-D tensor (nslot, n, n) of the matrix' data type on its device with strides (batch_stride, ld, 1), ld >= n, batch_stride >= n ld, that does not
    overlap the matrix' data area.  Returns (ld, batch_stride)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s: %s must be a torch tensor" % (name, what))
    if t.dtype != matrix.dtype:
        raise TypeError("%s: %s has data type %r, expected %r" % (name, what, t.dtype, matrix.dtype))
    if t.device != matrix.row_p.device:
        raise ValueError("%s: %s is not on the matrix' device" % (name, what))
    if t.dim() != 3 or tuple(t.shape) != (nslot, n, n):
        raise ValueError("%s: %s must be a 3-D tensor of shape (%d, %d, %d), got %r" % (name, what, nslot, n, n, tuple(t.shape)))
    s0, s1, s2 = t.stride()
    if n > 1 and s2 != 1:
        raise ValueError("%s: %s must have stride(2) == 1 (row by row), got strides %r" % (name, what, (s0, s1, s2)))
    ld = s1 if n > 1 else max(n, 1)   # (the stride of a dimension of one element, or of none, says nothing)
    if ld < n:
        raise ValueError("%s: %s has strides %r: the stride between its rows is below the %d elements of one" % (name, what, (s0, s1, s2), n))
    batch_stride = s0 if nslot > 1 else n * ld
    if batch_stride < n * ld:
        raise ValueError("%s: %s has strides %r: the stride between its windows is below the %d elements of one" % (name, what, (s0, s1, s2), n * ld))
    data = matrix.data
    if nslot and n and data.numel():
        e = t.element_size()
        a0, a1 = t.data_ptr(), t.data_ptr() + ((nslot - 1) * batch_stride + (n - 1) * ld + n) * e
        b0, b1 = data.data_ptr(), data.data_ptr() + data.numel() * data.element_size()
        if a0 < b1 and b0 < a1:
            raise ValueError("%s: %s overlaps the matrix' data area" % (name, what))
    return ld, batch_stride


def _on(stream):
    return torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream())


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


# ---- the two copies -------------------------------------------------------------------------------------------------------------------------------------------
def dbcsr_submatrix_gather(matrix, plan, subs=None, n=None, pad_diag=0.0, out=None, engine=None, stream=None):
    """A batch (nslot, n, n) of dense principal submatrices of the matrix: slot t holds submatrix subs[t] (subs=None: all of them, in their order).  The
    window of submatrix g receives every tile of S_g x S_g that the matrix stores, bit for bit; of a stored triangle also the twin of the block stored at
    the mirrored place (dbcsr_to_dense's reading: sign flips, exact; a diagonal block as stored); +0.0 everywhere else inside its side n_g.  Between n_g
    and n the window is +0.0 with pad_diag on the diagonal: blockdiag(A[S, S], pad_diag I), on whose two parts a matrix function acts separately --
    pad_diag=1 keeps an inverse or a sign well defined, pad_diag=0 is plain zero padding.  n: at least the largest side among the submatrices of the
    batch (ValueError otherwise); the default is plan.max_dim.  out=None allocates a contiguous tensor on the matrix' device and stream; otherwise out
    has shape (nslot, n, n), the matrix' data type and strides (batch_stride, ld, 1) with ld >= n and batch_stride >= n ld, and does not overlap
    matrix.data.  Every element of every window is written exactly once per call; nothing outside a window is written.  The matrix may have another
    pattern than the one the plan was made from (the sets are index sets), not another block structure.  It is only read: index_stamp() stays, no saved
    plan is touched.  Asynchronous on the stream, no synchronisation; the same bits on every call; every refusal comes before any call of the library.
    Returns out."""
    name = "dbcsr_submatrix_gather"
    kind = _check_plan(name, matrix, plan)
    ids = _check_subs(name, plan, subs)
    nslot = plan.nsub if ids is None else len(ids)
    need = _largest(plan.sub_dim_host, ids)
    if n is None:
        n = plan.max_dim
    if isinstance(n, bool) or int(n) != n or n < 0:
        raise ValueError("%s: n must be a non-negative integer, got %r" % (name, n))
    n = int(n)
    if n < need:
        raise ValueError("%s: n = %d is below the side %d of a submatrix of the batch" % (name, n, need))
    pad_diag = float(pad_diag)
    if not math.isfinite(pad_diag):
        raise ValueError("%s: pad_diag must be finite, got %r" % (name, pad_diag))
    ld, batch_stride = max(n, 1), n * max(n, 1)
    if out is not None:
        ld, batch_stride = _check_batch(name, matrix, out, nslot, n, "out")
    E = engine or default_engine()
    lib, handle = E.L, E.h
    st = StreamHandle(stream)
    with _on(stream):
        if out is None:
            out = torch.empty((nslot, n, n), dtype=matrix.dtype, device=matrix.row_p.device)
        slot_sub = None if ids is None else torch.tensor(ids, dtype=torch.int32).to(plan.device, non_blocking=True)
    d = matrix.desc()
    rc = lib.dbcsr_amd_bcsr_submatrix_gather(handle, matrix.dtype_code, C.byref(d), kind, plan.nsub, _ptr(plan.set_ptr), _ptr(plan.set_idx),
                                             _ptr(plan.set_off), _ptr(plan.sub_dim), nslot, _ptr(slot_sub), _largest(plan.members_host, ids),
                                             out.data_ptr() if nslot and n else None, n, ld, batch_stride, pad_diag, st.ptr)
    if rc != 0:
        raise RuntimeError("dbcsr_amd_bcsr_submatrix_gather failed (%d)" % rc)
    return out


def dbcsr_submatrix_scatter(dense, matrix, plan, subs=None, engine=None, stream=None):
    """The way back: every block (R, C) the matrix stores whose block column C is owned by a submatrix g of the batch and whose block row R is a member of
    S_g <- the elements of g's window at (set_off[R], set_off[C]), bit for bit -- the columns that belong to C out of the result of its own submatrix.
    dense: (nslot, n, n) in dbcsr_submatrix_gather's layout, slot t holding submatrix subs[t] (subs=None: all, in their order).  Everything else keeps its
    bits: blocks of block columns without an owner or whose submatrix is not in the batch, blocks whose row is no member, the holes of an unpacked
    matrix.  The pattern never changes: no index array is written, index_stamp() stays, a multiply with the matrix as operand afterwards reuses its plan;
    block norms a multiply announced are forgotten.  No symmetry is applied: of a stored triangle the blocks stored are taken from where they lie.  dense
    must not overlap matrix.data (ValueError).  Asynchronous on the stream, no synchronisation; every refusal comes before any call of the library.
    Returns matrix."""
    name = "dbcsr_submatrix_scatter"
    _check_plan(name, matrix, plan)
    ids = _check_subs(name, plan, subs)
    nslot = plan.nsub if ids is None else len(ids)
    if not isinstance(dense, torch.Tensor):
        raise TypeError("%s: dense must be a torch tensor" % name)
    n = int(dense.shape[1]) if dense.dim() == 3 else -1
    ld, batch_stride = _check_batch(name, matrix, dense, nslot, max(n, 0), "dense")
    need = _largest(plan.sub_dim_host, ids)
    if n < need:
        raise ValueError("%s: dense has windows of side %d, a submatrix of the batch has side %d" % (name, n, need))
    E = engine or default_engine()
    lib, handle = E.L, E.h
    st = StreamHandle(stream)
    if ids is None:
        sub_slot = plan.all_slots()
    else:
        slots = np.full(plan.nsub, -1, np.int32)
        slots[ids] = np.arange(len(ids), dtype=np.int32)
        with _on(stream):
            sub_slot = torch.from_numpy(slots).to(plan.device, non_blocking=True)
    d = matrix.desc()   # (only the data area is written)
    rc = lib.dbcsr_amd_bcsr_submatrix_scatter(handle, matrix.dtype_code, dense.data_ptr() if nslot and n else None, n, ld, batch_stride, plan.nsub,
                                              _ptr(plan.set_ptr), _ptr(plan.set_idx), _ptr(plan.set_off), _ptr(plan.owner), _ptr(sub_slot), C.byref(d),
                                              st.ptr)
    if rc != 0:
        raise RuntimeError("dbcsr_amd_bcsr_submatrix_scatter failed (%d)" % rc)
    return matrix


def dbcsr_submatrix_apply(matrix, fn, plan=None, out=None, pad_diag=1.0, max_waste=0.5, engine=None, stream=None):
    """f(A) by the submatrix method, on the pattern of A: for every bucket of plan.buckets(max_waste) -- submatrices of about one side, padded to the
    largest -- the batch is gathered (with pad_diag on the padding's diagonal), fn(batch) is applied -- any function of a (count, n, n) tensor that returns
    one of the same shape, data type and device: torch.linalg.inv, a Newton-Schulz sign, an eigh-based purification -- and the block columns each
    submatrix owns are scattered into out.  plan=None builds the default plan (one submatrix per block column).  out=None: a new matrix on A's pattern
    (A's index arrays, a copy of its data area), so that blocks no submatrix reaches keep A's values; otherwise a matrix of A's block structure whose
    data area does not overlap A's (a submatrix is gathered after others were scattered).  fn runs on the stream's torch context.  Returns out."""
    name = "dbcsr_submatrix_apply"
    if not callable(fn):
        raise TypeError("%s: fn must be callable" % name)
    if plan is None:
        plan = dbcsr_submatrix_plan(matrix)
    _check_plan(name, matrix, plan)
    pad_diag = float(pad_diag)
    if not math.isfinite(pad_diag):
        raise ValueError("%s: pad_diag must be finite, got %r" % (name, pad_diag))
    buckets = plan.buckets(max_waste)
    if out is not None:
        _check_plan(name, out, plan)
        if out.dtype != matrix.dtype:
            raise TypeError("%s: data types of the matrix and of out differ" % name)
        if out is matrix or _data_overlap(out.data, matrix.data):
            raise ValueError("%s: out.data overlaps matrix.data" % name)
    E = engine or default_engine()
    with _on(stream):
        if out is None:
            out = DbcsrMatrix(matrix.row_blk_size, matrix.col_blk_size, matrix.row_p, matrix.col_i, matrix.blk_p, matrix.data.clone(), matrix.name,
                              getattr(matrix, "symmetry", "N"), nze=matrix._nze)
        for ids in buckets:
            n = _largest(plan.sub_dim_host, ids)
            if n == 0:
                continue
            batch = dbcsr_submatrix_gather(matrix, plan, subs=ids, n=n, pad_diag=pad_diag, engine=E, stream=stream)
            res = fn(batch)
            if not isinstance(res, torch.Tensor) or res.shape != batch.shape or res.dtype != batch.dtype or res.device != batch.device:
                raise TypeError("%s: fn must return a tensor of the batch's shape, data type and device" % name)
            dbcsr_submatrix_scatter(res.contiguous(), out, plan, subs=ids, engine=E, stream=stream)
    return out
