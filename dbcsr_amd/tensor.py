"""Block-sparse tensors on the device -- the second public interface of the reference (src/tensors, dbcsr_t_*), on one device, for ranks 2, 3 and 4,
float64, float32 and complex128 data, without symmetry:

    dbcsr_t_create(blk_sizes, map1, map2, dtype, device, name)  an empty tensor
    dbcsr_t_create_from_blocks(blk_sizes, map1, map2, idx, data, offsets, summation)   a tensor from a list of blocks
    dbcsr_t_block_indices(tensor)                               (nblk, rank) int32: the stored blocks, in the matrix' index order
    dbcsr_t_put_blocks(tensor, idx, data, offsets, summation)   blocks into the tensor (the rules of dbcsr_put_blocks)
    dbcsr_t_get_blocks(tensor, idx, out, offsets)               (data, found): blocks out of the tensor (the rules of dbcsr_get_blocks)
    dbcsr_t_copy(tensor_in, tensor_out, order, summation)       tensor_out <- [tensor_out +] tensor_in with its dimensions permuted, any two mappings
    dbcsr_t_copy_matrix_to_tensor(matrix, tensor) / dbcsr_t_copy_tensor_to_matrix(tensor, matrix)   rank 2
    dbcsr_t_filter(tensor, eps)                                 the block filter on the tensor's matrix
    dbcsr_t_contract(alpha, tensor_1, tensor_2, beta, tensor_3, contract_1, notcontract_1, contract_2, notcontract_2, map_1, map_2, ...)
                                                                T3 <- beta*T3 + alpha * sum over the contracted dimensions of T1*T2; returns the flop count

The layout (the reference's sources could not be consulted, the semantics are those of dense numpy arrays).  A tensor of rank r has block
sizes per dimension.  A mapping (map1 | map2) -- two ordered, disjoint, non-empty tuples that together hold 0 ... r-1 -- folds it into a DbcsrMatrix
without symmetry: block (i_0 ... i_{r-1}) lies in block row R = i_{map1[0]} + nb_{map1[0]} (i_{map1[1]} + ...), the first entry of map1 running
fastest, and in the block column formed the same way from map2; the row and column block sizes are the products of the sizes; inside a block an element
has its row and column formed the same way from its place and the block's extents.  With column-major blocks a stored block is therefore the Fortran
array of the tensor block with its dimensions in the order map1 ++ map2, the STORED ORDER.  Across this interface blocks travel in CANONICAL order:
dimensions 0, 1, ..., r-1 with dimension 0 fastest.

Everything the library does to matrices applies to tensor.matrix as it is (scale, add on the same mapping, norms, filter, ...).  Changing a mapping
is index work on nblks integers, done here with torch operations on the device (they run on host tensors as well: the tests without a GPU use
that), and ONE launch of the HIP kernel behind dbcsr_amd_tensor_permute_blocks (include/dbcsr_amd_mm.h, "Tensors"; dbcsr_amd/csrc/mm_tensor.h) that
permutes the inside of every block straight into its place of the new data area.  A contraction is re-folding where needed, then dbcsr_multiply,
then re-folding back.  stats() counts the permute launches, so a caller can see what moved.

Not yet: bounds of a contraction, the TAS split, process grids and distributions, dbcsr_t_split_blocks, the batched contraction, the Fortran and C
tensor API, complex_4, and plan reuse across contractions that remap (a remapped operand has new index tensors)."""
import ctypes as C

import numpy as np
import torch

from .matrix import DbcsrMatrix, StreamHandle, _dtype_code
from .multiply import dbcsr_multiply, default_engine
from .operations import _check_flat, _check_offsets, _data_overlap, dbcsr_add, dbcsr_get_blocks, dbcsr_put_blocks, dbcsr_reserve_blocks
from .operations import _on_stream as _on_cuda_stream

__all__ = ["DbcsrTensor", "dbcsr_t_create", "dbcsr_t_create_from_blocks", "dbcsr_t_block_indices", "dbcsr_t_put_blocks", "dbcsr_t_get_blocks",
           "dbcsr_t_copy", "dbcsr_t_copy_matrix_to_tensor", "dbcsr_t_copy_tensor_to_matrix", "dbcsr_t_filter", "dbcsr_t_contract"]

_INT32_MAX = 2 ** 31 - 1
_STATS = {"permute_launches": 0, "permuted_elements": 0}


class _null:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def _on_stream(stream, device=None):
    """the torch stream context of the index work; nothing for host tensors (the tests without a GPU)"""
    if device is not None and torch.device(device).type != "cuda":
        return _null()
    return _on_cuda_stream(stream)


def stats():
    """{'permute_launches': launches of the permute kernel so far, 'permuted_elements': the elements they were handed}"""
    return dict(_STATS)


def reset_stats():
    _STATS["permute_launches"] = _STATS["permuted_elements"] = 0


# ---- the mapping, on the host ----------------------------------------------------------------------------------------------------------------------------
def check_mapping(name, rank, map1, map2):
    """(map1, map2) as tuples of ints; ValueError unless they are ordered, disjoint, non-empty and together hold 0 ... rank-1 of a rank 2 ... 4"""
    if rank < 2 or rank > 4:
        raise ValueError("%s: tensors of rank 2, 3 and 4, got rank %d" % (name, rank))
    m1, m2 = tuple(int(d) for d in map1), tuple(int(d) for d in map2)
    if not m1 or not m2:
        raise ValueError("%s: an empty half of the mapping (%r | %r)" % (name, m1, m2))
    if sorted(m1 + m2) != list(range(rank)):
        raise ValueError("%s: the mapping (%r | %r) does not hold every dimension 0 ... %d exactly once" % (name, m1, m2, rank - 1))
    return m1, m2


def check_limits(name, sizes_host, map1, map2):
    """ValueError unless the numbers of block rows and columns and every row and column block size fit an int32.  sizes_host: per dimension a numpy
    array of the block sizes (each >= 1)."""
    for what, dims in (("rows", map1), ("columns", map2)):
        count, largest = 1, 1
        for d in dims:
            count *= int(sizes_host[d].size)
            largest *= int(sizes_host[d].max()) if sizes_host[d].size else 1
        if count > _INT32_MAX:
            raise ValueError("%s: %d block %s do not fit an int32" % (name, count, what))
        if largest > _INT32_MAX:
            raise ValueError("%s: a block size of %d along the %s does not fit an int32" % (name, largest, what))


# ---- the index work: torch operations that run on device and host tensors alike -----------------------------------------------------------------------------
def combine_index(idx, nblks_per_dim, dims):
    """idx (n, rank) integer -> int64 (n): idx[:, dims[0]] + nb[dims[0]] * (idx[:, dims[1]] + nb[dims[1]] * ...), the first of dims fastest"""
    out = torch.zeros(idx.shape[0], dtype=torch.int64, device=idx.device)
    stride = 1
    for d in dims:
        out = out + idx[:, d].to(torch.int64) * stride
        stride *= int(nblks_per_dim[d])
    return out


def split_index(lin, nblks_per_dim, dims):
    """the inverse of combine_index: {d: int64 (n)} for d in dims"""
    out = {}
    rest = lin.to(torch.int64)
    for d in dims:
        nb = max(int(nblks_per_dim[d]), 1)
        out[d] = rest % nb
        rest = rest // nb
    return out


def fold_sizes(blk_sizes, dims):
    """int32 tensor of prod nb[d] entries: the product of the block sizes of the dimensions dims, the first of them fastest"""
    out = blk_sizes[dims[0]].to(torch.int64)
    for d in dims[1:]:
        out = (blk_sizes[d].to(torch.int64)[:, None] * out[None, :]).reshape(-1)
    return out.to(torch.int32)


def block_extents(idx, blk_sizes, dims):
    """int64 (n, len(dims)): the extents of the listed blocks along the dimensions dims, in that order"""
    return torch.stack([blk_sizes[d].to(torch.int64)[idx[:, d].to(torch.int64)] for d in dims], dim=1)


def fold_index(idx, blk_sizes, map1, map2):
    """The matrix index of the blocks idx (n, rank; distinct, in range) under the mapping (map1 | map2): (order, row_p, col_i, blk_p, nze) with order
    int64 (n) the list positions sorted by (block row, block column), row_p int32 by counts and a scan, col_i int32, blk_p int64 the running sum
    of the block sizes (packed), nze a 0-d int64 tensor (no synchronisation here)."""
    nb = [int(s.numel()) for s in blk_sizes]
    nbr, nbc = 1, 1
    for d in map1:
        nbr *= nb[d]
    for d in map2:
        nbc *= nb[d]
    dev = idx.device
    rows, cols = combine_index(idx, nb, map1), combine_index(idx, nb, map2)
    order = torch.argsort(rows * max(nbc, 1) + cols, stable=True)
    rows, cols = rows[order], cols[order]
    counts = torch.zeros(nbr, dtype=torch.int64, device=dev).scatter_add_(0, rows, torch.ones_like(rows))
    row_p = torch.zeros(nbr + 1, dtype=torch.int32, device=dev)
    row_p[1:] = torch.cumsum(counts, 0).to(torch.int32)
    size = block_extents(idx, blk_sizes, tuple(range(len(nb)))).prod(dim=1)[order]
    ends = torch.cumsum(size, 0)
    nze = ends[-1] if idx.shape[0] else torch.zeros((), dtype=torch.int64, device=dev)
    return order, row_p, cols.to(torch.int32), ends - size, nze


def unfold_index(row_p, col_i, nblks_per_dim, map1, map2):
    """(nblk, rank) int64: the tensor indices of the blocks of a matrix index under the mapping"""
    n = int(col_i.numel())
    nbr = int(row_p.numel()) - 1
    dev = col_i.device
    rows = torch.repeat_interleave(torch.arange(nbr, dtype=torch.int64, device=dev), torch.diff(row_p.to(torch.int64)), output_size=n)
    parts = split_index(rows, nblks_per_dim, map1)
    parts.update(split_index(col_i, nblks_per_dim, map2))
    return torch.stack([parts[d] for d in range(len(nblks_per_dim))], dim=1) if n else torch.zeros((0, len(nblks_per_dim)), dtype=torch.int64, device=dev)


def _padded_ext(ext):
    """(n, k) int64 extents -> (n, 4) int32 contiguous, padded with 1"""
    n, k = ext.shape
    out = torch.ones((n, 4), dtype=torch.int32, device=ext.device)
    out[:, :k] = ext.to(torch.int32)
    return out.contiguous()


# ---- the tensor ---------------------------------------------------------------------------------------------------------------------------------------------
def _host_sizes(name, blk_sizes):
    """per dimension a numpy int64 copy of the block sizes; ValueError for what is not 1-D or holds a size outside 1 ... 2^31 - 1"""
    out = []
    for d, s in enumerate(blk_sizes):
        h = s.detach().cpu().numpy().astype(np.int64) if isinstance(s, torch.Tensor) else np.asarray(list(s), dtype=np.int64)
        if h.ndim != 1:
            raise ValueError("%s: blk_sizes[%d] must be 1-D" % (name, d))
        if h.size and (h.min() < 1 or h.max() > _INT32_MAX):
            raise ValueError("%s: blk_sizes[%d] holds a block size outside 1 ... 2^31 - 1" % (name, d))
        out.append(h)
    return out


class DbcsrTensor:
    """A block-sparse tensor: blk_sizes (a tuple of int32 device tensors, one per dimension), the mapping (map1 | map2) and .matrix, the DbcsrMatrix
    without symmetry that stores it (see the module's text for the layout)."""

    def __init__(self, blk_sizes, map1, map2, matrix, name="", _host_sizes=None):
        self.blk_sizes = tuple(blk_sizes)
        self.map1, self.map2 = check_mapping("DbcsrTensor", len(self.blk_sizes), map1, map2)
        self.matrix = matrix
        self.name = name
        self._host_sizes = _host_sizes if _host_sizes is not None else [s.detach().cpu().numpy().astype(np.int64) for s in self.blk_sizes]

    @property
    def rank(self):
        return len(self.blk_sizes)

    @property
    def dtype(self):
        return self.matrix.dtype

    @property
    def nblks(self):
        return self.matrix.nblks

    @property
    def nblks_per_dim(self):
        return tuple(int(h.size) for h in self._host_sizes)

    @property
    def stored_order(self):
        return self.map1 + self.map2

    @property
    def device(self):
        return self.matrix.row_p.device


def _empty_matrix(blk_sizes, host_sizes, map1, map2, dtype, device, name):
    check_limits("dbcsr_t_create", host_sizes, map1, map2)
    return DbcsrMatrix.empty_like_pattern(fold_sizes(blk_sizes, map1), fold_sizes(blk_sizes, map2), dtype, device=device, name=name)


def dbcsr_t_create(blk_sizes, map1, map2, dtype, device="cuda", name=""):
    """An empty tensor.  blk_sizes: per dimension an int32 tensor (or a sequence of integers) of the block sizes, each >= 1.  ValueError -- before any
    device work -- for a rank outside 2 ... 4, a mapping that is not one, and a folded matrix whose numbers of block rows / columns or whose row / column
    block sizes do not fit an int32; TypeError for a data type other than float64, float32 and complex128."""
    fn = "dbcsr_t_create"
    blk_sizes = list(blk_sizes)
    m1, m2 = check_mapping(fn, len(blk_sizes), map1, map2)
    _dtype_code(dtype)
    host = _host_sizes(fn, blk_sizes)
    check_limits(fn, host, m1, m2)   # (from the host copies: nothing is allocated for a tensor that is refused)
    dev = torch.device(device)
    dev_sizes = tuple(s.to(device=dev, dtype=torch.int32).contiguous() if isinstance(s, torch.Tensor) else torch.as_tensor(h, dtype=torch.int32).to(dev)
                      for s, h in zip(blk_sizes, host))
    M = _empty_matrix(dev_sizes, host, m1, m2, dtype, dev, name)
    return DbcsrTensor(dev_sizes, m1, m2, M, name, _host_sizes=host)


def _like(tensor, map1, map2, name=""):
    """an empty tensor of the same block sizes, type and device under another mapping"""
    M = _empty_matrix(tensor.blk_sizes, tensor._host_sizes, map1, map2, tensor.dtype, tensor.device, name or tensor.name)
    return DbcsrTensor(tensor.blk_sizes, map1, map2, M, name or tensor.name, _host_sizes=tensor._host_sizes)


def dbcsr_t_block_indices(tensor, stream=None):
    """(nblk, rank) int32 on the tensor's device: the indices of the stored blocks, in the order of the matrix' index (by block row, then block column)"""
    with _on_stream(stream, tensor.device):
        return unfold_index(tensor.matrix.row_p, tensor.matrix.col_i, tensor.nblks_per_dim, tensor.map1, tensor.map2).to(torch.int32)


# ---- the permute launch ---------------------------------------------------------------------------------------------------------------------------------------
def _permute(E, stream, dtype, perm, ext, src_off, dst_off, src, dst, elements):
    """one launch of dbcsr_amd_tensor_permute_blocks: dimension j of a written block is dimension perm[j] of the read one"""
    n = int(ext.shape[0])
    if n == 0 or src.numel() == 0 or dst.numel() == 0:
        return
    st = StreamHandle(stream)
    rank = len(perm)
    p = (C.c_int * rank)(*[int(x) for x in perm])
    rc = E.L.dbcsr_amd_tensor_permute_blocks(E.h, _dtype_code(dtype), n, rank, p, ext.data_ptr(), src_off.data_ptr(), dst_off.data_ptr(), src.data_ptr(),
                                             int(src.numel()), dst.data_ptr(), int(dst.numel()), st.ptr)
    if rc != 0:
        raise RuntimeError("dbcsr_amd_tensor_permute_blocks failed (%d)" % rc)
    _STATS["permute_launches"] += 1
    _STATS["permuted_elements"] += int(elements)


def _check_idx(name, tensor, idx):
    if not isinstance(idx, torch.Tensor) or idx.dtype != torch.int32:
        raise TypeError("%s: idx must be an int32 torch tensor" % name)
    if idx.dim() != 2 or idx.shape[1] != tensor.rank:
        raise ValueError("%s: idx must be (n, %d), got %r" % (name, tensor.rank, tuple(idx.shape)))
    if idx.device != tensor.device:
        raise ValueError("%s: idx is not on the tensor's device" % name)
    return idx.contiguous()


def _list_of(tensor, idx):
    """(rows, cols, sizes, ext) of a list of tensor blocks: int32 matrix coordinates (-1, -1) for an index outside the tensor, int64 element counts (0
    there) and the int64 (n, rank) extents in canonical order (0 there)"""
    nb = tensor.nblks_per_dim
    ok = torch.ones(idx.shape[0], dtype=torch.bool, device=idx.device)
    for d in range(tensor.rank):
        ok &= (idx[:, d] >= 0) & (idx[:, d] < nb[d])
    safe = torch.where(ok[:, None], idx, torch.zeros((), dtype=idx.dtype, device=idx.device)).to(torch.int64)
    minus = torch.full((), -1, dtype=torch.int64, device=idx.device)
    rows = torch.where(ok, combine_index(safe, nb, tensor.map1), minus).to(torch.int32)
    cols = torch.where(ok, combine_index(safe, nb, tensor.map2), minus).to(torch.int32)
    if min(nb) == 0:
        ext = torch.zeros((idx.shape[0], tensor.rank), dtype=torch.int64, device=idx.device)
    else:   # (an entry outside the tensor gets extents of 0: it has no window, and the permute kernel skips it)
        ext = torch.where(ok[:, None], block_extents(safe, tensor.blk_sizes, tuple(range(tensor.rank))), torch.zeros((), dtype=torch.int64, device=idx.device))
    return rows, cols, ext.prod(dim=1), ext


def dbcsr_t_put_blocks(tensor, idx, data, offsets=None, summation=False, engine=None, stream=None):
    """Blocks into the tensor.  idx: (n, rank) int32 on the device; data: one flat tensor of the tensor's type that holds the blocks in canonical
    order (dimension 0 fastest); offsets: int64 device tensor of their element offsets, None: one after another.  One permute launch brings the list
    into the stored order (none when the stored order is canonical), then dbcsr_put_blocks puts it: its rules hold for the order of the list, for
    duplicates (summed in list order with summation, else the last wins), for indices outside the tensor (ValueError, the tensor unchanged) and for
    windows outside data (skipped)."""
    fn = "dbcsr_t_put_blocks"
    idx = _check_idx(fn, tensor, idx)
    _check_flat(fn, "data", data, tensor.matrix)
    n = int(idx.shape[0])
    if offsets is not None:
        offsets = _check_offsets(fn, offsets, n, tensor.device)
    if _data_overlap(data, tensor.matrix.data):
        raise ValueError("%s: data shares memory with the tensor's data area" % fn)
    if n == 0:
        return
    E = engine or default_engine()
    with _on_stream(stream):
        rows, cols, sizes, ext = _list_of(tensor, idx)
        if offsets is None:
            offsets = torch.cumsum(sizes, 0) - sizes
    if tensor.stored_order == tuple(range(tensor.rank)):
        dbcsr_put_blocks(tensor.matrix, rows, cols, data, offsets=offsets, summation=summation, engine=E, stream=stream)
        return
    dbcsr_reserve_blocks(tensor.matrix, rows, cols, engine=E, stream=stream)   # (its errors, before anything moves)
    with _on_stream(stream):
        inside = (offsets >= 0) & (offsets + sizes <= int(data.numel()))
        rows = torch.where(inside, rows, torch.full((), -1, dtype=torch.int32, device=rows.device))
        ends = torch.cumsum(sizes, 0)
        total = int(ends[-1])
        staged = torch.empty(total, dtype=data.dtype, device=data.device)
        st_off = ends - sizes
        _permute(E, stream, data.dtype, tensor.stored_order, _padded_ext(ext), offsets, st_off, data, staged, total)
    dbcsr_put_blocks(tensor.matrix, rows, cols, staged, offsets=st_off, summation=summation, keep_sparsity=True, engine=E, stream=stream)


def dbcsr_t_get_blocks(tensor, idx, out=None, offsets=None, engine=None, stream=None):
    """Blocks out of the tensor: (data, found) with every listed block in canonical order in the flat tensor data at its offset, bit for bit, and
    found[i] = 1; where the tensor stores no such block the window is +0.0 and found[i] = 0; an index outside the tensor has no window.  out, offsets:
    as in dbcsr_get_blocks (an entry whose window does not lie inside out is treated as out of range)."""
    fn = "dbcsr_t_get_blocks"
    idx = _check_idx(fn, tensor, idx)
    n = int(idx.shape[0])
    if out is not None:
        _check_flat(fn, "out", out, tensor.matrix)
        if _data_overlap(out, tensor.matrix.data):
            raise ValueError("%s: out shares memory with the tensor's data area" % fn)
    if offsets is not None:
        offsets = _check_offsets(fn, offsets, n, tensor.device)
    E = engine or default_engine()
    with _on_stream(stream):
        rows, cols, sizes, ext = _list_of(tensor, idx)
    if tensor.stored_order == tuple(range(tensor.rank)) or n == 0:
        return dbcsr_get_blocks(tensor.matrix, rows, cols, out=out, offsets=offsets, engine=E, stream=stream)
    staged, found = dbcsr_get_blocks(tensor.matrix, rows, cols, engine=E, stream=stream)   # (one block after another, in the stored order)
    with _on_stream(stream):
        ends = torch.cumsum(sizes, 0)
        st_off = ends - sizes
        if offsets is None:
            offsets = st_off
        elif out is None and int(offsets.min()) < 0:
            raise ValueError("%s: a negative offset" % fn)
        if out is None:
            out = torch.zeros(max(int((offsets + sizes).max()), 0), dtype=tensor.dtype, device=tensor.device)
        else:
            inside = (offsets >= 0) & (offsets + sizes <= int(out.numel()))
            found = torch.where(inside, found, torch.zeros((), dtype=torch.int32, device=found.device))
        order = tensor.stored_order
        perm = [order.index(j) for j in range(tensor.rank)]   # canonical dimension j is the stored dimension order.index(j)
        _permute(E, stream, tensor.dtype, perm, _padded_ext(ext[:, list(order)]), st_off, offsets, staged, out, int(staged.numel()))
    return out, found


def dbcsr_t_create_from_blocks(blk_sizes, map1, map2, idx, data, offsets=None, summation=True, name="", engine=None, stream=None):
    """A new tensor from a list of blocks: dbcsr_t_create, then dbcsr_t_put_blocks(idx, data, offsets, summation) onto it."""
    if not isinstance(data, torch.Tensor):
        raise TypeError("dbcsr_t_create_from_blocks: data must be a torch tensor")
    T = dbcsr_t_create(blk_sizes, map1, map2, data.dtype, device=data.device, name=name)
    dbcsr_t_put_blocks(T, idx, data, offsets=offsets, summation=summation, engine=engine, stream=stream)
    return T


# ---- copy between mappings ------------------------------------------------------------------------------------------------------------------------------------
def check_order(name, rank, order):
    order = tuple(range(rank)) if order is None else tuple(int(d) for d in order)
    if sorted(order) != list(range(rank)):
        raise ValueError("%s: order %r is no permutation of 0 ... %d" % (name, order, rank - 1))
    return order


def _check_copy(name, tensor_in, tensor_out, order):
    if tensor_in.rank != tensor_out.rank:
        raise ValueError("%s: tensors of rank %d and %d" % (name, tensor_in.rank, tensor_out.rank))
    order = check_order(name, tensor_in.rank, order)
    if tensor_in.dtype != tensor_out.dtype:
        raise TypeError("%s: data types of the two tensors differ" % name)
    for j, d in enumerate(order):
        if not np.array_equal(tensor_out._host_sizes[j], tensor_in._host_sizes[d]):
            raise ValueError("%s: the block sizes of dimension %d of tensor_out are not those of dimension %d of tensor_in" % (name, j, d))
    return order


def _remapped(tensor_in, like_out, order, E, stream):
    """a new packed matrix: tensor_in with dimension j <- its dimension order[j], folded by like_out's mapping.  The index by torch, then one permute
    launch that writes every block straight at its blk_p of the new data area."""
    M = tensor_in.matrix
    with _on_stream(stream, M.row_p.device):
        idx_in = unfold_index(M.row_p, M.col_i, tensor_in.nblks_per_dim, tensor_in.map1, tensor_in.map2)
        idx_out = idx_in[:, list(order)]
        by, row_p, col_i, blk_p, _ = fold_index(idx_out, like_out.blk_sizes, like_out.map1, like_out.map2)
        nze = int(M.nze)   # (known on the host: the element count the index names; the permutation keeps it)
        data = torch.empty(nze, dtype=M.dtype, device=M.data.device)
        dst_off = torch.empty_like(blk_p)
        dst_off[by] = blk_p
        s_in = tensor_in.stored_order
        ext = _padded_ext(block_extents(idx_in, tensor_in.blk_sizes, s_in))
        perm = [s_in.index(order[j]) for j in like_out.stored_order]   # written stored dimension: out dimension j = in dimension order[j]
        _permute(E, stream, M.dtype, perm, ext, M.blk_p, dst_off, M.data, data, nze)
    out = like_out.matrix
    return DbcsrMatrix(out.row_blk_size, out.col_blk_size, row_p, col_i, blk_p, data, out.name)


def _same_folding(tensor_in, tensor_out, order):
    return tuple(order[j] for j in tensor_out.map1) == tensor_in.map1 and tuple(order[j] for j in tensor_out.map2) == tensor_in.map2


def dbcsr_t_copy(tensor_in, tensor_out, order=None, summation=False, engine=None, stream=None):
    """tensor_out <- tensor_in with its dimensions permuted (summation: tensor_out + that).  order follows numpy.transpose: dimension j of tensor_out is
    dimension order[j] of tensor_in; None: the identity.  The block sizes must agree under order (ValueError); the two mappings may be any.  Without
    summation tensor_out afterwards stores exactly the permuted blocks of tensor_in, bit for bit, in a new packed matrix handed over with adopt (as a
    multiply hands its result to matrix_c); tensor_in is not written.  The path: the new index by torch operations, then ONE permute launch from
    tensor_in's data area straight into the new one, no intermediate buffer; with summation the same into a temporary, then dbcsr_add.  When the two
    foldings coincide under order no kernel is launched: a copy of the matrix, or the add."""
    fn = "dbcsr_t_copy"
    order = _check_copy(fn, tensor_in, tensor_out, order)
    if tensor_in is tensor_out or tensor_in.matrix is tensor_out.matrix:
        raise ValueError("%s: tensor_in and tensor_out are the same tensor" % fn)
    E = engine or default_engine()
    if _same_folding(tensor_in, tensor_out, order):
        if summation:
            dbcsr_add(tensor_out.matrix, tensor_in.matrix, 1.0, 1.0, engine=E, stream=stream)
            return
        M = tensor_in.matrix
        with _on_stream(stream, M.row_p.device):
            new = M.copy() if M.packed else E.cropped(M, stream=stream)
        tensor_out.matrix.adopt(DbcsrMatrix(tensor_out.matrix.row_blk_size, tensor_out.matrix.col_blk_size, new.row_p, new.col_i, new.blk_p, new.data))
        return
    new = _remapped(tensor_in, tensor_out, order, E, stream)
    if summation:
        dbcsr_add(tensor_out.matrix, new, 1.0, 1.0, engine=E, stream=stream)
    else:
        tensor_out.matrix.adopt(new)


def _as_tensor(matrix, name):
    if matrix.symmetry != "N":
        raise ValueError("%s: a matrix with symmetry %r" % (name, matrix.symmetry))
    return DbcsrTensor((matrix.row_blk_size, matrix.col_blk_size), (0,), (1,), matrix, matrix.name)


def dbcsr_t_copy_matrix_to_tensor(matrix, tensor, summation=False, engine=None, stream=None):
    """tensor (rank 2, any mapping) <- matrix.  A matrix with symmetry is expanded first (the engine's desymmetrized)."""
    fn = "dbcsr_t_copy_matrix_to_tensor"
    if tensor.rank != 2:
        raise ValueError("%s: a tensor of rank %d" % (fn, tensor.rank))
    E = engine or default_engine()
    full = E.desymmetrized(matrix, stream=stream) if matrix.symmetry != "N" else matrix
    dbcsr_t_copy(_as_tensor(full, fn), tensor, summation=summation, engine=E, stream=stream)


def dbcsr_t_copy_tensor_to_matrix(tensor, matrix, summation=False, engine=None, stream=None):
    """matrix <- tensor (rank 2, any mapping).  The matrix is one without symmetry afterwards."""
    fn = "dbcsr_t_copy_tensor_to_matrix"
    if tensor.rank != 2:
        raise ValueError("%s: a tensor of rank %d" % (fn, tensor.rank))
    E = engine or default_engine()
    if summation and matrix.symmetry != "N":
        matrix.adopt(E.desymmetrized(matrix, stream=stream))
    matrix.symmetry = "N"
    dbcsr_t_copy(tensor, _as_tensor(matrix, fn), summation=summation, engine=E, stream=stream)


def dbcsr_t_filter(tensor, eps, engine=None, stream=None):
    """The blocks whose Frobenius norm is below eps leave the tensor (the engine's block filter on tensor.matrix)."""
    E = engine or default_engine()
    out = E.filtered(tensor.matrix, eps, stream=stream)
    if out is not tensor.matrix:
        tensor.matrix.adopt(out)


# ---- contraction ----------------------------------------------------------------------------------------------------------------------------------------------
def plan_contract(rank_1, rank_2, rank_3, maps_1, maps_2, maps_3, contract_1, notcontract_1, contract_2, notcontract_2, map_1, map_2):
    """The foldings a contraction runs on, from the index tuples and the mappings (map1, map2) the three tensors have -- host integers only.  Returns
    (need_1, need_2, need_3): the (rows | columns) of the three matrices of dbcsr_multiply("N", "N", ...).  tensor_1 is (notcontract_1 | contract_1),
    tensor_2 (contract_2 | notcontract_2), tensor_3 (map_1 | map_2); the order inside each tuple is taken from what the operands have, so that a tensor
    that is folded compatibly (or exactly reversed: "T") is used as it is: the order of the contracted dimensions from tensor_1 if one half of its
    mapping is contract_1 as a set, else from tensor_2; the order of the free dimensions from the operand, else from tensor_3.  ValueError for tuples
    that are not disjoint, do not cover the ranks or do not match each other."""
    fn = "dbcsr_t_contract"
    c1, n1, c2, n2 = (tuple(int(d) for d in t) for t in (contract_1, notcontract_1, contract_2, notcontract_2))
    m1, m2 = tuple(int(d) for d in map_1), tuple(int(d) for d in map_2)
    if sorted(c1 + n1) != list(range(rank_1)):
        raise ValueError("%s: contract_1 %r and notcontract_1 %r do not hold every dimension of tensor_1 exactly once" % (fn, c1, n1))
    if sorted(c2 + n2) != list(range(rank_2)):
        raise ValueError("%s: contract_2 %r and notcontract_2 %r do not hold every dimension of tensor_2 exactly once" % (fn, c2, n2))
    if sorted(m1 + m2) != list(range(rank_3)):
        raise ValueError("%s: map_1 %r and map_2 %r do not hold every dimension of tensor_3 exactly once" % (fn, m1, m2))
    if len(c1) != len(c2) or not c1:
        raise ValueError("%s: contract_1 %r and contract_2 %r must pair up, at least one dimension" % (fn, c1, c2))
    if len(m1) != len(n1) or len(m2) != len(n2) or not n1 or not n2:
        raise ValueError("%s: map_1 / map_2 must pair up with notcontract_1 / notcontract_2, at least one dimension each" % fn)

    def order_from(maps, dims):
        """positions of dims in the order one half of the mapping holds them, None when no half is that set"""
        for half in maps:
            if sorted(half) == sorted(dims):
                return [dims.index(d) for d in half]
        return None

    pc = order_from(maps_1, c1) or order_from(maps_2, c2) or list(range(len(c1)))
    p1 = order_from(maps_1, n1) or order_from(maps_3, m1) or list(range(len(n1)))
    p2 = order_from(maps_2, n2) or order_from(maps_3, m2) or list(range(len(n2)))
    pick = lambda t, p: tuple(t[i] for i in p)
    return (pick(n1, p1), pick(c1, pc)), (pick(c2, pc), pick(n2, p2)), (pick(m1, p1), pick(m2, p2))


def _check_contract_sizes(t1, t2, t3, c1, n1, c2, n2, m1, m2):
    fn = "dbcsr_t_contract"
    for a, b in zip(c1, c2):
        if not np.array_equal(t1._host_sizes[a], t2._host_sizes[b]):
            raise ValueError("%s: the block sizes of dimension %d of tensor_1 and dimension %d of tensor_2 differ" % (fn, a, b))
    for (t, nn, mm, which) in ((t1, n1, m1, 1), (t2, n2, m2, 2)):
        for a, b in zip(nn, mm):
            if not np.array_equal(t._host_sizes[a], t3._host_sizes[b]):
                raise ValueError("%s: the block sizes of dimension %d of tensor_%d and dimension %d of tensor_3 differ" % (fn, a, which, b))


def dbcsr_t_contract(alpha, tensor_1, tensor_2, beta, tensor_3, contract_1, notcontract_1, contract_2, notcontract_2, map_1, map_2, filter_eps=None,
                     retain_sparsity=False, engine=None, stream=None):
    """T3 <- beta*T3 + alpha * sum over the contracted dimensions of T1*T2; returns the flop count of the multiply.  Dimension map_1[a] of tensor_3 is
    dimension notcontract_1[a] of tensor_1, dimension map_2[b] of tensor_3 is dimension notcontract_2[b] of tensor_2, contract_1[c] is summed against
    contract_2[c].  The block sizes of paired dimensions must agree and the tuples must be consistent (ValueError before any device work).  The three
    tensors are brought to the foldings of plan_contract -- a tensor that has its folding is used as it is, an operand that has exactly the reversed one
    takes "T" in the multiply, anything else is remapped with one permute launch (dbcsr_t_copy); a tensor_3 of another folding is not remapped on the way
    in when beta == 0 and retain_sparsity is off -- then dbcsr_multiply("N" / "T", "N" / "T", ...) runs with filter_eps and retain_sparsity passed through,
    and a tensor_3 of another folding receives the result through one more remap."""
    fn = "dbcsr_t_contract"
    t1, t2, t3 = tensor_1, tensor_2, tensor_3
    need = plan_contract(t1.rank, t2.rank, t3.rank, (t1.map1, t1.map2), (t2.map1, t2.map2), (t3.map1, t3.map2), contract_1, notcontract_1, contract_2,
                         notcontract_2, map_1, map_2)
    (n1, c1), (c2, n2), (m1, m2) = need
    _check_contract_sizes(t1, t2, t3, c1, n1, c2, n2, m1, m2)
    if t1.dtype != t2.dtype or t1.dtype != t3.dtype:
        raise TypeError("%s: data types of the three tensors differ" % fn)
    E = engine or default_engine()
    with _on_stream(stream, t3.device):   # (dbcsr_multiply and the remaps run on the current stream: `stream` is made current for all of it)
        return _contract(E, alpha, t1, t2, beta, t3, need, filter_eps, retain_sparsity)


def _contract(E, alpha, t1, t2, beta, t3, need, filter_eps, retain_sparsity):
    (n1, c1), (c2, n2), (m1, m2) = need

    def operand(t, rows, cols):
        if (t.map1, t.map2) == (rows, cols):
            return t.matrix, "N"
        if (t.map1, t.map2) == (cols, rows):
            return t.matrix, "T"
        r = _like(t, rows, cols)
        dbcsr_t_copy(t, r, engine=E)
        return r.matrix, "N"

    A, ta = operand(t1, n1, c1)
    B, tb = operand(t2, c2, n2)
    direct = (t3.map1, t3.map2) == (m1, m2)
    if direct:
        Ct = t3
    else:
        Ct = _like(t3, m1, m2)
        if beta != 0 or retain_sparsity:
            dbcsr_t_copy(t3, Ct, engine=E)
    counts = dbcsr_multiply(ta, tb, alpha, A, B, beta, Ct.matrix, retain_sparsity=retain_sparsity, filter_eps=filter_eps, engine=E)
    if not direct:
        dbcsr_t_copy(Ct, t3, engine=E)
    return int(counts.flop)
