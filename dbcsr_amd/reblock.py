"""A matrix under another block structure, on the device and without leaving the block-sparse form -- what the reference offers as
dbcsr_complete_redistribute (a copy between matrices of different blockings: CP2K goes from atomic to molecular or clustered blocks with it) and, for
tensors, as dbcsr_t_split_blocks:

    dbcsr_reblock(matrix, row_blk_size, col_blk_size)      a new packed matrix under the new structure
    dbcsr_reblock_into(matrix_in, matrix_out)              onto the blocks matrix_out stores: the keep_sparsity form and the way back
    dbcsr_merged_block_sizes(sizes, target)                host helper: consecutive blocks joined while the sum stays <= target
    dbcsr_split_block_sizes(sizes, max_size)               host helper: every block cut into pieces of at most max_size, as equal as possible

The reference's sources are not available here: the two rules are the semantics of this library.  Let A be a matrix without symmetry and (rs', cs') a
second block structure with the same sums of sizes, every size >= 1.
    pattern  a new block (I, J) is stored iff its element rectangle intersects the rectangle of at least one block that A's index names.  Values play
             no part: a stored block full of zeros counts, and the holes of an unpacked data area are never read.
    values   an element of a stored new block is the element of A at the same (row, column), bit for bit (-0.0, NaN and +-Inf included), where A's
             index names a block there, and +0.0 elsewhere.
Blocks are column-major as everywhere in the library.  The work is done by the C-ABI engine (include/dbcsr_amd_mm.h, "Re-blocking") on the GPU, for
float64, float32 and complex128 data."""
import ctypes as C

import torch

from .matrix import DbcsrMatrix, StreamHandle, _serial
from .multiply import default_engine
from .operations import _block_sizes, _check_symmetry, _data_overlap, _full_size, _on_stream

_INT32_MAX = 2 ** 31 - 1
_MIN_SIZES = {}    # (serial of a size tensor, its version) -> its smallest entry: fetched once per tensor, as _full_size fetches the sum
_PIECES = {}       # (index_stamp of the source, the two new size tensors) -> the length of the list of pieces, which only the device knows


def _sizes_list(name, what, sizes):
    """a sequence of block sizes as a list of Python integers, every one in [1, 2^31 - 1]"""
    try:
        out = [int(s) for s in sizes]
    except TypeError:
        raise TypeError("%s: %s must be a sequence of integers" % (name, what))
    if any(isinstance(s, (float, complex)) or int(s) != s for s in sizes):
        raise TypeError("%s: %s must be a sequence of integers" % (name, what))
    if any(s < 1 for s in out):
        raise ValueError("%s: %s has a block size below 1" % (name, what))
    if any(s > _INT32_MAX for s in out):
        raise ValueError("%s: %s has a block size above 2^31 - 1" % (name, what))
    return out


def dbcsr_merged_block_sizes(sizes, target):
    """Consecutive blocks joined greedily while the sum stays <= target; a block larger than target stays alone.  Pure Python: a list of integers that
    fit int32, with the same sum as sizes."""
    fn = "dbcsr_merged_block_sizes"
    sizes = _sizes_list(fn, "sizes", sizes)
    if isinstance(target, bool) or int(target) != target or int(target) < 1:
        raise ValueError("%s: target must be an integer >= 1, got %r" % (fn, target))
    target = int(target)
    out, cur = [], 0
    for s in sizes:
        if cur and cur + s <= target:
            cur += s
        else:
            if cur:
                out.append(cur)
            cur = s
    if cur:
        out.append(cur)
    if any(s > _INT32_MAX for s in out):
        raise ValueError("%s: a merged block above 2^31 - 1" % fn)
    return out


def dbcsr_split_block_sizes(sizes, max_size):
    """Every block cut into ceil(size / max_size) pieces, as equal as possible (the larger pieces first: 23 at max_size 12 gives 12, 11).  Pure Python:
    a list of integers with the same sum as sizes."""
    fn = "dbcsr_split_block_sizes"
    sizes = _sizes_list(fn, "sizes", sizes)
    if isinstance(max_size, bool) or int(max_size) != max_size or int(max_size) < 1:
        raise ValueError("%s: max_size must be an integer >= 1, got %r" % (fn, max_size))
    max_size = int(max_size)
    out = []
    for s in sizes:
        k = -(-s // max_size)
        base, rem = divmod(s, k)
        out += [base + 1] * rem + [base] * (k - rem)
    return out


def _min_size(sizes):
    key = (_serial(sizes), sizes._version)
    n = _MIN_SIZES.get(key)
    if n is None:
        if len(_MIN_SIZES) > 256:
            _MIN_SIZES.clear()
        n = _MIN_SIZES[key] = int(sizes.min().item()) if sizes.numel() else 1
    return n


def _new_sizes(name, what, sizes, device, total):
    """the new block sizes as the matrices hold them (an int32 device tensor is taken as it is), every one >= 1, summing to `total`"""
    if not isinstance(sizes, torch.Tensor):
        sizes = _sizes_list(name, what, sizes)   # (checked on the host, before anything reaches the device)
        if sum(sizes) != total:
            raise ValueError("%s: %s sums to %d, the matrix has %d" % (name, what, sum(sizes), total))
        return _block_sizes(name, what, sizes, device)
    t = _block_sizes(name, what, sizes, device)
    if _min_size(t) < 1:
        raise ValueError("%s: %s has a block size below 1" % (name, what))
    if _full_size(t) != total:
        raise ValueError("%s: %s sums to %d, the matrix has %d" % (name, what, _full_size(t), total))
    return t


def _check_source(name, what, matrix):
    """a known symmetry and type, arrays on a GPU: before any call of the library"""
    if not isinstance(matrix, DbcsrMatrix):
        raise TypeError("%s: %s must be a DbcsrMatrix" % (name, what))
    sym = _check_symmetry(name, matrix)
    matrix.dtype_code
    if sym != "N":
        matrix.symmetry_kind()
    if matrix.row_p.device.type != "cuda" or matrix.data.device.type != "cuda":
        raise ValueError("%s: %s is on the host" % (name, what))
    return sym


def _gather(fn, E, st, src, dst):
    a, b = src.desc(), dst.desc()   # (only dst's data area is written)
    rc = E.L.dbcsr_amd_bcsr_reblock_gather(E.h, src.dtype_code, C.byref(a), C.byref(b), st.ptr)
    if rc != 0:
        raise RuntimeError("dbcsr_amd_bcsr_reblock_gather failed (%d)" % rc)


def dbcsr_reblock(matrix, row_blk_size, col_blk_size, name="", engine=None, stream=None):
    """A new packed matrix without symmetry under the block structure row_blk_size x col_blk_size, by the two rules of this module: the blocks whose
    rectangle meets a stored block of `matrix`, each element the element of `matrix` at its place or +0.0; block columns ascend per block row.  The
    block sizes: int32 device tensors as the matrices hold them (taken as they are), or any sequence of integers; every size >= 1 and the sums those
    of the matrix (ValueError).  A matrix with symmetry ('S' 'A' 'H' 'K') is first expanded with MultiplyEngine.desymmetrized; otherwise the matrix is
    only read: it keeps its index_stamp() and its data bits.  The same sizes as a packed source give the source's index and data bit for bit, in new
    tensors; a matrix without blocks gives a matrix without blocks.  Every source block names the new blocks it meets (binary searches in the running
    sums of the new sizes, on the device), the list builds the pattern through the reserve's count on an empty matrix, the index alone is applied, and
    one gather writes the new data area once -- it is never zero-filled.  Synchronises for the counts: the reserve's once per call, the length of the
    list once per pair (index of the source, new size tensors), and the gather once when it meets the new matrix' sizes.  float64, float32 and
    complex128; the same bits on every call; every refusal comes before any call of the library."""
    fn = "dbcsr_reblock"
    sym = _check_source(fn, "matrix", matrix)
    dev = matrix.row_p.device
    rs = _new_sizes(fn, "row_blk_size", row_blk_size, dev, _full_size(matrix.row_blk_size))
    cs = _new_sizes(fn, "col_blk_size", col_blk_size, dev, _full_size(matrix.col_blk_size))
    E = engine or default_engine()
    if sym != "N":
        matrix = E.desymmetrized(matrix, stream=stream)
    st = StreamHandle(stream)
    nbr, nbc = int(rs.numel()), int(cs.numel())
    with _on_stream(stream):
        M = DbcsrMatrix.empty_like_pattern(rs, cs, matrix.dtype, device=dev, name=name)
    if matrix.nblks == 0 or nbr == 0 or nbc == 0:
        return M
    src = matrix.desc()
    key = (matrix.index_stamp(), _serial(rs), rs._version, _serial(cs), cs._version)
    n = _PIECES.get(key)
    if n is None:
        total = C.c_int64()
        rc = E.L.dbcsr_amd_bcsr_reblock_name_blocks(E.h, C.byref(src), rs.data_ptr(), cs.data_ptr(), nbr, nbc, C.byref(total), None, None, st.ptr)
        if rc != 0:
            raise RuntimeError("dbcsr_amd_bcsr_reblock_name_blocks failed (%d)" % rc)
        if len(_PIECES) > 256:
            _PIECES.clear()
        n = _PIECES[key] = int(total.value)
    if n == 0:
        return M
    with _on_stream(stream):
        rows = torch.empty(n, dtype=torch.int32, device=dev)
        cols = torch.empty(n, dtype=torch.int32, device=dev)
        row_p = torch.empty(nbr + 1, dtype=torch.int32, device=dev)
    total = C.c_int64(n)
    rc = E.L.dbcsr_amd_bcsr_reblock_name_blocks(E.h, C.byref(src), rs.data_ptr(), cs.data_ptr(), nbr, nbc, C.byref(total), rows.data_ptr(), cols.data_ptr(),
                                                st.ptr)
    if rc != 0:
        raise RuntimeError("dbcsr_amd_bcsr_reblock_name_blocks failed (%d)" % rc)
    m = M.desc()
    nb, nz, new, bad = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
    rc = E.L.dbcsr_amd_bcsr_reserve_count(E.h, C.byref(m), n, rows.data_ptr(), cols.data_ptr(), 0, row_p.data_ptr(), C.byref(nb), C.byref(nz),
                                          C.byref(new), C.byref(bad), st.ptr)
    if rc != 0 or bad.value or new.value == 0:
        raise RuntimeError("dbcsr_amd_bcsr_reserve_count failed (%d: %d of %d pieces outside the new structure, %d blocks)" % (rc, bad.value, n, new.value))
    with _on_stream(stream):
        out = DbcsrMatrix(rs, cs, row_p, torch.empty(nb.value, dtype=torch.int32, device=dev), torch.empty(nb.value, dtype=torch.int64, device=dev),
                          torch.empty(nz.value, dtype=matrix.dtype, device=dev), name)
    dst = out.desc(out=True)
    rc = E.L.dbcsr_amd_bcsr_reserve_apply_index(E.h, C.byref(m), C.byref(dst), st.ptr)
    if rc != 0:
        raise RuntimeError("dbcsr_amd_bcsr_reserve_apply_index failed (%d)" % rc)
    _gather(fn, E, st, matrix, out)
    return out


def dbcsr_reblock_into(matrix_in, matrix_out, engine=None, stream=None):
    """The keep_sparsity form and the way back: every element of every block matrix_out stores is written exactly once -- the element of matrix_in at
    its (row, column) where matrix_in's index names a block there, bit for bit, +0.0 elsewhere -- and nothing else.  No index array is written:
    matrix_out.index_stamp() stays and a multiply that had matrix_out as operand reuses its plan; the holes of an unpacked matrix_out keep their bits;
    the block norms a multiply announced are forgotten, as in dbcsr_from_csr.  The two matrices may have any two block structures with the same sums
    (ValueError otherwise); with the same structure this is dbcsr_copy(..., keep_sparsity=True) by another route, with the same bits.  matrix_in with
    symmetry is first expanded with MultiplyEngine.desymmetrized; matrix_out is served on its stored blocks as they are.  The matrices must be on one
    device, of one data type, and must not share a data area.  Asynchronous on the stream: nothing synchronises once the engine knows both sets of
    block sizes (the first call for a set fetches its sums).  float64, float32 and complex128; every refusal comes before any call of the library.
    Returns matrix_out."""
    fn = "dbcsr_reblock_into"
    sym = _check_source(fn, "matrix_in", matrix_in)
    _check_source(fn, "matrix_out", matrix_out)
    if matrix_in.row_p.device != matrix_out.row_p.device or matrix_in.data.device != matrix_out.data.device:
        raise ValueError("%s: the two matrices are on different devices" % fn)
    if matrix_in.dtype != matrix_out.dtype:
        raise TypeError("%s: the data types of the two matrices differ" % fn)
    for what, a, b in (("row", matrix_in.row_blk_size, matrix_out.row_blk_size), ("column", matrix_in.col_blk_size, matrix_out.col_blk_size)):
        if a is not b and _full_size(a) != _full_size(b):
            raise ValueError("%s: the %s block sizes sum to %d and %d" % (fn, what, _full_size(a), _full_size(b)))
    if matrix_in is matrix_out or _data_overlap(matrix_in.data, matrix_out.data):
        raise ValueError("%s: the two matrices share a data area" % fn)
    E = engine or default_engine()
    if sym != "N":
        matrix_in = E.desymmetrized(matrix_in, stream=stream)
    _gather(fn, E, StreamHandle(stream), matrix_in, matrix_out)
    return matrix_out
