"""Element CSR <-> block-sparse on the device -- host-side mirror of the reference's conversion between a matrix and the element-wise CSR form
(src/ops/dbcsr_csr_conversions.F: dbcsr_csr_create_from_dbcsr, dbcsr_convert_dbcsr_to_csr, dbcsr_convert_csr_to_dbcsr, dbcsr_to_csr_filter; what CP2K
hands to PEXSI and writes with KS_CSR_WRITE):

    dbcsr_to_csr(matrix, eps)                                        (crow, col, values) of the elements the index names, or of those above eps
    dbcsr_from_csr(crow, col, values, matrix)                        the stored blocks <- the CSR's elements, +0.0 where it has none
    dbcsr_create_from_csr(crow, col, values, row_blk_size, col_blk_size)  a new matrix of the blocks that hold at least one CSR entry
    dbcsr_csr_to_torch(crow, col, values, shape)                     the three arrays as a torch.sparse_csr_tensor

The CSR form of this library: crow[n_rows + 1] int64 with crow[0] = 0 (positions pass 2^31 on matrices that fit one GPU), col[nnz] int32, 0-based
element columns ascending inside a row, values[nnz] of the matrix' type -- all three device tensors.  It is what torch.sparse_csr_tensor, hipSPARSE and
outside sparse solvers take, and what a matrix arrives in when it was not built by DBCSR.

The reference's source is not available here: the rule of the eps filter (an element is dropped iff |x| <= eps) is the semantics of this library.  The
work is done by the C-ABI engine (include/dbcsr_amd_mm.h, "Element CSR") on the GPU, for float64, float32 and complex128 data."""
import ctypes as C

import torch

from .matrix import DbcsrMatrix, StreamHandle, _dtype_code
from .multiply import default_engine
from .operations import _block_sizes, _check_symmetry, _data_overlap, _full_size, _on_stream, dbcsr_reserve_blocks

_MAX_COLS = 2 ** 31 - 1


def _check_matrix(name, matrix):
    """what both directions ask of the matrix, before any call of the library: a known symmetry and type, arrays on a GPU, columns that fit int32"""
    sym = _check_symmetry(name, matrix)
    matrix.dtype_code
    if sym != "N":
        matrix.symmetry_kind()
    n_rows, n_cols = _full_size(matrix.row_blk_size), _full_size(matrix.col_blk_size)
    if n_cols > _MAX_COLS:
        raise ValueError("%s: %d element columns: col is int32" % (name, n_cols))
    if matrix.row_p.device.type != "cuda" or matrix.data.device.type != "cuda":
        raise ValueError("%s: the matrix is on the host" % name)
    return sym, n_rows, n_cols


def _check_csr(name, crow, col, values, dtype, device, n_rows):
    """crow int64 [n_rows + 1], col int32 [nnz], values [nnz] of `dtype`: 1-D tensors on `device`, checked before any call of the library"""
    for what, t, dt in (("crow", crow, torch.int64), ("col", col, torch.int32), ("values", values, dtype)):
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s: %s must be a torch tensor" % (name, what))
        if t.dtype != dt:
            raise TypeError("%s: %s has data type %r, expected %r" % (name, what, t.dtype, dt))
        if t.dim() != 1:
            raise ValueError("%s: %s must be 1-D, got %d dimensions" % (name, what, t.dim()))
        if t.device != device:
            raise ValueError("%s: %s is not on the device of the matrix" % (name, what))
    if n_rows is not None and crow.numel() != n_rows + 1:
        raise ValueError("%s: crow has %d entries, the matrix has %d rows" % (name, crow.numel(), n_rows))
    if crow.numel() < 1:
        raise ValueError("%s: crow is empty (it has n_rows + 1 entries)" % name)
    if col.numel() != values.numel():
        raise ValueError("%s: col and values differ in length (%d, %d)" % (name, col.numel(), values.numel()))
    return crow.contiguous(), col.contiguous(), values.contiguous()


def dbcsr_to_csr(matrix, eps=None, engine=None, stream=None):
    """The element-wise CSR form (crow, col, values) of the matrix, without leaving the device (dbcsr_convert_dbcsr_to_csr; dbcsr_to_csr_filter with eps).
    eps=None: every element the index names is an entry, bit for bit (-0.0, NaN and Inf included): nnz == matrix.nze, crow comes from the index alone
    and no element is read for it; nothing synchronises once the engine has met the index (the first call for an index fetches its sizes).  eps >= 0: an
    element is DROPPED iff |x| <= eps -- real types compare in their own precision, complex ones hypot(re, im) in double -- so eps = 0 drops exactly +-0
    and a NaN stays; this costs one synchronisation, for nnz.  The reference's source is not available here: this rule is this library's semantics.
    Everything goes by the index: the holes of an unpacked matrix are never read.  A matrix with symmetry ('S' 'A' 'H' 'K') is first expanded with
    MultiplyEngine.desymmetrized (which uses the engine's work areas, as every expansion does).  Otherwise the matrix is only read: it keeps its
    index_stamp() and no saved plan is touched.  float64, float32 and complex128; the same bits on every call; every refusal -- eps < 0 or NaN, a matrix
    on the host, more than 2^31 - 1 element columns -- comes before any call of the library."""
    name = "dbcsr_to_csr"
    if eps is not None:
        eps = float(eps)
        if not eps >= 0:   # (a NaN compares false)
            raise ValueError("%s: eps must be None or >= 0, got %r" % (name, eps))
    sym, n_rows, n_cols = _check_matrix(name, matrix)
    E = engine or default_engine()
    if sym != "N":
        matrix = E.desymmetrized(matrix, stream=stream)
    st = StreamHandle(stream)
    dev = matrix.row_p.device
    code = matrix.dtype_code
    with _on_stream(stream):
        crow = torch.empty(n_rows + 1, dtype=torch.int64, device=dev)
    d = matrix.desc()
    nnz = C.c_int64()
    rc = E.L.dbcsr_amd_bcsr_to_csr_count(E.h, code, C.byref(d), 0 if eps is None else 1, 0.0 if eps is None else eps, crow.data_ptr(), C.byref(nnz),
                                         st.ptr)
    if rc != 0:
        raise RuntimeError("dbcsr_amd_bcsr_to_csr_count failed (%d)" % rc)
    with _on_stream(stream):
        col = torch.empty(nnz.value, dtype=torch.int32, device=dev)
        values = torch.empty(nnz.value, dtype=matrix.dtype, device=dev)
    rc = E.L.dbcsr_amd_bcsr_to_csr_apply(E.h, code, C.byref(d), col.data_ptr() if nnz.value else None, values.data_ptr() if nnz.value else None, st.ptr)
    if rc != 0:
        raise RuntimeError("dbcsr_amd_bcsr_to_csr_apply failed (%d)" % rc)
    return crow, col, values


def dbcsr_from_csr(crow, col, values, matrix, engine=None, stream=None):
    """The mirror of dbcsr_from_dense (dbcsr_convert_csr_to_dbcsr onto an existing pattern): every element of every block the matrix stores is written
    exactly once -- the CSR value at its (row, column), or +0.0 where the CSR has none -- and nothing else.  No index array is written: index_stamp()
    stays and a multiply afterwards reuses its plan; the holes of an unpacked matrix keep their bits; block norms a multiply announced are forgotten.
    CSR entries whose block the matrix does not store are ignored, as are entries with a column outside [0, n_cols).  Contract: columns ascend strictly
    inside a row -- what dbcsr_to_csr and torch's to_sparse_csr() produce; a CSR that breaks it gives wrong values but never an access outside col /
    values or outside the blocks.  No symmetry is applied: of a stored triangle the stored blocks take the elements at their places.  values must not
    share memory with matrix.data (ValueError).  Asynchronous on the stream, nothing synchronises (the first call for a set of block sizes fetches their
    sums); every refusal comes before any call of the library.  Returns matrix."""
    name = "dbcsr_from_csr"
    _, n_rows, n_cols = _check_matrix(name, matrix)
    crow, col, values = _check_csr(name, crow, col, values, matrix.dtype, matrix.row_p.device, n_rows)
    if _data_overlap(values, matrix.data):
        raise ValueError("%s: values shares memory with the matrix' data area" % name)
    E = engine or default_engine()
    st = StreamHandle(stream)
    nnz = int(col.numel())
    d = matrix.desc()   # (only the data area is written)
    rc = E.L.dbcsr_amd_bcsr_from_csr(E.h, matrix.dtype_code, n_rows, n_cols, nnz, crow.data_ptr(), col.data_ptr() if nnz else None,
                                     values.data_ptr() if nnz else None, C.byref(d), st.ptr)
    if rc != 0:
        raise RuntimeError("dbcsr_amd_bcsr_from_csr failed (%d)" % rc)
    return matrix


def dbcsr_create_from_csr(crow, col, values, row_blk_size, col_blk_size, name="", engine=None, stream=None):
    """A new packed matrix without symmetry of the blocks of the structure row_blk_size x col_blk_size that hold at least one CSR entry (explicit zeros
    count), filled with dbcsr_from_csr: the device-side way in for a matrix that arrives as CSR (dbcsr_convert_csr_to_dbcsr into a new matrix).  crow
    has one entry more than the block sizes sum to rows (ValueError otherwise).  Every entry is given its block by binary searches in the running sums
    of the block sizes on the device; the list builds the pattern with dbcsr_reserve_blocks on an empty matrix (its one synchronisation; an entry
    outside the block structure: its ValueError).  The block sizes: int32 device tensors as the matrices hold them (taken as they are), or any
    sequence of integers.  float64, float32 and complex128."""
    fn = "dbcsr_create_from_csr"
    if not isinstance(values, torch.Tensor):
        raise TypeError("%s: values must be a torch tensor" % fn)
    _dtype_code(values.dtype)
    if values.device.type != "cuda":
        raise ValueError("%s: values is not on a GPU" % fn)
    dev = values.device
    rs, cs = _block_sizes(fn, "row_blk_size", row_blk_size, dev), _block_sizes(fn, "col_blk_size", col_blk_size, dev)
    n_rows, n_cols = _full_size(rs), _full_size(cs)
    if n_cols > _MAX_COLS:
        raise ValueError("%s: %d element columns: col is int32" % (fn, n_cols))
    crow, col, values = _check_csr(fn, crow, col, values, values.dtype, dev, n_rows)
    nnz = int(col.numel())
    if nnz > 2 ** 31 - 1:
        raise ValueError("%s: a CSR of %d entries (the block list is 32-bit)" % (fn, nnz))
    E = engine or default_engine()
    st = StreamHandle(stream)
    nbr, nbc = int(rs.numel()), int(cs.numel())
    with _on_stream(stream):
        M = DbcsrMatrix.empty_like_pattern(rs, cs, values.dtype, device=dev, name=name)
        rows = torch.empty(nnz, dtype=torch.int32, device=dev)
        cols = torch.empty(nnz, dtype=torch.int32, device=dev)
    if nnz == 0:
        return M
    rc = E.L.dbcsr_amd_bcsr_csr_name_blocks(E.h, n_rows, nnz, crow.data_ptr(), col.data_ptr(), rs.data_ptr() if nbr else None, cs.data_ptr() if nbc else None,
                                            nbr, nbc, rows.data_ptr(), cols.data_ptr(), st.ptr)
    if rc != 0:
        raise RuntimeError("dbcsr_amd_bcsr_csr_name_blocks failed (%d)" % rc)
    dbcsr_reserve_blocks(M, rows, cols, engine=E, stream=stream)
    return dbcsr_from_csr(crow, col, values, M, engine=E, stream=stream)


def dbcsr_csr_to_torch(crow, col, values, shape):
    """torch.sparse_csr_tensor of the three arrays (col widened to int64, which torch asks for beside an int64 crow)"""
    return torch.sparse_csr_tensor(crow, col.to(torch.int64), values, size=tuple(shape))
