"""Matrix algebra between multiplies -- host-side mirror of the reference's element-wise and reduction operations
(src/ops/dbcsr_operations.F) on device-resident matrices:

    dbcsr_add(matrix_a, matrix_b, alpha_scalar, beta_scalar)    A <- alpha*A + beta*B
    dbcsr_scale(matrix, alpha)                                  A <- alpha*A
    dbcsr_add_on_diag(matrix, alpha)                            A <- A + alpha*I
    dbcsr_trace(matrix)                                         sum of the diagonal elements
    dbcsr_dot(matrix_a, matrix_b)                               sum a_ij * b_ij = trace(A^T B)          (real data)
    dbcsr_frobenius_norm(matrix)                                sqrt(sum |x|^2)
    dbcsr_maxabs_norm(matrix)                                   max |x|
    dbcsr_gershgorin_norm(matrix)                               max_i sum_j |a_ij|
    dbcsr_norm(matrix, which_norm, norm_vector)                 one of the three, or the column norms sqrt(sum_i |a_ij|^2)
    dbcsr_get_diag(matrix) / dbcsr_set_diag(matrix, diag)       the diagonal as a device vector
    dbcsr_scale_by_vector(matrix, alpha, side)                  A <- A*diag(alpha) ("right") or diag(alpha)*A ("left")
    dbcsr_matvec(matrix, vec_in, vec_out, alpha, beta, trans)   y <- alpha*op(A)*x + beta*y with dense device vectors (not a mirror, see there)
    dbcsr_multivec(matrix, vecs_in, vecs_out, alpha, beta, trans)  Y <- alpha*op(A)*X + beta*Y with nrhs dense device vectors at once: A is read once
    dbcsr_rank_update(matrix, vecs_x, vecs_y, alpha, beta, trans)  A_IJ <- beta*A_IJ + alpha*X_I*op(Y_J) on the stored blocks only (not a mirror, see there)
    dbcsr_multiply_dense(matrix, dense_in, dense_out, alpha, beta, trans)  Y <- alpha*op(A)*X + beta*Y with a dense operand of many columns, row by row
                                                                or column by column, on the matrix cores (not a mirror, see there)
    dbcsr_get_block_diag(matrix)                                a new matrix of the diagonal blocks the matrix stores
    dbcsr_invert_block_diag(matrix, check)                      every stored diagonal block <- its inverse, in place (not a mirror, see there)
    dbcsr_scale_by_block_diag(matrix, diag, side, trans, alpha) A_IJ <- alpha*op(D_I)*A_IJ ("left"), alpha*A_IJ*op(D_J) ("right") or both, in place (not a mirror)
    dbcsr_to_dense(matrix, out)                                 the full matrix as a dense device tensor (dbcsr_to_dense_local / copy_dbcsr_to_fm)
    dbcsr_from_dense(dense, matrix)                             the stored blocks <- the dense tensor's elements (copy_fm_to_dbcsr, keep_sparsity)
    dbcsr_create_from_dense(dense, row_blk_size, col_blk_size, eps)  a new matrix of the blocks of a dense tensor that the block filter keeps
    dbcsr_hadamard_product(matrix_a, matrix_b, matrix_c, b_assume_value)  C <- A o B on the blocks both store (or on A's, B's missing blocks assumed)
    dbcsr_copy(matrix_b, matrix_a, keep_sparsity)               B <- A; keep_sparsity: A projected onto B's pattern, in place
    dbcsr_function_of_elements(matrix_a, func, a0, a1)          x <- f(a1*x + a0) in place, func one of dbcsr_func_*                 (real data)
    dbcsr_reserve_blocks(matrix, rows, cols)                    the pattern grows by a list of blocks, new blocks are zero; returns the number created
    dbcsr_put_blocks(matrix, rows, cols, data, offsets, summation, alpha, keep_sparsity)  A_rc <- [A_rc +] alpha*X per list entry, in list order (dbcsr_put_block)
    dbcsr_get_blocks(matrix, rows, cols, out, offsets)          (data, found): the listed blocks bit for bit, zero where absent (dbcsr_get_block_p)
    dbcsr_reserve_diag_blocks(matrix) / dbcsr_reserve_all_blocks(matrix)  the diagonal / every block reserved
    dbcsr_create_from_blocks(row_blk_size, col_blk_size, rows, cols, data, offsets, summation)  a new matrix from a list of blocks

Same argument names and error behaviour; the work is done by the C-ABI engine (include/dbcsr_amd_mm.h, "Matrix algebra between
multiplies") on the GPU, for float64, float32 and complex128 data.  One rank / one device here: of a distributed matrix trace, dot
and the squared norm are the local results summed over the ranks."""
import ctypes as C
import math

import torch

from .matrix import DbcsrMatrix, StreamHandle, _dtype_code, _serial
from .multiply import _z, default_engine

_SYMMETRIES = ("N", "S", "A", "H", "K")

# which_norm of dbcsr_norm (the reference's constants)
dbcsr_norm_frobenius = 1
dbcsr_norm_maxabsnorm = 2
dbcsr_norm_gershgorin = 3
dbcsr_norm_column = 4


def _check_symmetry(name, m):
    s = getattr(m, "symmetry", "N")
    if s not in _SYMMETRIES:
        raise ValueError("%s: unsupported matrix symmetry %r" % (name, s))
    return s


def _check_scalar(name, m, *scalars):
    if not m.dtype.is_complex and any(isinstance(s, complex) for s in scalars):
        raise TypeError("%s: complex scalars with real matrices" % name)


def _same_sizes(a, b):
    return (a.nblkrows == b.nblkrows and a.nblkcols == b.nblkcols and
            (a.row_blk_size is b.row_blk_size or torch.equal(a.row_blk_size, b.row_blk_size)) and
            (a.col_blk_size is b.col_blk_size or torch.equal(a.col_blk_size, b.col_blk_size)))


def _check_pair(name, a, b):
    """the conditions two operands of an add or a dot must meet, before any device call of the library"""
    if a.dtype != b.dtype:
        raise TypeError("%s: data types of the two matrices differ" % name)
    sa, sb = _check_symmetry(name, a), _check_symmetry(name, b)
    if sa != sb:
        raise ValueError("%s: matrices of different symmetry (%r, %r): summing general with symmetric matrix NYI" % (name, sa, sb))
    if not _same_sizes(a, b):
        raise ValueError("%s: row or column block sizes of the two matrices differ" % name)
    return sa


def dbcsr_add(matrix_a, matrix_b, alpha_scalar=1.0, beta_scalar=1.0, engine=None, stream=None):
    """A <- alpha*A + beta*B (dbcsr_add).  The result's block pattern is the union of both patterns, its blocks packed; with
    beta == 0 only A is scaled, its pattern stays and B is not read.  Blocks of A stay stored with alpha == 0.  Matrices with symmetry are
    added on their stored triangles.  When B has A's index (row_p, col_i, blk_p) and A is packed -- the usual case inside an iteration --
    the add is one flat pass in place: A keeps its index tensors and its index_stamp(), so a multiply with A as operand still reuses
    its plan.  Returns True in that case, False when A was handed a new index."""
    _check_pair("dbcsr_add", matrix_a, matrix_b)
    _check_scalar("dbcsr_add", matrix_a, alpha_scalar, beta_scalar)
    E = engine or default_engine()
    st = StreamHandle(stream)
    A, B = matrix_a, matrix_b
    dev = A.row_p.device
    a, b = A.desc(), B.desc()
    row_p = torch.empty(A.nblkrows + 1, dtype=torch.int32, device=dev)
    nb, nz, same = C.c_int64(), C.c_int64(), C.c_int32()
    rc = E.L.dbcsr_amd_bcsr_add_count(E.h, C.byref(a), C.byref(b), 1 if beta_scalar == 0 else 0, row_p.data_ptr(), C.byref(nb), C.byref(nz),
                                      C.byref(same), st.ptr)
    if rc != 0:
        raise RuntimeError("dbcsr_amd_bcsr_add_count failed (%d)" % rc)
    if same.value:
        # in place: the descriptor of A itself is the destination, no index array is written (A.desc(out=True) would bump the stamp)
        rc = E.L.dbcsr_amd_bcsr_add_apply(E.h, A.dtype_code, _z(alpha_scalar), C.byref(a), _z(beta_scalar), C.byref(b), C.byref(a), st.ptr)
        if rc != 0:
            raise RuntimeError("dbcsr_amd_bcsr_add_apply failed (%d)" % rc)
        return True
    out = DbcsrMatrix(A.row_blk_size, A.col_blk_size, row_p, torch.empty(nb.value, dtype=torch.int32, device=dev),
                      torch.empty(nb.value, dtype=torch.int64, device=dev), torch.empty(nz.value, dtype=A.dtype, device=dev), A.name)
    dst = out.desc(out=True)
    rc = E.L.dbcsr_amd_bcsr_add_apply(E.h, A.dtype_code, _z(alpha_scalar), C.byref(a), _z(beta_scalar), C.byref(b), C.byref(dst), st.ptr)
    if rc != 0:
        raise RuntimeError("dbcsr_amd_bcsr_add_apply failed (%d)" % rc)
    matrix_a.adopt(out)   # as a multiply hands its result to matrix_c
    return False


def dbcsr_scale(matrix, alpha, engine=None, stream=None):
    """A <- alpha*A in place, on every block the index names (dbcsr_scale without limits); alpha == 1 touches nothing."""
    _check_symmetry("dbcsr_scale", matrix)
    _check_scalar("dbcsr_scale", matrix, alpha)
    matrix.dtype_code   # (TypeError for a data type the library does not know)
    if alpha == 1:
        return
    E = engine or default_engine()
    st = StreamHandle(stream)
    d = matrix.desc()   # (only the data area is written)
    if matrix.dtype.is_complex:
        rc = E.L.dbcsr_amd_bcsr_scale_window_z(E.h, C.byref(d), _z(alpha), -1, -1, -1, -1, st.ptr)
    else:
        rc = E.L.dbcsr_amd_bcsr_scale_window(E.h, matrix.dtype_code, C.byref(d), float(alpha), -1, -1, -1, -1, st.ptr)
    if rc != 0:
        raise RuntimeError("dbcsr_amd_bcsr_scale_window failed (%d)" % rc)


def dbcsr_add_on_diag(matrix, alpha, engine=None, stream=None):
    """A <- A + alpha*I (dbcsr_add_on_diag): alpha is added to every diagonal element; diagonal blocks A lacks are created (= alpha*I).
    Square matrices with row_blk_size == col_blk_size, symmetry 'N', 'S' or 'H'.  With every diagonal block present nothing but the
    data area is written (A keeps its index and its index_stamp()); otherwise the missing blocks come in through dbcsr_add."""
    sym = _check_symmetry("dbcsr_add_on_diag", matrix)
    if sym in ("A", "K"):
        raise ValueError("dbcsr_add_on_diag: not defined for an antisymmetric / antihermitian matrix (symmetry %r)" % sym)
    _check_scalar("dbcsr_add_on_diag", matrix, alpha)
    rs, cs = matrix.row_blk_size, matrix.col_blk_size
    if matrix.nblkrows != matrix.nblkcols or not (rs is cs or torch.equal(rs, cs)):
        raise ValueError("dbcsr_add_on_diag: the matrix is not square (row and column block sizes differ)")
    E = engine or default_engine()
    st = StreamHandle(stream)
    A = matrix
    dev = A.row_p.device
    n = A.nblkrows
    a = A.desc()
    row_p = torch.empty(n + 1, dtype=torch.int32, device=dev)
    col_i = torch.empty(n, dtype=torch.int32, device=dev)
    blk_p = torch.empty(n, dtype=torch.int64, device=dev)
    nb, nz = C.c_int64(), C.c_int64()
    rc = E.L.dbcsr_amd_bcsr_diag_count(E.h, C.byref(a), row_p.data_ptr(), col_i.data_ptr() if n else None, blk_p.data_ptr() if n else None,
                                       C.byref(nb), C.byref(nz), st.ptr)
    if rc != 0:
        raise RuntimeError("dbcsr_amd_bcsr_diag_count failed (%d)" % rc)
    rc = E.L.dbcsr_amd_bcsr_diag_shift(E.h, A.dtype_code, C.byref(a), _z(alpha), st.ptr)
    if rc != 0:
        raise RuntimeError("dbcsr_amd_bcsr_diag_shift failed (%d)" % rc)
    if nb.value == 0:
        return
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        D = DbcsrMatrix(A.row_blk_size, A.col_blk_size, row_p, col_i[:nb.value].contiguous(), blk_p[:nb.value].contiguous(),
                        torch.empty(nz.value, dtype=A.dtype, device=dev), A.name, symmetry=sym)
    d = D.desc(out=True)
    rc = E.L.dbcsr_amd_bcsr_diag_fill(E.h, A.dtype_code, _z(alpha), C.byref(d), st.ptr)
    if rc != 0:
        raise RuntimeError("dbcsr_amd_bcsr_diag_fill failed (%d)" % rc)
    dbcsr_add(A, D, 1.0, 1.0, engine=E, stream=stream)


def dbcsr_trace(matrix, engine=None, stream=None):
    """Sum of the diagonal elements of the diagonal blocks present (dbcsr_trace); a complex number for complex data."""
    _check_symmetry("dbcsr_trace", matrix)
    if matrix.nblkrows != matrix.nblkcols:
        raise ValueError("dbcsr_trace: the matrix is not square")
    E = engine or default_engine()
    st = StreamHandle(stream)
    out = (C.c_double * 2)()
    d = matrix.desc()
    rc = E.L.dbcsr_amd_bcsr_trace(E.h, matrix.dtype_code, C.byref(d), out, st.ptr)
    if rc != 0:
        raise RuntimeError("dbcsr_amd_bcsr_trace failed (%d)" % rc)
    return complex(out[0], out[1]) if matrix.dtype.is_complex else out[0]


def dbcsr_dot(matrix_a, matrix_b, engine=None, stream=None):
    """sum a_ij * b_ij over the blocks both matrices store = trace(A^T B) (dbcsr_dot).  Symmetric ('S') matrices: blocks off the
    diagonal count twice.  Real data only: the reference's conjugation convention for complex data could not be checked against its
    sources, so the complex dot is not offered (NotImplementedError) rather than guessed."""
    sym = _check_pair("dbcsr_dot", matrix_a, matrix_b)
    if matrix_a.dtype.is_complex:
        raise NotImplementedError("dbcsr_dot: complex data")
    if sym not in ("N", "S"):
        raise ValueError("dbcsr_dot: symmetry %r (the dot is offered for 'N' and 'S')" % sym)
    E = engine or default_engine()
    st = StreamHandle(stream)
    out = (C.c_double * 2)()
    a, b = matrix_a.desc(), matrix_b.desc()
    rc = E.L.dbcsr_amd_bcsr_dot(E.h, matrix_a.dtype_code, C.byref(a), C.byref(b), 1 if sym == "S" else 0, out, st.ptr)
    if rc != 0:
        raise RuntimeError("dbcsr_amd_bcsr_dot failed (%d)" % rc)
    return out[0]


def dbcsr_frobenius_norm(matrix, engine=None, stream=None):
    """sqrt(sum |x|^2) (dbcsr_frobenius_norm); with symmetry 'S', 'A', 'H', 'K' blocks off the diagonal count twice."""
    sym = _check_symmetry("dbcsr_frobenius_norm", matrix)
    E = engine or default_engine()
    st = StreamHandle(stream)
    out = (C.c_double * 2)()
    d = matrix.desc()
    rc = E.L.dbcsr_amd_bcsr_norm2(E.h, matrix.dtype_code, C.byref(d), 0 if sym == "N" else 1, out, st.ptr)
    if rc != 0:
        raise RuntimeError("dbcsr_amd_bcsr_norm2 failed (%d)" % rc)
    return math.sqrt(out[0])


# ---- norms and vectors --------------------------------------------------------------------------------------------------------------------------
_FULL_SIZES = {}   # (serial, version) of a block-size tensor -> its sum: the length of a vector over the full rows / columns


def _full_size(sizes):
    key = (_serial(sizes), sizes._version)
    n = _FULL_SIZES.get(key)
    if n is None:
        if len(_FULL_SIZES) > 256:
            _FULL_SIZES.clear()
        n = _FULL_SIZES[key] = int(sizes.sum().item()) if sizes.numel() else 0
    return n


def _check_square(name, matrix):
    rs, cs = matrix.row_blk_size, matrix.col_blk_size
    if matrix.nblkrows != matrix.nblkcols or not (rs is cs or torch.equal(rs, cs)):
        raise ValueError("%s: the matrix is not square (row and column block sizes differ)" % name)


def _check_vector(name, matrix, vec, n, dtype=None):
    """a device vector of n elements of the matrix' data type (or `dtype`), contiguous: checked before any call of the library"""
    if not isinstance(vec, torch.Tensor):
        raise TypeError("%s: the vector must be a torch tensor" % name)
    if vec.dtype != (dtype or matrix.dtype):
        raise TypeError("%s: the vector has data type %r, expected %r" % (name, vec.dtype, dtype or matrix.dtype))
    if vec.device != matrix.row_p.device:
        raise ValueError("%s: the vector is not on the matrix' device" % name)
    if vec.dim() != 1 or vec.numel() != n or not vec.is_contiguous():
        raise ValueError("%s: the vector must be contiguous with %d elements" % (name, n))


def dbcsr_maxabs_norm(matrix, engine=None, stream=None):
    """max |x| over the stored blocks (dbcsr_maxabs_norm); the modulus for complex data."""
    _check_symmetry("dbcsr_maxabs_norm", matrix)
    E = engine or default_engine()
    st = StreamHandle(stream)
    out = (C.c_double * 2)()
    d = matrix.desc()
    rc = E.L.dbcsr_amd_bcsr_maxabs(E.h, matrix.dtype_code, C.byref(d), out, st.ptr)
    if rc != 0:
        raise RuntimeError("dbcsr_amd_bcsr_maxabs failed (%d)" % rc)
    return out[0]


def dbcsr_gershgorin_norm(matrix, engine=None, stream=None):
    """max over the full rows of sum_j |a_ij| (dbcsr_gershgorin_norm).  With symmetry 'S', 'A', 'H', 'K' a stored block off the diagonal
    also adds its column sums to the rows of its twin: the value is that of the desymmetrized matrix."""
    sym = _check_symmetry("dbcsr_gershgorin_norm", matrix)
    if sym != "N":
        _check_square("dbcsr_gershgorin_norm", matrix)
    E = engine or default_engine()
    st = StreamHandle(stream)
    out = (C.c_double * 2)()
    d = matrix.desc()
    rc = E.L.dbcsr_amd_bcsr_gershgorin(E.h, matrix.dtype_code, C.byref(d), 0 if sym == "N" else 1, out, st.ptr)
    if rc != 0:
        raise RuntimeError("dbcsr_amd_bcsr_gershgorin failed (%d)" % rc)
    return out[0]


def dbcsr_norm(matrix, which_norm, norm_vector=None, engine=None, stream=None):
    """dbcsr_norm: which_norm = dbcsr_norm_frobenius, dbcsr_norm_maxabsnorm or dbcsr_norm_gershgorin returns the scalar;
    dbcsr_norm_column returns a float64 device tensor with sqrt(sum_i |a_ij|^2) per full column (norm_vector, when given, is filled and
    returned).  The column norms are offered for symmetry 'N' only (NotImplementedError otherwise: how the reference treats the twin blocks
    there could not be checked, and it is not guessed)."""
    if which_norm == dbcsr_norm_frobenius:
        return dbcsr_frobenius_norm(matrix, engine=engine, stream=stream)
    if which_norm == dbcsr_norm_maxabsnorm:
        return dbcsr_maxabs_norm(matrix, engine=engine, stream=stream)
    if which_norm == dbcsr_norm_gershgorin:
        return dbcsr_gershgorin_norm(matrix, engine=engine, stream=stream)
    if which_norm != dbcsr_norm_column:
        raise ValueError("dbcsr_norm: unknown which_norm %r" % (which_norm,))
    sym = _check_symmetry("dbcsr_norm", matrix)
    if sym != "N":
        raise NotImplementedError("dbcsr_norm: column norms of a matrix with symmetry %r" % sym)
    matrix.dtype_code
    n = _full_size(matrix.col_blk_size)
    if norm_vector is not None:
        _check_vector("dbcsr_norm", matrix, norm_vector, n, torch.float64)
    E = engine or default_engine()
    st = StreamHandle(stream)
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        out = norm_vector if norm_vector is not None else torch.empty(n, dtype=torch.float64, device=matrix.row_p.device)
        d = matrix.desc()
        rc = E.L.dbcsr_amd_bcsr_col_sums(E.h, matrix.dtype_code, C.byref(d), 1, 0, out.data_ptr() if n else None, n, st.ptr)
        if rc != 0:
            raise RuntimeError("dbcsr_amd_bcsr_col_sums failed (%d)" % rc)
        torch.sqrt(out, out=out)   # (one root per column of the vector the kernels made)
    return out


def dbcsr_get_diag(matrix, engine=None, stream=None):
    """The diagonal as a device tensor of the matrix' data type and full-row length (dbcsr_get_diag): the diagonal elements of the diagonal
    blocks present, zero where a block row has no diagonal block.  Any symmetry: what is stored is read."""
    _check_symmetry("dbcsr_get_diag", matrix)
    _check_square("dbcsr_get_diag", matrix)
    matrix.dtype_code
    n = _full_size(matrix.row_blk_size)
    E = engine or default_engine()
    st = StreamHandle(stream)
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        out = torch.empty(n, dtype=matrix.dtype, device=matrix.row_p.device)
    d = matrix.desc()
    rc = E.L.dbcsr_amd_bcsr_get_diag(E.h, matrix.dtype_code, C.byref(d), out.data_ptr() if n else None, n, st.ptr)
    if rc != 0:
        raise RuntimeError("dbcsr_amd_bcsr_get_diag failed (%d)" % rc)
    return out


def dbcsr_set_diag(matrix, diag, engine=None, stream=None):
    """a_ii <- diag[i] (dbcsr_set_diag), in place.  Only the diagonal blocks PRESENT are written: no block is created and nothing else is
    touched (the matrix keeps its index and its index_stamp()); dbcsr_add_on_diag(matrix, 0.0) creates the missing diagonal blocks first.
    Square matrices with symmetry 'N', 'S' or 'H'; diag: a device tensor of the matrix' data type and full-row length."""
    sym = _check_symmetry("dbcsr_set_diag", matrix)
    if sym in ("A", "K"):
        raise ValueError("dbcsr_set_diag: not defined for an antisymmetric / antihermitian matrix (symmetry %r)" % sym)
    _check_square("dbcsr_set_diag", matrix)
    matrix.dtype_code
    n = _full_size(matrix.row_blk_size)
    _check_vector("dbcsr_set_diag", matrix, diag, n)
    E = engine or default_engine()
    st = StreamHandle(stream)
    d = matrix.desc()   # (only the data area is written)
    rc = E.L.dbcsr_amd_bcsr_set_diag(E.h, matrix.dtype_code, C.byref(d), diag.data_ptr() if n else None, n, st.ptr)
    if rc != 0:
        raise RuntimeError("dbcsr_amd_bcsr_set_diag failed (%d)" % rc)


def dbcsr_scale_by_vector(matrix, alpha, side, engine=None, stream=None):
    """A <- A * diag(alpha) (side = "right": column j times alpha[j]) or diag(alpha) * A (side = "left": row i times alpha[i]), in place
    (dbcsr_scale_by_vector).  alpha: a device tensor of the matrix' data type with one element per full column / row.  Symmetry 'N' only:
    a stored triangle scaled on one side is not a matrix with that symmetry."""
    if side not in ("left", "right"):
        raise ValueError("dbcsr_scale_by_vector: side must be 'left' or 'right', got %r" % (side,))
    sym = _check_symmetry("dbcsr_scale_by_vector", matrix)
    if sym != "N":
        raise ValueError("dbcsr_scale_by_vector: not defined for a matrix with symmetry %r" % sym)
    matrix.dtype_code
    n = _full_size(matrix.col_blk_size if side == "right" else matrix.row_blk_size)
    _check_vector("dbcsr_scale_by_vector", matrix, alpha, n)
    E = engine or default_engine()
    st = StreamHandle(stream)
    d = matrix.desc()   # (only the data area is written)
    rc = E.L.dbcsr_amd_bcsr_scale_by_vector(E.h, matrix.dtype_code, C.byref(d), alpha.data_ptr() if n else None, n, 1 if side == "right" else 0, st.ptr)
    if rc != 0:
        raise RuntimeError("dbcsr_amd_bcsr_scale_by_vector failed (%d)" % rc)


def dbcsr_matvec(matrix, vec_in, vec_out=None, alpha=1.0, beta=0.0, trans="N", engine=None, stream=None):
    """vec_out <- alpha * op(A) * vec_in + beta * vec_out with dense device vectors of the matrix' data type: what a Lanczos, Arnoldi or power step, a
    residual or the application of a preconditioner needs.  NOT a mirror of a routine of the reference: the reference keeps its vectors as one-column
    DBCSR matrices (dbcsr_matrix_colvec_multiply), and its signature could not be checked against its sources -- so this name does not claim to be it.
    trans: 'N', 'T' or 'C' (conjugate transpose; real data: 'T').  vec_in has one element per full column of op(A), vec_out one per full row, in the
    order of the dense matrix (as dbcsr_get_diag).  With symmetry 'S' / 'A' (real data) or 'H' / 'K' (complex data) the matrix is a stored triangle
    with a square structure and the product is that of the desymmetrized matrix.  beta == 0: vec_out is not read (a NaN in it does not reach the
    result); alpha == 0: the matrix and vec_in are not read.  vec_out=None (then beta must be 0) allocates the result on the matrix' device and stream.
    The vectors must not overlap.  Asynchronous on the stream; returns vec_out."""
    sym = _check_symmetry("dbcsr_matvec", matrix)
    if trans not in ("N", "T", "C"):
        raise ValueError("dbcsr_matvec: trans must be 'N', 'T' or 'C', got %r" % (trans,))
    matrix.dtype_code
    kind = -1
    if sym != "N":
        kind = matrix.symmetry_kind()
        _check_square("dbcsr_matvec", matrix)
    _check_scalar("dbcsr_matvec", matrix, alpha, beta)
    n_rows, n_cols = _full_size(matrix.row_blk_size), _full_size(matrix.col_blk_size)
    n_x, n_y = (n_cols, n_rows) if trans == "N" else (n_rows, n_cols)
    _check_vector("dbcsr_matvec", matrix, vec_in, n_x)
    if vec_out is None:
        if beta != 0:
            raise ValueError("dbcsr_matvec: beta != 0 needs a vec_out")
    else:
        _check_vector("dbcsr_matvec", matrix, vec_out, n_y)
        size = vec_in.element_size()
        x0, y0 = vec_in.data_ptr(), vec_out.data_ptr()
        if n_x and n_y and x0 < y0 + size * n_y and y0 < x0 + size * n_x:
            raise ValueError("dbcsr_matvec: vec_in and vec_out overlap")
    E = engine or default_engine()
    st = StreamHandle(stream)
    if vec_out is None:
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            vec_out = torch.empty(n_y, dtype=matrix.dtype, device=matrix.row_p.device)
    d = matrix.desc()
    rc = E.L.dbcsr_amd_bcsr_matvec(E.h, matrix.dtype_code, trans.encode(), _z(alpha), C.byref(d), kind, vec_in.data_ptr() if n_x else None, n_x,
                                   _z(beta), vec_out.data_ptr() if n_y else None, n_y, st.ptr)
    if rc != 0:
        raise RuntimeError("dbcsr_amd_bcsr_matvec failed (%d)" % rc)
    return vec_out


def _check_vectors(name, matrix, vecs, n):
    """a device matrix of n rows, one right-hand side per column, of the matrix' data type, its rows contiguous: checked before any call of the library"""
    if not isinstance(vecs, torch.Tensor):
        raise TypeError("%s: the vectors must be a torch tensor" % name)
    if vecs.dtype != matrix.dtype:
        raise TypeError("%s: the vectors have data type %r, expected %r" % (name, vecs.dtype, matrix.dtype))
    if vecs.device != matrix.row_p.device:
        raise ValueError("%s: the vectors are not on the matrix' device" % name)
    if vecs.dim() != 2 or vecs.shape[0] != n:
        raise ValueError("%s: the vectors must be a 2-D tensor with %d rows, one right-hand side per column" % (name, n))
    nrhs = vecs.shape[1]
    if nrhs > 1 and vecs.stride(1) != 1:
        raise ValueError("%s: the vectors must have stride(1) == 1 (the right-hand sides of one row are consecutive)" % name)
    if n > 1 and vecs.stride(0) < nrhs:
        raise ValueError("%s: the vectors must have stride(0) >= nrhs" % name)
    return nrhs, (vecs.stride(0) if n > 1 else nrhs)


def dbcsr_multivec(matrix, vecs_in, vecs_out=None, alpha=1.0, beta=0.0, trans="N", engine=None, stream=None):
    """vecs_out <- alpha * op(A) * vecs_in + beta * vecs_out with nrhs right-hand sides at once: dbcsr_matvec for the columns of a dense device matrix,
    with A read once for all of them -- what block Lanczos / LOBPCG, a Chebyshev filter on a block of vectors, subspace iteration or the product of a
    sparse matrix with a tall-and-skinny coefficient matrix need.  vecs_in is (n_x, nrhs), vecs_out (n_y, nrhs): 2-D device tensors of the matrix'
    data type with stride(1) == 1 and stride(0) >= nrhs -- a contiguous tensor, or a column slice of a wider one.  trans, the symmetries, alpha == 0
    and beta == 0 are dbcsr_matvec's, per column; so are the checks.  The padding columns of a slice are never written.  vecs_out=None (then beta
    must be 0) allocates (n_y, nrhs) on the matrix' device and stream.  One column is served by the same kernels, not by dbcsr_matvec.  The two
    tensors must not overlap.  For a dense operand of hundreds of columns, or one stored column by column, see dbcsr_multiply_dense (matrix cores, no
    partial sums): on the benchmark's 23 x 23 operand this function is the faster one at 16 and 32 columns (0.57 and 0.79 of its time) and the
    slower one from 48 columns on (1.06 of its time at 48, 1.22 at 64, 1.57 at 1024; profiles/multiply_dense.txt).  Asynchronous on the stream; returns vecs_out."""
    sym = _check_symmetry("dbcsr_multivec", matrix)
    if trans not in ("N", "T", "C"):
        raise ValueError("dbcsr_multivec: trans must be 'N', 'T' or 'C', got %r" % (trans,))
    matrix.dtype_code
    kind = -1
    if sym != "N":
        kind = matrix.symmetry_kind()
        _check_square("dbcsr_multivec", matrix)
    _check_scalar("dbcsr_multivec", matrix, alpha, beta)
    n_rows, n_cols = _full_size(matrix.row_blk_size), _full_size(matrix.col_blk_size)
    n_x, n_y = (n_cols, n_rows) if trans == "N" else (n_rows, n_cols)
    nrhs, ldx = _check_vectors("dbcsr_multivec", matrix, vecs_in, n_x)
    if vecs_out is None:
        if beta != 0:
            raise ValueError("dbcsr_multivec: beta != 0 needs a vecs_out")
        ldy = nrhs
    else:
        nout, ldy = _check_vectors("dbcsr_multivec", matrix, vecs_out, n_y)
        if nout != nrhs:
            raise ValueError("dbcsr_multivec: vecs_in has %d right-hand sides, vecs_out %d" % (nrhs, nout))
        size = vecs_in.element_size()
        x0, y0 = vecs_in.data_ptr(), vecs_out.data_ptr()
        if nrhs and n_x and n_y and x0 < y0 + size * ((n_y - 1) * ldy + nrhs) and y0 < x0 + size * ((n_x - 1) * ldx + nrhs):
            raise ValueError("dbcsr_multivec: vecs_in and vecs_out overlap")
    E = engine or default_engine()
    st = StreamHandle(stream)
    if vecs_out is None:
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            vecs_out = torch.empty((n_y, nrhs), dtype=matrix.dtype, device=matrix.row_p.device)
    d = matrix.desc()
    rc = E.L.dbcsr_amd_bcsr_multivec(E.h, matrix.dtype_code, trans.encode(), _z(alpha), C.byref(d), kind, nrhs, vecs_in.data_ptr() if n_x and nrhs else None,
                                     n_x, ldx, _z(beta), vecs_out.data_ptr() if n_y and nrhs else None, n_y, ldy, st.ptr)
    if rc != 0:
        raise RuntimeError("dbcsr_amd_bcsr_multivec failed (%d)" % rc)
    return vecs_out


def _overlaps(t, n, ld, nrhs, data):
    """the element range of an (n, nrhs) tensor with row stride ld intersects the range of a data area"""
    if not n or not nrhs or not data.numel():
        return False
    t0, d0 = t.data_ptr(), data.data_ptr()
    return t0 < d0 + data.numel() * data.element_size() and d0 < t0 + t.element_size() * ((n - 1) * ld + nrhs)


def dbcsr_rank_update(matrix, vecs_x, vecs_y=None, alpha=1.0, beta=1.0, trans="T", engine=None, stream=None):
    """A_IJ <- beta * A_IJ + alpha * X_I * op(Y_J) for every stored block (I, J), in place, and nothing else: the rank-nrhs update restricted to the pattern
    the matrix has -- the density matrix P = C C^T on the pattern of S, energy-weighted density matrices, low-rank corrections, outer products of Lanczos /
    LOBPCG blocks.  NOT a mirror of a routine of the reference: it serves the call CP2K makes as cp_dbcsr_plus_fm_fm_t with keep_sparsity, with dense
    device tensors in place of full matrices, and does not claim that name.  op is the transpose (trans "T") or the conjugate transpose ("C"; real data:
    "T").  vecs_x is (full rows, nrhs), vecs_y (full columns, nrhs): 2-D device tensors of the matrix' data type in dbcsr_multivec's layout (stride(1) == 1,
    stride(0) >= nrhs: a contiguous tensor or a column slice of a wider basis); X_I are the rows of vecs_x of block row I, Y_J the rows of vecs_y of block
    column J.  vecs_y=None: Y is X (the matrix must have equal row and column block sizes).  The pattern never changes: no index array is written,
    index_stamp() stays, a multiply with the matrix as operand afterwards reuses its plan; the holes of an unpacked matrix keep their bits.  Products and sums
    in double / complex double, alpha and beta applied in double, one rounding per element, the same bits on every call.  beta == 0: the matrix' values are
    not read; alpha == 0 or nrhs == 0: X and Y are not read and A <- beta * A in the data's own precision; alpha == 0 and beta == 1: nothing is launched.
    Symmetry 'N': any X, Y.  'S': vecs_y must be None and op the transpose; 'H': vecs_y must be None, trans "C", alpha and beta real -- the stored triangle
    is then updated block by block, which is the update of the full symmetric / hermitian matrix.  'A' and 'K': ValueError.  X and Y are only read: they
    may be the same tensor or overlap each other, but neither may overlap matrix.data (ValueError).  Asynchronous on the stream; returns None."""
    name = "dbcsr_rank_update"
    sym = _check_symmetry(name, matrix)
    if trans not in ("T", "C"):
        raise ValueError("%s: trans must be 'T' or 'C', got %r" % (name, trans))
    matrix.dtype_code
    if not matrix.dtype.is_complex:
        trans = "T"   # (real data: the conjugate transpose is the transpose)
    _check_scalar(name, matrix, alpha, beta)
    if sym != "N":
        if sym in ("A", "K"):
            raise ValueError("%s: not defined for an antisymmetric / antihermitian matrix (symmetry %r)" % (name, sym))
        matrix.symmetry_kind()   # (which symmetries go with which data)
        _check_square(name, matrix)
        if vecs_y is not None:
            raise ValueError("%s: a matrix with symmetry %r takes X alone (vecs_y=None): X op(Y) would not keep the symmetry" % (name, sym))
        if sym == "S" and trans != "T":
            raise ValueError("%s: a symmetric matrix takes trans 'T' (X X^H is not symmetric)" % name)
        if sym == "H" and (trans != "C" or complex(alpha).imag != 0 or complex(beta).imag != 0):
            raise ValueError("%s: a hermitian matrix takes trans 'C' and real alpha and beta" % name)
    n_rows, n_cols = _full_size(matrix.row_blk_size), _full_size(matrix.col_blk_size)
    nrhs, ldx = _check_vectors(name, matrix, vecs_x, n_rows)
    if vecs_y is None:
        _check_square(name, matrix)
        vecs_y, ldy = vecs_x, ldx
    else:
        ny, ldy = _check_vectors(name, matrix, vecs_y, n_cols)
        if ny != nrhs:
            raise ValueError("%s: vecs_x has %d columns, vecs_y %d" % (name, nrhs, ny))
    if _overlaps(vecs_x, n_rows, ldx, nrhs, matrix.data) or _overlaps(vecs_y, n_cols, ldy, nrhs, matrix.data):
        raise ValueError("%s: vecs_x / vecs_y overlap the matrix' data area" % name)
    E = engine or default_engine()
    st = StreamHandle(stream)
    d = matrix.desc()   # (only the data area is written)
    rc = E.L.dbcsr_amd_bcsr_rank_update(E.h, matrix.dtype_code, trans.encode(), _z(alpha), nrhs, vecs_x.data_ptr() if n_rows and nrhs else None, n_rows, ldx,
                                        vecs_y.data_ptr() if n_cols and nrhs else None, n_cols, ldy, _z(beta), C.byref(d), st.ptr)
    if rc != 0:
        raise RuntimeError("dbcsr_amd_bcsr_rank_update failed (%d)" % rc)


# ---- matrix times a dense matrix ---------------------------------------------------------------------------------------------------------------------
def _dense_layouts(shape, strides):
    """(ld row by row or None, ld column by column or None) of a 2-D tensor of this shape and these strides: row by row is stride(1) == 1 and
    stride(0) = ld >= ncol, column by column stride(0) == 1 and stride(1) = ld >= n.  The stride of a dimension of one element, or of none, says nothing:
    a tensor with one row or one column fits both.  Plain integers in and out: no device is needed."""
    n, ncol = shape
    s0, s1 = strides
    by_row = by_col = None
    if (ncol <= 1 or s1 == 1) and (n <= 1 or s0 >= max(ncol, 1)):
        by_row = s0 if n > 1 else max(ncol, 1)
    if (n <= 1 or s0 == 1) and (ncol <= 1 or s1 >= max(n, 1)):
        by_col = s1 if ncol > 1 else max(n, 1)
    return by_row, by_col


def _check_dense_operand(name, matrix, what, t, n):
    """a 2-D device tensor of n rows of the matrix' data type in one of the two layouts: checked before any call of the library"""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s: %s must be a torch tensor" % (name, what))
    if t.dtype != matrix.dtype:
        raise TypeError("%s: %s has data type %r, expected %r" % (name, what, t.dtype, matrix.dtype))
    if t.device != matrix.row_p.device:
        raise ValueError("%s: %s is not on the matrix' device" % (name, what))
    if t.dim() != 2 or t.shape[0] != n:
        raise ValueError("%s: %s must be a 2-D tensor with %d rows" % (name, what, n))
    layouts = _dense_layouts(tuple(t.shape), t.stride())
    if layouts == (None, None):
        raise ValueError("%s: %s must be row by row (stride(1) == 1, stride(0) >= ncol) or column by column (stride(0) == 1, stride(1) >= n), got "
                         "strides %r" % (name, what, tuple(t.stride())))
    return layouts


def dbcsr_multiply_dense(matrix, dense_in, dense_out=None, alpha=1.0, beta=0.0, trans="N", engine=None, stream=None):
    """dense_out <- alpha * op(A) * dense_in + beta * dense_out with a dense operand of many columns, on the matrix cores: the sparse matrix times the
    coefficient matrix of every SCF step (H C and S C in OT and in the diagonalisation).  NOT a mirror of a routine of the reference: it serves the
    call CP2K makes as cp_dbcsr_sm_fm_multiply, with dense device tensors in place of full matrices, and does not claim that name.  It is the forward
    direction of dbcsr_rank_update and runs on the same v_mfma_f64_16x16x4_f64 core.
    dense_in is (n_x, ncol), dense_out (n_y, ncol): 2-D device tensors of the matrix' data type, BOTH in the same layout -- row by row (stride(1) == 1,
    stride(0) = ld >= ncol: dbcsr_multivec's layout, a contiguous tensor or a column slice of a wider basis) or column by column (stride(0) == 1,
    stride(1) = ld >= n: a Fortran full matrix, t.T of a contiguous (ncol, n) tensor, or a window of leading dimension ld).  A tensor with one row or
    one column fits both and takes the layout of the other tensor (row by row when both do).  Mixed layouts: ValueError.
    trans is 'N', 'T' or 'C' (conjugate transpose; real data: 'T'); n_x is the full column count of op(A), n_y its full row count.  With symmetry
    'S' / 'A' (real data) or 'H' / 'K' (complex data) the matrix is a stored triangle with a square structure and the product is that of the
    desymmetrized matrix.  beta == 0: dense_out is not read (a NaN in it does not reach the result); alpha == 0: the matrix and dense_in are not read and
    dense_out <- beta * dense_out in the data's own precision.  dense_out=None (then beta must be 0) allocates the result in dense_in's layout on the
    matrix' device and stream.  The two tensors must not overlap (ValueError).  float64, float32 and complex128: products and sums in double / complex
    double, alpha and beta applied in double, one rounding per element.  Every element of the (n_y, ncol) window is written exactly once -- the rows
    of a block row that stores nothing become beta * dense_out, +0.0 for beta == 0 -- and nothing outside it: padding columns or rows of a window keep
    their bits.  One workgroup owns its piece of the result from the first block to the end: no atomics, no partial sums, the same bits on every call;
    within one layout the bits of a column depend neither on its position nor on how many columns come with it.  Rows and columns outside a block are
    never loaded: an Inf or NaN in row r of dense_in reaches only the rows of the result whose row of op(A) stores an element in column r.  No index
    array is written and no saved plan is touched.  Which width is whose (profiles/multiply_dense.txt, the benchmark's 23 x 23 operand, float64): at 16
    and 32 columns dbcsr_multivec is faster (this function takes 1.75 and 1.27 of its time), from 48 columns on this function is (0.94 of its time
    at 48, 0.82 at 64, 0.69 at 256, 0.64 at 1024; column by column from 64 on: 0.95 / 0.76 / 0.74 of dbcsr_multivec with the two transposing copies).
    It LOSES to dbcsr_create_from_dense -> dbcsr_multiply -> dbcsr_to_dense at every width measured (1.02 to 1.79 of that route's time) where the
    dense operand fits as a block-sparse matrix.  Every check comes before any call of the library.  Asynchronous on the stream; returns dense_out."""
    name = "dbcsr_multiply_dense"
    sym = _check_symmetry(name, matrix)
    if trans not in ("N", "T", "C"):
        raise ValueError("%s: trans must be 'N', 'T' or 'C', got %r" % (name, trans))
    matrix.dtype_code
    kind = -1
    if sym != "N":
        kind = matrix.symmetry_kind()
        _check_square(name, matrix)
    _check_scalar(name, matrix, alpha, beta)
    n_rows, n_cols = _full_size(matrix.row_blk_size), _full_size(matrix.col_blk_size)
    n_x, n_y = (n_cols, n_rows) if trans == "N" else (n_rows, n_cols)
    x_row, x_col = _check_dense_operand(name, matrix, "dense_in", dense_in, n_x)
    ncol = dense_in.shape[1]
    if dense_out is None:
        if beta != 0:
            raise ValueError("%s: beta != 0 needs a dense_out" % name)
        layout = 0 if x_row is not None else 1
        ldx = x_row if layout == 0 else x_col
        ldy = max(ncol, 1) if layout == 0 else max(n_y, 1)
    else:
        y_row, y_col = _check_dense_operand(name, matrix, "dense_out", dense_out, n_y)
        if dense_out.shape[1] != ncol:
            raise ValueError("%s: dense_in has %d columns, dense_out %d" % (name, ncol, dense_out.shape[1]))
        if x_row is not None and y_row is not None:
            layout, ldx, ldy = 0, x_row, y_row
        elif x_col is not None and y_col is not None:
            layout, ldx, ldy = 1, x_col, y_col
        else:
            raise ValueError("%s: dense_in and dense_out must be in the same layout (strides %r and %r)" %
                             (name, tuple(dense_in.stride()), tuple(dense_out.stride())))
        size = dense_in.element_size()
        ex = (n_x - 1) * ldx + ncol if layout == 0 else (ncol - 1) * ldx + n_x
        ey = (n_y - 1) * ldy + ncol if layout == 0 else (ncol - 1) * ldy + n_y
        x0, y0 = dense_in.data_ptr(), dense_out.data_ptr()
        if ncol and n_x and n_y and x0 < y0 + size * ey and y0 < x0 + size * ex:
            raise ValueError("%s: dense_in and dense_out overlap" % name)
    E = engine or default_engine()
    st = StreamHandle(stream)
    if dense_out is None:
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            if layout == 0:
                dense_out = torch.empty((n_y, ncol), dtype=matrix.dtype, device=matrix.row_p.device)
            else:
                dense_out = torch.empty((ncol, n_y), dtype=matrix.dtype, device=matrix.row_p.device).t()
    d = matrix.desc()
    rc = E.L.dbcsr_amd_bcsr_multiply_dense(E.h, matrix.dtype_code, trans.encode(), _z(alpha), C.byref(d), kind, ncol,
                                           dense_in.data_ptr() if n_x and ncol else None, n_x, ldx, _z(beta),
                                           dense_out.data_ptr() if n_y and ncol else None, n_y, ldy, layout, st.ptr)
    if rc != 0:
        raise RuntimeError("dbcsr_amd_bcsr_multiply_dense failed (%d)" % rc)
    return dense_out


# ---- block diagonal --------------------------------------------------------------------------------------------------------------------------------
BLOCK_INVERSE_MAX_DIM = 96   # the largest diagonal block dbcsr_invert_block_diag takes (include/dbcsr_amd_mm.h)
_MAX_SIZES = {}   # (serial, version) of a block-size tensor -> its largest entry, as _FULL_SIZES holds the sums


def _max_size(sizes):
    key = (_serial(sizes), sizes._version)
    n = _MAX_SIZES.get(key)
    if n is None:
        if len(_MAX_SIZES) > 256:
            _MAX_SIZES.clear()
        n = _MAX_SIZES[key] = int(sizes.max().item()) if sizes.numel() else 0
    return n


def dbcsr_get_block_diag(matrix, engine=None, stream=None):
    """A new matrix of the diagonal blocks the matrix stores (dbcsr_get_block_diag(matrix, diag)): the matrix' block sizes, data type, name and symmetry;
    exactly its stored diagonal blocks, in block-row order and packed, as bit-for-bit copies; a block row without a diagonal block has none in the result.
    Any symmetry: a diagonal block is stored in full and taken as it is.  Square block structure (nblkrows == nblkcols and equal row / column block sizes,
    else ValueError).  The matrix is only read: it keeps its index_stamp() and no saved plan is invalidated.  Synchronises once (the size of the result).
    dbcsr_invert_block_diag of the result is the initial guess X0 = blockdiag(S)^-1 of a Hotelling / Newton-Schulz inverse, and
    dbcsr_multivec(that, R) the block-Jacobi preconditioner Y <- blockdiag(A)^-1 R."""
    name = "dbcsr_get_block_diag"
    sym = _check_symmetry(name, matrix)
    _check_square(name, matrix)
    matrix.dtype_code
    E = engine or default_engine()
    st = StreamHandle(stream)
    A = matrix
    dev = A.row_p.device
    n = A.nblkrows
    a = A.desc()
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        row_p = torch.empty(n + 1, dtype=torch.int32, device=dev)
        col_i = torch.empty(n, dtype=torch.int32, device=dev)
        blk_p = torch.empty(n, dtype=torch.int64, device=dev)
    nb, nz, md = C.c_int64(), C.c_int64(), C.c_int32()
    rc = E.L.dbcsr_amd_bcsr_block_diag_count(E.h, C.byref(a), row_p.data_ptr(), col_i.data_ptr() if n else None, blk_p.data_ptr() if n else None,
                                             C.byref(nb), C.byref(nz), C.byref(md), st.ptr)
    if rc != 0:
        raise RuntimeError("dbcsr_amd_bcsr_block_diag_count failed (%d)" % rc)
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        D = DbcsrMatrix(A.row_blk_size, A.col_blk_size, row_p, col_i[:nb.value].contiguous(), blk_p[:nb.value].contiguous(),
                        torch.empty(nz.value, dtype=A.dtype, device=dev), A.name, symmetry=sym)
    d = D.desc(out=True)
    rc = E.L.dbcsr_amd_bcsr_block_diag_apply(E.h, A.dtype_code, C.byref(a), C.byref(d), st.ptr)
    if rc != 0:
        raise RuntimeError("dbcsr_amd_bcsr_block_diag_apply failed (%d)" % rc)
    return D


def dbcsr_invert_block_diag(matrix, check=True, engine=None, stream=None):
    """Every diagonal block the matrix stores <- its inverse, in place, and nothing else.  NOT a mirror of a routine of the reference: it is what CP2K does
    on the host with an iterator over the blocks and invmat (the initial guess of invert_Hotelling, the block-Jacobi preconditioners), and does not
    claim a DBCSR name.  With D = dbcsr_get_block_diag(S), dbcsr_invert_block_diag(D) makes D the initial guess X0 = blockdiag(S)^-1 of a Hotelling /
    Newton-Schulz inverse, and dbcsr_multivec(D, R) then is the block-Jacobi preconditioner Y <- blockdiag(A)^-1 R.
    Blocks off the diagonal, the holes of an unpacked matrix and everything else of the data area keep their bits; no index array is written,
    index_stamp() stays, a multiply with the matrix as operand afterwards reuses its plan.  Gauss-Jordan with partial pivoting in double / complex double
    (float32: converted on load, rounded once on store); the same bits on every call, wherever the block lies.  Symmetry 'N', 'S', 'H': the stored full
    diagonal block is inverted as a general matrix and nothing is symmetrised afterwards; 'A' / 'K': ValueError.  Square block structure, else
    ValueError; a block size above 96: NotImplementedError; every refusal comes before any call of the library.
    A singular block (a pivot column that is exactly zero, or all NaN) is not written at all and every other block is still inverted.  check=True:
    returns (n_singular, first_singular_block_row), the row -1 when there is none -- one synchronisation.  check=False: returns None and nothing
    synchronises (the first call for a block-size tensor synchronises once to learn the largest block size)."""
    name = "dbcsr_invert_block_diag"
    sym = _check_symmetry(name, matrix)
    if sym in ("A", "K"):
        raise ValueError("%s: not defined for an antisymmetric / antihermitian matrix (symmetry %r)" % (name, sym))
    _check_square(name, matrix)
    matrix.dtype_code
    max_dim = _max_size(matrix.row_blk_size)
    if max_dim > BLOCK_INVERSE_MAX_DIM:
        raise NotImplementedError("%s: a block of %d (diagonal blocks of up to %d are inverted)" % (name, max_dim, BLOCK_INVERSE_MAX_DIM))
    E = engine or default_engine()
    st = StreamHandle(stream)
    d = matrix.desc()   # (only the data area is written)
    info = (C.c_int64 * 3)() if check else None
    rc = E.L.dbcsr_amd_bcsr_block_diag_invert(E.h, matrix.dtype_code, C.byref(d), max_dim, info, st.ptr)
    if rc != 0:
        raise RuntimeError("dbcsr_amd_bcsr_block_diag_invert failed (%d)" % rc)
    return (int(info[0]), int(info[1])) if check else None


def _data_overlap(a, b):
    """the data areas of two matrices intersect (the same tensor, or two views of one allocation)"""
    if not a.numel() or not b.numel():
        return False
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


def _same_blk_sizes(a, b):
    return a is b or (a.numel() == b.numel() and torch.equal(a, b))


_BLOCK_SCALE_DAGGER = {"N": "C", "C": "N", "T": "J"}   # op' = op followed by the conjugate transpose ('J': the conjugate alone)


def dbcsr_scale_by_block_diag(matrix, diag, side, trans="N", alpha=1.0, engine=None, stream=None):
    """The block analogue of dbcsr_scale_by_vector: every stored block of `matrix` is multiplied by a diagonal block of `diag`, in place, and nothing else.
        side="left":   A_IJ <- alpha * op(D_I) * A_IJ                 (the block-Jacobi preconditioned operator D^-1 A, the first Newton-Schulz product X0 S)
        side="right":  A_IJ <- alpha * A_IJ * op(D_J)
        side="both":   A_IJ <- alpha * op(D_I) * A_IJ * op(D_J)^+     (a block congruence; ^+ the transpose, for complex data the conjugate transpose)
    NOT a mirror of a routine of the reference: there the product goes through dbcsr_multiply, with a symbolic phase, a second matrix and a new index for
    the result.  Here the product has the pattern of the matrix itself.  op is "N", "T" or "C" (conjugate transpose; real data: "T").  D_I is the diagonal
    block (I, I) that diag STORES: blocks of diag off the diagonal are never read -- the operand is blockdiag(diag).  A block row of diag without a stored
    diagonal block counts as a zero block, as it would in dbcsr_multiply(diag, A, beta=0, retain_sparsity): the blocks of the matrix in that block row
    (left) or block column (right) become +0.0 and their old values are not read, so a NaN there does not survive.  alpha == 0: every element of every
    stored block becomes +0.0 and neither operand's data is read.  side="both" is the left pass (with alpha) followed by the right pass with op followed
    by ^+, on the same stream: two launches, two roundings per element.
    Products and sums in double / complex double (float32 converted on load), alpha applied in double, one rounding to the data's type per element and
    pass; no atomics, the same bits on every call.  No index array is written: index_stamp() of both matrices stays and a multiply that had the matrix as
    operand before reuses its plan; the holes of an unpacked matrix and the bytes around the data area keep their bits.
    Matrix symmetry 'N': any side.  'S' (real data) and 'H': side="both" only, which keeps the symmetry ('H': real alpha) -- the stored triangle is
    transformed block by block, which is the congruence of the full matrix.  'A', 'K' and 'S' of complex data: ValueError (not yet).  diag 'N', 'S', 'H':
    its stored full diagonal blocks are taken as they are, as in dbcsr_invert_block_diag; 'A' / 'K': ValueError.  diag must have a square block structure
    whose block sizes are the matrix' row block sizes (left, both) and column block sizes (right, both), the matrix' data type (TypeError), and a data
    area that does not overlap the matrix' (ValueError; diag is matrix included).  A diagonal block dimension above 96: NotImplementedError (what can be
    inverted can be applied); the other dimension of a block of the matrix is not limited.  Every refusal comes before any call of the library.
    Asynchronous on the stream; returns None."""
    name = "dbcsr_scale_by_block_diag"
    if side not in ("left", "right", "both"):
        raise ValueError("%s: side must be 'left', 'right' or 'both', got %r" % (name, side))
    if trans not in ("N", "T", "C"):
        raise ValueError("%s: trans must be 'N', 'T' or 'C', got %r" % (name, trans))
    sym, dsym = _check_symmetry(name, matrix), _check_symmetry(name, diag)
    if matrix.dtype != diag.dtype:
        raise TypeError("%s: data types of the matrix and of diag differ" % name)
    matrix.dtype_code
    zc = matrix.dtype.is_complex
    if not zc and trans == "C":
        trans = "T"   # (real data: the conjugate transpose is the transpose)
    _check_scalar(name, matrix, alpha)
    if dsym in ("A", "K"):
        raise ValueError("%s: diag with symmetry %r (its diagonal blocks are not stored as they are)" % (name, dsym))
    if sym in ("A", "K") or (sym == "S" and zc):
        raise ValueError("%s: not yet for a matrix with symmetry %r%s" % (name, sym, " of complex data" if sym == "S" else ""))
    if sym != "N":
        matrix.symmetry_kind()   # (which symmetries go with which data)
        _check_square(name, matrix)
        if side != "both":
            raise ValueError("%s: a matrix with symmetry %r takes side='both' (one side alone does not keep the symmetry)" % (name, sym))
        if sym == "H" and complex(alpha).imag != 0:
            raise ValueError("%s: a hermitian matrix takes a real alpha" % name)
    if diag.nblkrows != diag.nblkcols or not _same_blk_sizes(diag.row_blk_size, diag.col_blk_size):
        raise ValueError("%s: diag is not square in its block structure" % name)
    if side in ("left", "both") and not _same_blk_sizes(diag.row_blk_size, matrix.row_blk_size):
        raise ValueError("%s: the block sizes of diag differ from the matrix' row block sizes" % name)
    if side in ("right", "both") and not _same_blk_sizes(diag.row_blk_size, matrix.col_blk_size):
        raise ValueError("%s: the block sizes of diag differ from the matrix' column block sizes" % name)
    if diag is matrix or _data_overlap(diag.data, matrix.data):
        raise ValueError("%s: diag.data overlaps matrix.data (the update is in place)" % name)
    max_dim = _max_size(diag.row_blk_size)
    if max_dim > BLOCK_INVERSE_MAX_DIM:
        raise NotImplementedError("%s: a diagonal block of %d (diagonal blocks of up to %d are applied)" % (name, max_dim, BLOCK_INVERSE_MAX_DIM))
    E = engine or default_engine()
    st = StreamHandle(stream)
    d, a = diag.desc(), matrix.desc()   # (only the matrix' data area is written)
    if alpha == 0:
        passes = (("R" if side == "right" else "L", trans, 0.0),)   # (zeros without a read: one launch, whatever the side)
    elif side == "both":
        dagger = _BLOCK_SCALE_DAGGER[trans] if zc else ("T" if trans == "N" else "N")
        passes = (("L", trans, alpha), ("R", dagger, 1.0))
    else:
        passes = (("L" if side == "left" else "R", trans, alpha),)
    for sd, op, al in passes:
        rc = E.L.dbcsr_amd_bcsr_block_diag_multiply(E.h, matrix.dtype_code, sd.encode(), op.encode(), _z(al), C.byref(d), C.byref(a), max_dim, st.ptr)
        if rc != 0:
            raise RuntimeError("dbcsr_amd_bcsr_block_diag_multiply failed (%d)" % rc)


# ---- dense conversion ------------------------------------------------------------------------------------------------------------------------------
def _check_dense(name, dtype, device, dense, n_rows, n_cols, what="dense"):
    """a 2-D device tensor of (n_rows, n_cols) elements of `dtype` whose rows or whose columns are contiguous: checked before any call of the library.
    Returns (ld, col_major): strides (ld, 1) with ld >= n_cols -- torch's layout, or a column slice of a wider tensor -- or (1, ld) with ld >= n_rows,
    column by column as a Fortran full matrix is (t.T of a contiguous tensor)."""
    if not isinstance(dense, torch.Tensor):
        raise TypeError("%s: %s must be a torch tensor" % (name, what))
    if dense.dtype != dtype:
        raise TypeError("%s: %s has data type %r, expected %r" % (name, what, dense.dtype, dtype))
    if dense.device != device:
        raise ValueError("%s: %s is not on the matrix' device" % (name, what))
    if dense.dim() != 2 or tuple(dense.shape) != (n_rows, n_cols):
        raise ValueError("%s: %s must be a 2-D tensor of shape (%d, %d), got %r" % (name, what, n_rows, n_cols, tuple(dense.shape)))
    s0, s1 = dense.stride()
    rows_ok, cols_ok = n_cols <= 1 or s1 == 1, n_rows <= 1 or s0 == 1   # (the stride of a dimension of one element, or of none, says nothing)
    if rows_ok and (n_rows <= 1 or s0 >= max(n_cols, 1)):
        return (s0 if n_rows > 1 else max(n_cols, 1)), 0
    if cols_ok and (n_cols <= 1 or s1 >= max(n_rows, 1)):
        return (s1 if n_cols > 1 else max(n_rows, 1)), 1
    if not rows_ok and not cols_ok:
        raise ValueError("%s: %s must have stride(1) == 1 (row by row) or stride(0) == 1 (column by column), got strides %r" % (name, what, (s0, s1)))
    raise ValueError("%s: %s has strides %r: the stride between its rows (columns) is below the %d columns (%d rows) of one" % (name, what, (s0, s1), n_cols, n_rows))


def _dense_overlaps(dense, n_rows, n_cols, ld, col_major, data):
    return _overlaps(dense, n_cols, ld, n_rows, data) if col_major else _overlaps(dense, n_rows, ld, n_cols, data)


def dbcsr_to_dense(matrix, out=None, engine=None, stream=None):
    """The full (n_rows, n_cols) matrix as a dense device tensor (dbcsr_to_dense_local; CP2K's copy_dbcsr_to_fm), without leaving the device: what
    torch.linalg.eigh / cholesky / svd, a dense Rayleigh-Ritz step or a comparison with a dense matrix take.  The stored blocks are at their places as
    bit-for-bit copies, every other element is +0.0.  A stored triangle is expanded with the reading of the desymmetrized operands of a multiply: where
    (r, c) is not stored and (c, r) is, the tile is that block's twin -- 'S' its transpose, 'A' minus its transpose, 'H' its conjugate transpose, 'K' minus
    its conjugate transpose (sign flips: exact); diagonal blocks are taken in full as stored, nothing is symmetrised.
    out=None allocates a contiguous row-by-row tensor on the matrix' device and stream.  Otherwise out is a 2-D device tensor of the matrix' data type and
    that shape with strides (ld, 1), ld >= n_cols -- torch's layout, or a column slice of a wider tensor -- or (1, ld), ld >= n_rows -- column by column, what
    a Fortran full matrix is: t.T of a contiguous tensor.  Every element of the window is written exactly once per call, whatever out held; nothing outside
    it is written: the padding between the window and ld keeps its bits.  out must not overlap matrix.data (ValueError).  The matrix is only read: it keeps
    its index_stamp() and no saved plan is touched.  float64, float32 and complex128; packed and unpacked matrices.  Asynchronous on the stream (the first
    call for a set of block sizes synchronises once to learn their sums), the same bits on every call; every refusal comes before any call of the
    library.  Returns out."""
    name = "dbcsr_to_dense"
    sym = _check_symmetry(name, matrix)
    matrix.dtype_code
    kind = -1
    if sym != "N":
        kind = matrix.symmetry_kind()
        _check_square(name, matrix)
    n_rows, n_cols = _full_size(matrix.row_blk_size), _full_size(matrix.col_blk_size)
    ld, col_major = max(n_cols, 1), 0
    if out is not None:
        ld, col_major = _check_dense(name, matrix.dtype, matrix.row_p.device, out, n_rows, n_cols, "out")
        if _dense_overlaps(out, n_rows, n_cols, ld, col_major, matrix.data):
            raise ValueError("%s: out overlaps the matrix' data area" % name)
    E = engine or default_engine()
    st = StreamHandle(stream)
    if out is None:
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            out = torch.empty((n_rows, n_cols), dtype=matrix.dtype, device=matrix.row_p.device)
    d = matrix.desc()
    rc = E.L.dbcsr_amd_bcsr_to_dense(E.h, matrix.dtype_code, C.byref(d), kind, out.data_ptr() if n_rows and n_cols else None, n_rows, n_cols, ld, col_major,
                                     st.ptr)
    if rc != 0:
        raise RuntimeError("dbcsr_amd_bcsr_to_dense failed (%d)" % rc)
    return out


def dbcsr_from_dense(dense, matrix, engine=None, stream=None):
    """Every block the matrix stores <- the dense tensor's elements at its place, bit for bit, and nothing else (CP2K's copy_fm_to_dbcsr with keep_sparsity):
    the way back from a dense step -- eigenvectors, a Cholesky factor, a dense guess -- onto the pattern the matrix has.  dense: a 2-D device tensor of the
    matrix' data type and full shape, in one of dbcsr_to_dense's two layouts.  The pattern never changes: no index array is written, index_stamp() stays, a
    multiply with the matrix as operand afterwards reuses its plan; the holes of an unpacked matrix and everything around the blocks keep their bits; block
    norms a multiply announced are forgotten.  No symmetry is applied: of a stored triangle the blocks the matrix stores are taken from where they lie, the
    other triangle of dense is not read.  dense must not overlap matrix.data (ValueError).  Asynchronous on the stream as dbcsr_to_dense is; every refusal
    comes before any call of the library.  Returns matrix."""
    name = "dbcsr_from_dense"
    sym = _check_symmetry(name, matrix)
    matrix.dtype_code
    if sym != "N":
        matrix.symmetry_kind()
        _check_square(name, matrix)
    n_rows, n_cols = _full_size(matrix.row_blk_size), _full_size(matrix.col_blk_size)
    ld, col_major = _check_dense(name, matrix.dtype, matrix.row_p.device, dense, n_rows, n_cols)
    if _dense_overlaps(dense, n_rows, n_cols, ld, col_major, matrix.data):
        raise ValueError("%s: dense overlaps the matrix' data area" % name)
    E = engine or default_engine()
    st = StreamHandle(stream)
    d = matrix.desc()   # (only the data area is written)
    rc = E.L.dbcsr_amd_bcsr_from_dense_apply(E.h, matrix.dtype_code, dense.data_ptr() if n_rows and n_cols else None, n_rows, n_cols, ld, col_major,
                                             C.byref(d), st.ptr)
    if rc != 0:
        raise RuntimeError("dbcsr_amd_bcsr_from_dense_apply failed (%d)" % rc)
    return matrix


def _block_sizes(name, what, sizes, device):
    """block sizes as the matrices hold them: a 1-D int32 tensor on the device (a tensor that already is one is taken as it is)"""
    if isinstance(sizes, torch.Tensor) and sizes.dtype == torch.int32 and sizes.device == device and sizes.dim() == 1 and sizes.is_contiguous():
        return sizes
    t = torch.as_tensor(sizes)
    if t.dim() != 1 or t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
        raise TypeError("%s: %s must be a 1-D sequence of integers" % (name, what))
    if t.numel() and int(t.min()) < 0:
        raise ValueError("%s: %s has a negative block size" % (name, what))
    return t.to(dtype=torch.int32).contiguous().to(device)


def dbcsr_create_from_dense(dense, row_blk_size, col_blk_size, eps=0.0, name="", engine=None, stream=None):
    """A new packed matrix without symmetry that holds the blocks of the dense device tensor which the block filter would keep: a block of the structure
    row_blk_size x col_blk_size is dropped iff ||blk||_F^2 < eps^2 (dbcsr_filter's rule: a block whose norm is NaN stays; eps = 0.0 keeps every block, a
    full pattern).  The index is sorted and packed -- block columns ascending inside a block row, blk_p the running sum of the block sizes -- and the
    blocks are bit-for-bit copies.  dense: a 2-D device tensor (float64, float32 or complex128) in one of dbcsr_to_dense's two layouts, whose shape is the
    sums of the block sizes (ValueError otherwise); the block sizes: int32 device tensors as the matrices hold them (taken as they are), or any sequence of
    integers.  Norms summed in double in a fixed order: the same pattern and bits on every call.  Synchronises once (the size of the result); every
    refusal comes before any call of the library."""
    fn = "dbcsr_create_from_dense"
    if not isinstance(dense, torch.Tensor):
        raise TypeError("%s: dense must be a torch tensor" % fn)
    code = _dtype_code(dense.dtype)
    eps = float(eps)
    if not eps >= 0:   # (a NaN compares false)
        raise ValueError("%s: eps must be >= 0, got %r" % (fn, eps))
    if dense.dim() != 2:
        raise ValueError("%s: dense must be a 2-D tensor" % fn)
    if dense.device.type != "cuda":
        raise ValueError("%s: dense is not on a GPU" % fn)
    dev = dense.device
    rs, cs = _block_sizes(fn, "row_blk_size", row_blk_size, dev), _block_sizes(fn, "col_blk_size", col_blk_size, dev)
    n_rows, n_cols = _full_size(rs), _full_size(cs)
    if tuple(dense.shape) != (n_rows, n_cols):
        raise ValueError("%s: dense has shape %r, the block sizes sum to (%d, %d)" % (fn, tuple(dense.shape), n_rows, n_cols))
    ld, col_major = _check_dense(fn, dense.dtype, dev, dense, n_rows, n_cols)
    nbr, nbc = int(rs.numel()), int(cs.numel())
    nt = nbr * nbc
    if nt > 2 ** 31 - 9:
        raise ValueError("%s: a block structure of %d x %d blocks" % (fn, nbr, nbc))
    E = engine or default_engine()
    st = StreamHandle(stream)
    ptr = dense.data_ptr() if n_rows and n_cols else None
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        row_p = torch.empty(nbr + 1, dtype=torch.int32, device=dev)
        col_i = torch.empty(nt, dtype=torch.int32, device=dev)
        blk_p = torch.empty(nt, dtype=torch.int64, device=dev)
    nb, nz = C.c_int64(), C.c_int64()
    rc = E.L.dbcsr_amd_bcsr_from_dense_count(E.h, code, ptr, n_rows, n_cols, ld, col_major, rs.data_ptr() if nbr else None, cs.data_ptr() if nbc else None,
                                             nbr, nbc, float(eps), row_p.data_ptr(), col_i.data_ptr() if nt else None, blk_p.data_ptr() if nt else None,
                                             C.byref(nb), C.byref(nz), st.ptr)
    if rc != 0:
        raise RuntimeError("dbcsr_amd_bcsr_from_dense_count failed (%d)" % rc)
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        M = DbcsrMatrix(rs, cs, row_p, col_i[:nb.value].clone(), blk_p[:nb.value].clone(), torch.empty(nz.value, dtype=dense.dtype, device=dev), name)
    d = M.desc()
    rc = E.L.dbcsr_amd_bcsr_from_dense_apply(E.h, code, ptr, n_rows, n_cols, ld, col_major, C.byref(d), st.ptr)
    if rc != 0:
        raise RuntimeError("dbcsr_amd_bcsr_from_dense_apply failed (%d)" % rc)
    return M


# ---- element-wise operations on two patterns ------------------------------------------------------------------------------------------------------------
# func of dbcsr_function_of_elements (the reference's constants; 5, 6 and 14 are inverse_special, spread_from_zero and truncate: not offered)
dbcsr_func_inverse = 0
dbcsr_func_tanh = 1
dbcsr_func_dtanh = 2
dbcsr_func_ddtanh = 3
dbcsr_func_artanh = 4
dbcsr_func_sin = 7
dbcsr_func_dsin = 8
dbcsr_func_ddsin = 9
dbcsr_func_asin = 10
dbcsr_func_cos = 11
dbcsr_func_dcos = 12
dbcsr_func_ddcos = 13
_FUNCTIONS = (dbcsr_func_inverse, dbcsr_func_tanh, dbcsr_func_dtanh, dbcsr_func_ddtanh, dbcsr_func_artanh, dbcsr_func_sin, dbcsr_func_dsin,
              dbcsr_func_ddsin, dbcsr_func_asin, dbcsr_func_cos, dbcsr_func_dcos, dbcsr_func_ddcos)


def _check_like(name, what, m, like):
    """m can take a result with like's sizes, data type and symmetry"""
    if m.dtype != like.dtype:
        raise TypeError("%s: the data type of %s differs" % (name, what))
    s, t = _check_symmetry(name, m), _check_symmetry(name, like)
    if s != t:
        raise ValueError("%s: %s has another symmetry (%r, %r)" % (name, what, s, t))
    if not _same_sizes(m, like):
        raise ValueError("%s: row or column block sizes of %s differ" % (name, what))


def _has_index_of(c, a):
    """c's index arrays are a's, or hold the same numbers (compared on the device: synchronises)"""
    if c.row_p is a.row_p and c.col_i is a.col_i and c.blk_p is a.blk_p:
        return True
    return c.nblks == a.nblks and torch.equal(c.row_p, a.row_p) and torch.equal(c.col_i, a.col_i) and torch.equal(c.blk_p, a.blk_p)


def dbcsr_hadamard_product(matrix_a, matrix_b, matrix_c, b_assume_value=None, engine=None, stream=None):
    """C <- A o B, element by element (dbcsr_hadamard_product).  The result has the blocks that both A and B store, in A's order, packed;
    with b_assume_value given it has every block of A, and a block B lacks counts as filled with that value (a value of exactly 1 copies
    A's block bit for bit).  What matrix_c held before is replaced: it adopts the result, as a multiply hands over C.  The reference's
    source could not be consulted for the pattern of the result: this is the semantics of this library.  float64, float32 (one
    multiplication per element: a*b in the data's precision, bit for bit) and complex128; symmetry 'N', and 'S' / 'H' on the stored
    triangles (the element-wise product of two symmetric or hermitian matrices is one again; 'A' / 'K' change class: ValueError).
    matrix_c may be matrix_a or matrix_b.  When B has A's index (row_p, col_i, blk_p) and A is packed -- the usual case inside an
    iteration -- the product is one flat pass, and a matrix_c that is A or B or already has that index is written in place: no index
    array is written, its index_stamp() stays and a multiply with it still reuses its plan.  Returns True when the flat pass was taken,
    False otherwise.  Two patterns cost one synchronisation (the size of the result); the engine's saved plan survives either way."""
    fn = "dbcsr_hadamard_product"
    sym = _check_pair(fn, matrix_a, matrix_b)
    if sym in ("A", "K"):
        raise ValueError("%s: the product of two matrices of symmetry %r is not one of them" % (fn, sym))
    _check_like(fn, "matrix_c", matrix_c, matrix_a)
    if b_assume_value is not None:
        _check_scalar(fn, matrix_a, b_assume_value)
    code = matrix_a.dtype_code
    E = engine or default_engine()
    st = StreamHandle(stream)
    A, B = matrix_a, matrix_b
    dev = A.row_p.device
    a, b = A.desc(), B.desc()
    on_stream = lambda: torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream())
    with on_stream():
        row_p = torch.empty(A.nblkrows + 1, dtype=torch.int32, device=dev)
    nb, nz, same = C.c_int64(), C.c_int64(), C.c_int32()
    rc = E.L.dbcsr_amd_bcsr_hadamard_count(E.h, C.byref(a), C.byref(b), 0 if b_assume_value is None else 1, row_p.data_ptr(), C.byref(nb),
                                           C.byref(nz), C.byref(same), st.ptr)
    if rc != 0:
        raise RuntimeError("dbcsr_amd_bcsr_hadamard_count failed (%d)" % rc)
    value = None if b_assume_value is None else _z(b_assume_value)
    in_place = bool(same.value) and (matrix_c is A or matrix_c is B or _has_index_of(matrix_c, A))
    if in_place:
        # A's own index with C's data area: only that area is written (C.desc(out=True) would bump the stamp)
        dst = A.desc()
        dst.data = matrix_c.data.data_ptr() if matrix_c.data.numel() else None
        out = None
    else:
        with on_stream():
            out = DbcsrMatrix(A.row_blk_size, A.col_blk_size, row_p, torch.empty(nb.value, dtype=torch.int32, device=dev),
                              torch.empty(nb.value, dtype=torch.int64, device=dev), torch.empty(nz.value, dtype=A.dtype, device=dev), matrix_c.name)
        dst = out.desc(out=True)
    rc = E.L.dbcsr_amd_bcsr_hadamard_apply(E.h, code, C.byref(a), C.byref(b), value, C.byref(dst), st.ptr)
    if rc != 0:
        raise RuntimeError("dbcsr_amd_bcsr_hadamard_apply failed (%d)" % rc)
    if out is not None:
        matrix_c.adopt(out)   # as a multiply hands its result to matrix_c
    return bool(same.value)


def dbcsr_copy(matrix_b, matrix_a, keep_sparsity=False, engine=None, stream=None):
    """B <- A (dbcsr_copy).  Without keep_sparsity B adopts a copy of A, index and data, and takes A's symmetry.  With
    keep_sparsity=True B keeps its pattern: every block B stores takes A's block bit for bit where A stores it and becomes +0.0 where A
    does not -- A projected onto B's pattern.  Only B's data area is written, in place: no index array is written, index_stamp() stays, holes
    of a B that is not packed keep their bits.  No count step and no synchronisation: asynchronous on stream.  float64, float32 and
    complex128; same sizes, data type and symmetry (TypeError / ValueError); matrices that share a data area: ValueError."""
    fn = "dbcsr_copy"
    _check_symmetry(fn, matrix_a)
    code = matrix_a.dtype_code
    if not keep_sparsity:
        if matrix_b.dtype != matrix_a.dtype:
            raise TypeError("%s: the data types of the two matrices differ" % fn)
        if not _same_sizes(matrix_b, matrix_a):
            raise ValueError("%s: row or column block sizes of the two matrices differ" % fn)
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            matrix_b.adopt(matrix_a.copy())
        matrix_b.symmetry = matrix_a.symmetry
        return
    _check_like(fn, "matrix_b", matrix_b, matrix_a)
    if matrix_b is matrix_a or _data_overlap(matrix_a.data, matrix_b.data):
        raise ValueError("%s: the two matrices share a data area" % fn)
    E = engine or default_engine()
    st = StreamHandle(stream)
    a, b = matrix_a.desc(), matrix_b.desc()   # (only B's data area is written)
    rc = E.L.dbcsr_amd_bcsr_copy_onto(E.h, code, C.byref(a), C.byref(b), st.ptr)
    if rc != 0:
        raise RuntimeError("dbcsr_amd_bcsr_copy_onto failed (%d)" % rc)


def dbcsr_function_of_elements(matrix_a, func, a0=0.0, a1=1.0, a2=None, engine=None, stream=None):
    """x <- f(a1*x + a0) in place on every element the index names (dbcsr_function_of_elements); holes keep their bits, the index and
    index_stamp() stay.  With y = a1*x + a0, func is one of dbcsr_func_inverse 1/y, _tanh tanh y, _dtanh a1*(1 - tanh^2 y), _ddtanh
    -2*a1^2*tanh y*(1 - tanh^2 y), _artanh atanh y, _sin sin y, _dsin a1*cos y, _ddsin -a1^2*sin y, _asin asin y, _cos cos y, _dcos
    -a1*sin y, _ddcos -a1^2*cos y.  The reference has three functions more (inverse_special, spread_from_zero, truncate) and a parameter
    a2; their definitions could not be checked against its sources, so they are not offered rather than guessed: any other func, or an
    a2 that is not None / 0, raises NotImplementedError.  float64 and float32 (the value is formed in double and rounded once); complex
    data: NotImplementedError.  Asynchronous on stream."""
    fn = "dbcsr_function_of_elements"
    _check_symmetry(fn, matrix_a)
    if isinstance(func, bool) or not isinstance(func, int) or func not in _FUNCTIONS:
        raise NotImplementedError("%s: func %r" % (fn, func))
    if a2 is not None and a2 != 0:
        raise NotImplementedError("%s: a2 = %r (no function offered here takes a third parameter)" % (fn, a2))
    code = matrix_a.dtype_code
    if matrix_a.dtype.is_complex:
        raise NotImplementedError("%s: complex data" % fn)
    E = engine or default_engine()
    st = StreamHandle(stream)
    d = matrix_a.desc()   # (only the data area is written)
    rc = E.L.dbcsr_amd_bcsr_function_of_elements(E.h, code, C.byref(d), int(func), float(a0), float(a1), st.ptr)
    if rc != 0:
        raise RuntimeError("dbcsr_amd_bcsr_function_of_elements failed (%d)" % rc)


# ---- block lists: reserve, put and get through a coordinate list of blocks ----------------------------------------------------------------------------------
def _on_stream(stream):
    return torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream())


def _check_list(name, matrix, rows, cols):
    """rows / cols of a block list: 1-D int32 tensors of one length on the matrix' device (TypeError for what is no int32 tensor, ValueError otherwise);
    returns them contiguous and their length"""
    for what, t in (("rows", rows), ("cols", cols)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32:
            raise TypeError("%s: %s must be an int32 torch tensor" % (name, what))
        if t.dim() != 1:
            raise ValueError("%s: %s must be 1-D, got %d dimensions" % (name, what, t.dim()))
    if rows.numel() != cols.numel():
        raise ValueError("%s: rows and cols differ in length (%d, %d)" % (name, rows.numel(), cols.numel()))
    for what, t in (("rows", rows), ("cols", cols)):
        if t.device != matrix.row_p.device:
            raise ValueError("%s: %s is not on the matrix' device" % (name, what))
    if rows.numel() > 2 ** 31 - 1:
        raise ValueError("%s: a list of %d entries" % (name, rows.numel()))
    return rows.contiguous(), cols.contiguous(), int(rows.numel())


def _check_offsets(name, offsets, n, device):
    if not isinstance(offsets, torch.Tensor) or offsets.dtype != torch.int64:
        raise TypeError("%s: offsets must be an int64 torch tensor" % name)
    if offsets.dim() != 1 or offsets.numel() != n:
        raise ValueError("%s: offsets must be 1-D with one entry per block of the list" % name)
    if offsets.device != device:
        raise ValueError("%s: offsets is not on the matrix' device" % name)
    return offsets.contiguous()


def _check_flat(name, what, t, matrix):
    if not isinstance(t, torch.Tensor) or t.dtype != matrix.dtype:
        raise TypeError("%s: %s must be a torch tensor of the matrix' data type" % (name, what))
    if t.dim() != 1 or not t.is_contiguous():
        raise ValueError("%s: %s must be a flat (1-D, contiguous) tensor" % (name, what))
    if t.device != matrix.row_p.device:
        raise ValueError("%s: %s is not on the matrix' device" % (name, what))


def _list_windows(matrix, rows, cols, offsets, extent):
    """(rows as the kernels are to see them, offsets, end of the last window or None) of a list, formed with torch on the device without a
    synchronisation.  The size of entry i's window is row_blk_size[rows[i]] * col_blk_size[cols[i]], zero for a coordinate outside the matrix; offsets
    None: the windows one after another.  With an extent (the length of the flat tensor) an entry whose window does not lie inside [0, extent) is
    given the row -1, which every kernel skips: nothing is ever read or written outside the tensor."""
    nbr, nbc = matrix.nblkrows, matrix.nblkcols
    if nbr == 0 or nbc == 0:
        sizes = torch.zeros(rows.numel(), dtype=torch.int64, device=rows.device)
    else:
        ok = (rows >= 0) & (rows < nbr) & (cols >= 0) & (cols < nbc)
        r, c = rows.clamp(0, nbr - 1).long(), cols.clamp(0, nbc - 1).long()
        sizes = torch.where(ok, matrix.row_blk_size[r].long() * matrix.col_blk_size[c].long(), torch.zeros((), dtype=torch.int64, device=rows.device))
    if offsets is None:
        ends = torch.cumsum(sizes, 0)
        offsets = ends - sizes
    else:
        ends = offsets + sizes
    if extent is not None:
        inside = (offsets >= 0) & (ends <= extent)
        rows = torch.where(inside, rows, torch.full((), -1, dtype=torch.int32, device=rows.device))
    return rows, offsets, ends


def dbcsr_reserve_blocks(matrix, rows, cols, engine=None, stream=None):
    """The pattern grows (dbcsr_reserve_blocks): afterwards the matrix stores every block it stored and every block (rows[i], cols[i]) of the list --
    int32 device tensors, any order, duplicates allowed.  Every stored block keeps its bits, every new block is +0.0; the result is packed with
    ascending block columns per row and handed to the matrix with adopt, as the add does.  Returns the number of blocks created.  When the list names
    no block the matrix lacks -- the usual case inside an iteration -- nothing is written: the same tensor objects stay, index_stamp() is unchanged and
    a multiply that had the matrix as operand still reuses its plan.  A coordinate outside [0, nblkrows) x [0, nblkcols), or below the diagonal of a
    matrix with symmetry ('S' 'A' 'H' 'K': the stored triangle is served as it is, a block is not transposed onto its twin), raises ValueError and
    leaves the matrix unchanged.  float64, float32 and complex128.  Synchronises once."""
    fn = "dbcsr_reserve_blocks"
    rows, cols, n = _check_list(fn, matrix, rows, cols)
    sym = _check_symmetry(fn, matrix)
    code = matrix.dtype_code
    if sym != "N" and matrix.nblkrows != matrix.nblkcols:
        raise ValueError("%s: a matrix with symmetry %r that is not square" % (fn, sym))
    if n == 0:
        return 0
    E = engine or default_engine()
    st = StreamHandle(stream)
    A = matrix
    dev = A.row_p.device
    a = A.desc()
    with _on_stream(stream):
        row_p = torch.empty(A.nblkrows + 1, dtype=torch.int32, device=dev)
    nb, nz, new, bad = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
    rc = E.L.dbcsr_amd_bcsr_reserve_count(E.h, C.byref(a), n, rows.data_ptr(), cols.data_ptr(), 0 if sym == "N" else 1, row_p.data_ptr(), C.byref(nb),
                                          C.byref(nz), C.byref(new), C.byref(bad), st.ptr)
    if rc != 0:
        raise RuntimeError("dbcsr_amd_bcsr_reserve_count failed (%d)" % rc)
    if bad.value:
        raise ValueError("%s: %d of %d coordinates lie outside the %d x %d blocks of the matrix%s" %
                         (fn, bad.value, n, A.nblkrows, A.nblkcols, "" if sym == "N" else " or below the diagonal of its stored triangle"))
    if new.value == 0:
        return 0
    with _on_stream(stream):
        out = DbcsrMatrix(A.row_blk_size, A.col_blk_size, row_p, torch.empty(nb.value, dtype=torch.int32, device=dev),
                          torch.empty(nb.value, dtype=torch.int64, device=dev), torch.empty(nz.value, dtype=A.dtype, device=dev), A.name)
    dst = out.desc(out=True)
    rc = E.L.dbcsr_amd_bcsr_reserve_apply(E.h, code, C.byref(a), C.byref(dst), st.ptr)
    if rc != 0:
        raise RuntimeError("dbcsr_amd_bcsr_reserve_apply failed (%d)" % rc)
    matrix.adopt(out)   # as a multiply hands its result to matrix_c
    return int(new.value)


def dbcsr_put_blocks(matrix, rows, cols, data, offsets=None, summation=False, alpha=1.0, keep_sparsity=False, engine=None, stream=None):
    """Blocks into the matrix (dbcsr_put_block with summation and scale, for a whole list at once): per entry A_rc <- A_rc + alpha*X with summation,
    A_rc <- alpha*X without.  rows, cols: int32 device tensors, any order, duplicates allowed; data: one flat tensor of the matrix' type that holds
    the blocks, each column-major as the library stores blocks; offsets: int64 device tensor of the element offsets of the blocks in data, None: one
    block after another in list order.  keep_sparsity=False first reserves the listed blocks (dbcsr_reserve_blocks: its errors, its one
    synchronisation, and a new index only when the pattern grows); with True, entries whose block the matrix does not store are skipped.
    Contributions to one block are applied in list order: with summation all are added in that order, without it the last of the list wins.  The
    same bits on every call.  With alpha == 1 nothing is multiplied: an overwrite is bit for bit, a sum is the type's own addition.  The put itself
    never synchronises and writes no index array: index_stamp() stays, holes of an unpacked matrix keep their bits, and a multiply afterwards reuses
    its plan when the pattern held.  An entry whose window does not lie inside data is skipped (checked on the device, nothing outside data is read).
    data sharing memory with the matrix' data area: ValueError.  float64, float32 and complex128."""
    fn = "dbcsr_put_blocks"
    rows, cols, n = _check_list(fn, matrix, rows, cols)
    _check_flat(fn, "data", data, matrix)
    if offsets is not None:
        offsets = _check_offsets(fn, offsets, n, matrix.row_p.device)
    _check_symmetry(fn, matrix)
    _check_scalar(fn, matrix, alpha)
    code = matrix.dtype_code
    if _data_overlap(data, matrix.data):
        raise ValueError("%s: data shares memory with the matrix' data area" % fn)
    if n == 0:
        return
    if not keep_sparsity:
        dbcsr_reserve_blocks(matrix, rows, cols, engine=engine, stream=stream)
    E = engine or default_engine()
    st = StreamHandle(stream)
    with _on_stream(stream):
        seen, offsets, _ = _list_windows(matrix, rows, cols, offsets, int(data.numel()))
    d = matrix.desc()   # (only the data area is written)
    rc = E.L.dbcsr_amd_bcsr_put_blocks(E.h, code, C.byref(d), n, seen.data_ptr(), cols.data_ptr(), offsets.data_ptr(),
                                       data.data_ptr() if data.numel() else None, _z(alpha), 1 if summation else 0, st.ptr)
    if rc != 0:
        raise RuntimeError("dbcsr_amd_bcsr_put_blocks failed (%d)" % rc)


def dbcsr_get_blocks(matrix, rows, cols, out=None, offsets=None, engine=None, stream=None):
    """Blocks out of the matrix (dbcsr_get_block_p, for a whole list at once): returns (data, found).  Every listed block is copied bit for bit into the
    flat tensor data at its offset (offsets as in dbcsr_put_blocks; None: one block after another) and found[i] (int32, device) is 1; where the
    matrix stores no such block the window is +0.0 and found[i] is 0; a coordinate outside the matrix has no window and found[i] is 0.  Every element
    of every window is written exactly once, nothing outside; duplicates are fine, each has its window.  out: the flat tensor to write into (then
    nothing synchronises; an entry whose window does not lie inside out is treated as out of range; windows that overlap each other are the caller's
    error; out sharing memory with the matrix' data area: ValueError); None: a tensor of the needed length is made, zero between windows, which costs
    one synchronisation for its length.  Uses no saved plan and no work area.  float64, float32 and complex128."""
    fn = "dbcsr_get_blocks"
    rows, cols, n = _check_list(fn, matrix, rows, cols)
    if out is not None:
        _check_flat(fn, "out", out, matrix)
    if offsets is not None:
        offsets = _check_offsets(fn, offsets, n, matrix.row_p.device)
    _check_symmetry(fn, matrix)
    code = matrix.dtype_code
    if out is not None and _data_overlap(out, matrix.data):
        raise ValueError("%s: out shares memory with the matrix' data area" % fn)
    dev = matrix.row_p.device
    E = engine or default_engine()
    st = StreamHandle(stream)
    with _on_stream(stream):
        found = torch.empty(n, dtype=torch.int32, device=dev)
        if n == 0:
            return (out if out is not None else torch.empty(0, dtype=matrix.dtype, device=dev)), found
        if out is None:
            given = offsets is not None
            _, offsets, ends = _list_windows(matrix, rows, cols, offsets, None)
            if given and int(offsets.min()) < 0:
                raise ValueError("%s: a negative offset" % fn)
            length = max(int(ends.max()), 0)
            out = torch.zeros(length, dtype=matrix.dtype, device=dev) if given else torch.empty(length, dtype=matrix.dtype, device=dev)
            seen = rows
        else:
            seen, offsets, _ = _list_windows(matrix, rows, cols, offsets, int(out.numel()))
    d = matrix.desc()
    rc = E.L.dbcsr_amd_bcsr_get_blocks(E.h, code, C.byref(d), n, seen.data_ptr(), cols.data_ptr(), offsets.data_ptr(),
                                       out.data_ptr() if out.numel() else None, found.data_ptr(), st.ptr)
    if rc != 0:
        raise RuntimeError("dbcsr_amd_bcsr_get_blocks failed (%d)" % rc)
    return out, found


def dbcsr_reserve_diag_blocks(matrix, engine=None, stream=None):
    """dbcsr_reserve_diag_blocks: every diagonal block (i, i), i below min(nblkrows, nblkcols), is stored afterwards; returns the number created."""
    k = min(matrix.nblkrows, matrix.nblkcols)
    with _on_stream(stream):
        d = torch.arange(k, dtype=torch.int32, device=matrix.row_p.device)
    return dbcsr_reserve_blocks(matrix, d, d, engine=engine, stream=stream)


def dbcsr_reserve_all_blocks(matrix, engine=None, stream=None):
    """dbcsr_reserve_all_blocks: every block is stored afterwards -- of a matrix with symmetry every block of the stored (upper) triangle; returns the
    number created."""
    nbr, nbc = matrix.nblkrows, matrix.nblkcols
    if nbr * nbc > 2 ** 31 - 1:
        raise ValueError("dbcsr_reserve_all_blocks: a block structure of %d x %d blocks" % (nbr, nbc))
    with _on_stream(stream):
        t = torch.arange(nbr * nbc, dtype=torch.int64, device=matrix.row_p.device)
        r, c = (t // max(nbc, 1)).to(torch.int32), (t % max(nbc, 1)).to(torch.int32)
        if _check_symmetry("dbcsr_reserve_all_blocks", matrix) != "N":
            upper = c >= r
            r, c = r[upper], c[upper]
    return dbcsr_reserve_blocks(matrix, r, c, engine=engine, stream=stream)


def dbcsr_create_from_blocks(row_blk_size, col_blk_size, rows, cols, data, offsets=None, summation=True, name="", engine=None, stream=None):
    """A new packed matrix without symmetry from a list of blocks: an empty matrix of these block sizes, then dbcsr_put_blocks(rows, cols, data,
    offsets, summation) onto it -- the device-side from_host for callers who hold blocks, not CSR arrays.  Blocks named more than once are summed in
    list order (summation=True) or the last one wins.  The block sizes: int32 device tensors as the matrices hold them (taken as they are), or any
    sequence of integers.  data: a flat device tensor (float64, float32 or complex128)."""
    fn = "dbcsr_create_from_blocks"
    if not isinstance(data, torch.Tensor):
        raise TypeError("%s: data must be a torch tensor" % fn)
    _dtype_code(data.dtype)
    if data.device.type != "cuda":
        raise ValueError("%s: data is not on a GPU" % fn)
    dev = data.device
    rs, cs = _block_sizes(fn, "row_blk_size", row_blk_size, dev), _block_sizes(fn, "col_blk_size", col_blk_size, dev)
    with _on_stream(stream):
        M = DbcsrMatrix.empty_like_pattern(rs, cs, data.dtype, device=dev, name=name)
    dbcsr_put_blocks(M, rows, cols, data, offsets=offsets, summation=summation, engine=engine, stream=stream)
    return M
