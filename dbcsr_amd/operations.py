"""Matrix algebra between multiplies -- host-side mirror of the reference's element-wise and reduction operations
(src/ops/dbcsr_operations.F) on device-resident matrices:

    dbcsr_add(matrix_a, matrix_b, alpha_scalar, beta_scalar)    A <- alpha*A + beta*B
    dbcsr_scale(matrix, alpha)                                  A <- alpha*A
    dbcsr_add_on_diag(matrix, alpha)                            A <- A + alpha*I
    dbcsr_trace(matrix)                                         sum of the diagonal elements
    dbcsr_dot(matrix_a, matrix_b)                               sum a_ij * b_ij = trace(A^T B)          (real data)
    dbcsr_frobenius_norm(matrix)                                sqrt(sum |x|^2)

Same argument names and error behaviour; the work is done by the C-ABI engine (include/dbcsr_amd_mm.h, "Matrix algebra between
multiplies") on the GPU, for float64, float32 and complex128 data.  One rank / one device here: of a distributed matrix trace, dot
and the squared norm are the local results summed over the ranks."""
import ctypes as C
import math

import torch

from .matrix import DbcsrMatrix, StreamHandle
from .multiply import _z, default_engine

_SYMMETRIES = ("N", "S", "A", "H", "K")


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
