"""Helpers shared by the -m gpu parity tests (device <-> oracle plumbing)."""

import ctypes as C

import numpy as np
import torch

from dbcsr_amd import lib as L
from dbcsr_amd.matrix import DbcsrMatrix, StreamHandle


def to_dev(M, name=""):
    return DbcsrMatrix.from_host(M.row_sizes, M.col_sizes, M.row_p, M.col_i, M.blk_p, M.data, name=name)


def dev_to_bcsr(D):
    from oracle import oracle as O
    rs, cs, row_p, col_i, blk_p, data = D.to_host()
    return O.Bcsr(rs, cs, row_p, col_i, blk_p, data)


def fetch(lib, ptr, count, dtype):
    """count elements of dtype from a device pointer of the C ABI"""
    out = np.empty(count, dtype)
    if count:
        assert lib.c_dbcsr_acc_memcpy_d2h(C.c_void_p(ptr), out.ctypes.data_as(C.c_void_p), C.c_size_t(out.nbytes), None) == 0
        assert lib.c_dbcsr_acc_device_synchronize() == 0
    return out


def fetch_result(lib, out, like, dtype):
    """a matrix the C entry allocated (dbcsr_amd_bcsr) on the host, with the block sizes of `like`; the device arrays are released"""
    from oracle import oracle as O
    nbr, nblks = int(out.nblkrows), int(out.nblks)
    row_p = fetch(lib, out.row_p, nbr + 1, np.int32)
    assert row_p[-1] == nblks
    col_i, blk_p = fetch(lib, out.col_i, nblks, np.int32), fetch(lib, out.blk_p, nblks, np.int64)
    rows = np.repeat(np.arange(nbr), np.diff(row_p))
    size = like.row_sizes[rows].astype(np.int64) * like.col_sizes[col_i]
    extent = int((blk_p + size).max()) if nblks else 0   # (an in-place filter leaves the blocks where they were: the data area may have holes)
    data = fetch(lib, out.data, extent, dtype)
    assert lib.dbcsr_amd_bcsr_release(C.byref(out)) == 0
    return O.Bcsr(like.row_sizes, like.col_sizes, row_p, col_i, blk_p, data)


def native_multiply_any(E, transa, transb, alpha, A, B, beta, Cm, limits=None, retain=False, eps=0.0, symm_c="N", klimits=None):
    """One multiply through the C entry on engine E's handle, host matrices in, (host result, flop) out.  The entry follows the data type and the product's
    symmetry: dbcsr_amd_multiply (real), dbcsr_amd_multiply_z (complex128), dbcsr_amd_multiply_symmetric_c / _symmetric_c_klimits (klimits given) /
    _symmetric_c_z for a product matrix with symmetry symm_c (Cm: its stored triangle)."""
    lib, dtype = E.L, Cm.data.dtype
    cplx = dtype.kind == "c"
    dA, dB, dC = to_dev(A), to_dev(B), to_dev(Cm)
    a, b, c = dA.desc(), dB.desc(), dC.desc()
    out, flop = L.BcsrDesc(), C.c_int64(0)
    lim = (C.c_int64 * 6)(*limits) if limits is not None else None
    code = L.dbcsr_type_complex_8 if cplx else (L.dbcsr_type_real_8 if dtype == np.float64 else L.dbcsr_type_real_4)
    z = lambda x: (C.c_double * 2)(complex(x).real, complex(x).imag)
    ta, tb = transa.encode(), transb.encode()
    k0, k1 = klimits or (0, 0)
    if symm_c != "N":
        kind = L.SYMMETRY_KIND[symm_c]
        if cplx:
            rc = lib.dbcsr_amd_multiply_symmetric_c_z(E.h, ta, tb, z(alpha), C.byref(a), C.byref(b), z(beta), C.byref(c), kind, k0, k1, 1 if retain else 0,
                                                      float(eps), C.byref(out), C.byref(flop), None)
        elif klimits is not None:   # (no argument types are declared for this entry: every argument in its C type)
            rc = lib.dbcsr_amd_multiply_symmetric_c_klimits(E.h, C.c_char(ta), C.c_char(tb), C.c_int(code), C.c_double(alpha), C.byref(a), C.byref(b),
                                                            C.c_double(beta), C.byref(c), C.c_int(kind), C.c_int64(k0), C.c_int64(k1),
                                                            C.c_int(1 if retain else 0), C.c_double(eps), C.byref(out), C.byref(flop), None)
        else:
            rc = lib.dbcsr_amd_multiply_symmetric_c(E.h, ta, tb, code, float(alpha), C.byref(a), C.byref(b), float(beta), C.byref(c), kind,
                                                    1 if retain else 0, float(eps), C.byref(out), C.byref(flop), None)
    elif cplx:
        rc = lib.dbcsr_amd_multiply_z(E.h, ta, tb, z(alpha), C.byref(a), C.byref(b), z(beta), C.byref(c), lim, 1 if retain else 0, float(eps), C.byref(out),
                                      C.byref(flop), None)
    else:
        rc = lib.dbcsr_amd_multiply(E.h, ta, tb, code, float(alpha), C.byref(a), C.byref(b), float(beta), C.byref(c), lim, 1 if retain else 0, float(eps),
                                    C.byref(out), C.byref(flop), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return fetch_result(lib, out, Cm, dtype), flop.value


def rel_err(x, ref):
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    if ref.size == 0:
        return 0.0
    scale = np.maximum(np.abs(ref), 1e-300)
    return float(np.max(np.abs(x - ref) / scale))


def run_stack(stack, a, b, c, m, n, k, dtype_code, max_kernel_dim=80, transpose_b=True):
    """transpose B blocks (as the Fortran host does each tick) then libsmm_acc_process; returns C (host)."""
    lib = L.load_library()
    dev = "cuda"
    st = StreamHandle()
    ta, tb, tc = torch.as_tensor(a).to(dev), torch.as_tensor(b).to(dev), torch.as_tensor(c).to(dev)
    tstack = torch.as_tensor(np.ascontiguousarray(stack, np.int32)).to(dev)
    nstack = len(stack) // 3
    if transpose_b:
        kn = k * n
        trs = torch.arange(0, b.size, kn, dtype=torch.int32, device=dev)
        rc = lib.libsmm_acc_transpose(trs.data_ptr(), 0, int(trs.numel()), tb.data_ptr(), dtype_code, k, n, max_kernel_dim, st.ptr)
        assert rc == 0
    rc = lib.libsmm_acc_process(None, tstack.data_ptr(), nstack, dtype_code, ta.data_ptr(), tb.data_ptr(), tc.data_ptr(), m, n, k,
                                max_kernel_dim, 1, st.ptr, st.ptr)
    torch.cuda.synchronize()
    return rc, tc.cpu().numpy()
