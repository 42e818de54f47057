"""The in-place block filter (dbcsr_amd_bcsr_filter_apply_index, dbcsr_amd_mm_set_filter_in_place) as far as it can be checked
without a GPU: the entry points exist in the header, the binding and the library, and the Python side counts the stored elements of
an unpacked matrix (DbcsrMatrix.nze / packed) instead of the size of its data area."""
import os
import re

import numpy as np
import pytest
import torch

from dbcsr_amd import lib
from dbcsr_amd.matrix import DbcsrMatrix
from dbcsr_amd.multiply import MultiplyEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dbcsr_amd_bcsr_filter_apply_index", "dbcsr_amd_mm_set_filter_in_place")


@pytest.mark.parametrize("name", NEW)
def test_entry_points_in_header_binding_and_library(name):
    header = open(os.path.join(ROOT, "include", "dbcsr_amd_mm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"^int\s+%s\s*\(" % name, code, flags=re.M), "%s is not declared in include/dbcsr_amd_mm.h" % name
    assert name in lib.MM_SYMBOLS
    import __graft_entry__ as g
    g.build_native()
    L = lib.load_library()
    assert hasattr(L, name), "libdbcsr_acc_amd.so does not export %s" % name
    assert getattr(L, name).argtypes is not None


def host_matrix(nbr, nbc, bs, per_row, area=None, nze=None):
    """nbr x nbc blocks of bs x bs, per_row blocks in every block row, on CPU tensors; area: size of the data area (default: packed)"""
    rs = torch.full((nbr,), bs, dtype=torch.int32)
    cs = torch.full((nbc,), bs, dtype=torch.int32)
    nb = nbr * per_row
    row_p = torch.arange(0, nb + 1, per_row, dtype=torch.int32)
    col_i = (torch.arange(nb, dtype=torch.int32) % per_row)
    stride = bs * bs if area is None else area // nb
    blk_p = torch.arange(nb, dtype=torch.int64) * stride
    data = torch.zeros(nb * bs * bs if area is None else area, dtype=torch.float64)
    return DbcsrMatrix(rs, cs, row_p, col_i, blk_p, data, "M", nze=nze)


def test_nze_and_packed():
    M = host_matrix(4, 6, 3, 2)
    assert M.nze == M.data.numel() == 4 * 2 * 9 and M.packed
    U = host_matrix(4, 6, 3, 2, area=3 * 4 * 2 * 9, nze=4 * 2 * 9)
    assert U.nze == 72 and U.data.numel() == 216 and not U.packed
    for X in (M, U):
        Y = X.copy()
        assert Y.nze == X.nze and Y.packed == X.packed and Y.data.numel() == X.data.numel()
        assert Y.data.data_ptr() != X.data.data_ptr() and np.array_equal(Y.blk_p.numpy(), X.blk_p.numpy())
    # the result of a multiply travels with its element count
    T = host_matrix(4, 6, 3, 1)
    T.adopt(U)
    assert T.data is U.data and T.blk_p is U.blk_p and T.nze == 72 and not T.packed
    T.adopt(M)
    assert T.packed and T.nze == 72


def test_auto_kchunks_counts_stored_elements_not_the_data_area(monkeypatch):
    monkeypatch.delenv("DBCSR_AMD_MM_KCHUNKS", raising=False)
    eng = object.__new__(MultiplyEngine)   # (no handle: _auto_kchunks is arithmetic on the operands' descriptions)
    # 64 x 256 blocks of 16 x 16, 250 per row: rows of 0.5 MB -- one pass.  The same operand in a data area three times as large
    # (1.5 MB per row by data.numel(): two passes) must give the same answer.
    nbr, nbc, bs, per_row = 64, 256, 16, 250
    nze = nbr * per_row * bs * bs
    packed = host_matrix(nbr, nbc, bs, per_row)
    unpacked = host_matrix(nbr, nbc, bs, per_row, area=3 * nze, nze=nze)
    assert nze * 8 / nbr <= MultiplyEngine.KCHUNK_ROW_BYTES < 3 * nze * 8 / nbr
    assert eng._auto_kchunks(packed, 0.0, packed) == eng._auto_kchunks(unpacked, 0.0, packed) == 1
    # ... and blocks of 30 x 30, rows of 1.8 MB: two passes either way (by data.numel() a data area four times as large would look
    # like "blocks above 32 x 32 on average", one pass, or like rows of 7.2 MB, eight)
    bs = 30
    nze = nbr * per_row * bs * bs
    packed = host_matrix(nbr, nbc, bs, per_row)
    unpacked = host_matrix(nbr, nbc, bs, per_row, area=4 * nze, nze=nze)
    assert eng._auto_kchunks(packed, 0.0, packed) == 2
    assert eng._auto_kchunks(unpacked, 0.0, packed) == 2
