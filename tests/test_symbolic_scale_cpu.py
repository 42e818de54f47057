"""The symbolic phase at scale, without a GPU: the choices of dbcsr_amd/csrc/mm_choose.h (choose_symbolic_pattern, choose_symbolic_count, choose_panels,
panel_bytes_of_mb) held to a table, the conditions on every case of tests/symbolic_scale.py, and the launch order (order_count / order_fill and the class
form of mm_symbolic.h) restated in numpy and shown to be a permutation of C's blocks for one, three and W column panels -- the property
tests/test_gpu_symbolic_scale.py then checks on the device's own arrays through the results."""
import ctypes
import shutil
import subprocess
import time

import numpy as np
import pytest

from tests import symbolic_scale as S
from tests.test_numeric_choice import CSRC, choose, shims  # noqa: F401  (the host build of mm_choose.h around choose_numeric: a module-scoped fixture)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++ to compile the shim around mm_choose.h")
    d = tmp_path_factory.mktemp("symbolic_choice")
    (d / "shim.cpp").write_text(S.SHIM)
    subprocess.run([gxx, "-std=c++17", "-O1", "-shared", "-fPIC", "-I", CSRC, str(d / "shim.cpp"), "-o", str(d / "shim.so")], check=True)
    lib = ctypes.CDLL(str(d / "shim.so"))
    lib.panel_bytes.restype = ctypes.c_longlong
    lib.panel_bytes.argtypes = [ctypes.c_longlong]
    return lib


def class_mode(shims, case):  # noqa: F811
    """cls_mode of choose_classes for the case's sizes and C blocks (complex data: the rule reads sizes and counts only)"""
    q, kw = S.choice_query(case)
    return choose(shims, case["env"], q, **kw)[1]["cls_mode"]


# ---- the table ---------------------------------------------------------------------------------------------------------------------------------------------
# (nbr, nbk, nbc, a_nblks, b_nblks, c_nblks, keywords) -> the fields that must come out
TABLE = [
    # both sides of nbr = 2048, a sparse product
    ((2047, 100, 2047, 3000, 3000, 100000, {}), dict(sparse_guess=0, rows=0, grid=1)),
    ((2048, 100, 2047, 3000, 3000, 100000, {}), dict(sparse_guess=1, rows=1, grid=0)),
    # the 60 % rule on C's blocks: 10 c < 6 nbr nbc (2048 x 100: 122880 is 60 %) ...
    ((2048, 100, 100, 3000, 3000, 122879, {}), dict(rows=1, grid=0)),
    ((2048, 100, 100, 3000, 3000, 122880, {}), dict(rows=0, grid=1)),
    # ... and on the expected products: a b / nbk < 0.6 nbr nbc
    ((2048, 100, 100, 4096, 2999, 1000, {}), dict(sparse_guess=1)),
    ((2048, 100, 100, 4096, 3000, 1000, {}), dict(sparse_guess=0)),
    # the per-word kernels: nbr nJ 64 > 256 c (1000 rows x 10 groups of 64 columns: 2500 C blocks is the boundary; no C block counts as one)
    ((1000, 50, 640, 500, 500, 2500, {}), dict(grid=1, rows=0)),
    ((1000, 50, 640, 500, 500, 2499, {}), dict(grid=0, rows=0)),
    ((3, 5, 64, 1, 1, 0, {}), dict(grid=1)),
    ((5, 5, 64, 1, 1, 0, {}), dict(grid=0)),
    # forced modes
    ((2048, 100, 2047, 3000, 3000, 100000, dict(forced="word")), dict(sparse_guess=0, rows=0, grid=0)),
    ((2048, 100, 2047, 3000, 3000, 100000, dict(forced="grid")), dict(sparse_guess=0, rows=0, grid=1)),
    ((1000, 50, 640, 500, 500, 2499, dict(forced="grid")), dict(grid=0, rows=0)),   # (grid excludes the product-driven kernels; the density rule stays)
    ((40, 10, 40, 100, 100, 1600, dict(forced="rows")), dict(sparse_guess=1, rows=1, grid=0)),
    ((40, 10, 40, 100, 100, 1600, dict(forced="word")), dict(rows=0, grid=0)),
    # filtering: the grid kernels unless the product-driven ones take over; the product-driven pattern kernel only without retain
    ((1000, 50, 640, 500, 500, 2499, dict(filtering=True)), dict(grid=1, bitmap_rows=0)),
    ((1000, 50, 640, 500, 500, 2499, dict(filtering=True, forced="word")), dict(grid=1, bitmap_rows=0)),
    ((2048, 100, 2047, 3000, 3000, 100000, dict(filtering=True)), dict(sparse_guess=1, bitmap_rows=1, rows=1, grid=0)),
    ((2048, 100, 2047, 3000, 3000, 100000, dict(filtering=True, retain=True)), dict(sparse_guess=1, bitmap_rows=0, rows=1)),
    ((2048, 100, 2047, 3000, 3000, 100000, dict(retain=True)), dict(sparse_guess=1, bitmap_rows=0, rows=1)),
    ((40, 10, 40, 100, 100, 1600, dict(filtering=True, forced="rows")), dict(bitmap_rows=1, rows=1)),
    # column panels: NP = ceil(B / panel), at most W; PW = ceil(W / NP); NP again = ceil(W / PW)
    ((650, 73, 650, 1, 1, 1, dict(b_bytes_est=2_500_000, panel_mb=1)), dict(W=21, NP=3, PW=7)),
    ((650, 73, 650, 1, 1, 1, dict(b_bytes_est=2_500_000)), dict(NP=1, PW=21)),
    ((650, 73, 650, 1, 1, 1, dict(b_bytes_est=0, panel_mb=1)), dict(NP=1, PW=21)),
    ((100, 10, 128, 1, 1, 1, dict(b_bytes_est=100 << 20, panel_mb=1)), dict(W=4, NP=4, PW=1)),              # clamped to W
    ((100, 10, 320, 1, 1, 1, dict(b_bytes_est=6 << 20, panel_mb=1)), dict(W=10, NP=5, PW=2)),               # 6 panels of 2 words are 5
    ((100, 10, 320, 1, 1, 1, dict(b_bytes_est=4 << 20, panel_mb=1)), dict(W=10, NP=4, PW=3)),               # the last panel has one word
    ((100, 10, 810, 1, 1, 1, dict(b_bytes_est=(5 << 20) + 1, panel_mb=1)), dict(W=26, NP=6, PW=5)),
    ((100, 10, 810, 1, 1, 1, dict(b_bytes_est=1 << 20, panel_mb=1)), dict(NP=1, PW=26)),
    ((100, 10, 810, 1, 1, 1, dict(b_bytes_est=(1 << 20) + 1, panel_mb=1)), dict(NP=2, PW=13)),
    ((100, 10, 810, 1, 1, 1, dict(b_bytes_est=(1 << 20) + 1, panel_mb=0)), dict(NP=2, PW=13)),              # DBCSR_AMD_MM_PANEL_MB=0 is 1 MB
]


@pytest.mark.parametrize("row", range(len(TABLE)))
def test_choose_symbolic_table(shim, row):
    (nbr, nbk, nbc, a, b, c, kw), want = TABLE[row]
    got = S.symbolic_choice(shim, nbr, nbk, nbc, a, b, c, **kw)
    assert {k: got[k] for k in want} == want, (TABLE[row], got)


def test_panel_size_of_zero_is_clamped(shim):
    """DBCSR_AMD_MM_PANEL_MB=0 (and DBCSR_AMD_MM_GROUP_PANEL_MB=0) made panel_bytes 0, and the panel count divides by it"""
    assert shim.panel_bytes(0) == 1 << 20 and shim.panel_bytes(-7) == 1 << 20 and shim.panel_bytes(1) == 1 << 20
    assert shim.panel_bytes(256) == 256 << 20 and shim.panel_bytes(4096) == 4096 << 20
    import os
    env = open(os.path.join(CSRC, "mm_engine_env.h")).read()
    assert env.count("panel_bytes_of_mb(atoll(k))") == 2 and "atoll(k) << 20" not in env


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.NAMES)
def test_case_meets_its_conditions(shim, shims, name):  # noqa: F811
    case = S.BY_NAME[name]
    t0 = time.perf_counter()
    failed = S.conditions(case, shim, class_mode(shims, case))
    n, ref = S.counts(case), S.reference(case)
    print("%s: nbr %d nbc %d C blocks %d (symbolic %d) products %d of %d; %s; host %.2f s" % (
        name, n["nbr"], n["nbc"], ref.C.nblks, n["c_nblks"], ref.nproducts, ref.nproducts_unfiltered,
        S.line_of(S.predicted(case, shim, class_mode(shims, case))), time.perf_counter() - t0))
    assert not failed, failed


def test_every_branch_of_the_table_is_reached_without_a_forcing_variable(shim, shims):  # noqa: F811
    """each branch by itself (DBCSR_AMD_MM_SYMBOLIC is in no case's switches; the panel cases need DBCSR_AMD_MM_PANEL_MB)"""
    assert not any("DBCSR_AMD_MM_SYMBOLIC" in c["env"] for c in S.CASES)
    seen = [dict(S.predicted(c, shim, class_mode(shims, c)), c_nblks=S.counts(c)["c_nblks"], nbr=S.counts(c)["nbr"]) for c in S.CASES]
    assert any(p["count"] == "rows" and p["bitmap"] == "plain" for p in seen)
    assert any(p["bitmap"] == "rows_filtered" for p in seen)
    assert any(p["bitmap"] == "filtered" and p["count"] == "rows" for p in seen)
    assert any(p["count"] == "word" and p["nbr"] < 2048 for p in seen)
    assert any(p["W"] > 64 for p in seen) and any(p["rowp_chunks"] > 1 for p in seen) and any(p["c_nblks"] > 1048576 for p in seen)
    assert any(p["NP"] > 1 and p["W"] % p["NP"] != 0 and p["classes"] == 0 for p in seen)
    assert any(p["NP"] >= 3 and p["W"] % p["NP"] != 0 and p["classes"] == 1 and p["nbr"] > 512 for p in seen)


def test_the_bar_notices_one_wrong_element():
    """the comparison is element-wise: one element off by 1e-9 of its size, a block moved by one column, a product count off by one are all caught"""
    case = S.BY_NAME["thr_2047-NN-f64"]
    ref = S.reference(case)
    same = S.bcsr(ref.C, ref.C.data.copy())
    assert S.compare(case, same, ref.flop, ref.nproducts)[0] is None
    w = int(np.argmax(np.abs(ref.C.data)))
    off = S.bcsr(ref.C, ref.C.data.copy())
    off.data[w] *= 1 + 1e-9
    assert S.compare(case, off, ref.flop, ref.nproducts)[0]["what"] == "values"
    moved = S.bcsr(ref.C, ref.C.data)
    moved.col_i = ref.C.col_i.copy()
    moved.col_i[-1] += 1
    assert S.compare(case, moved, ref.flop, ref.nproducts)[0]["what"] == "col_i"
    assert S.compare(case, same, ref.flop, ref.nproducts + 1)[0]["what"] == "nproducts"
    assert S.compare(case, same, ref.flop + 2, ref.nproducts)[0]["what"] == "flop"


# ---- the launch order, restated ---------------------------------------------------------------------------------------------------------------------------------
def first_of_group(group):
    """for a non-decreasing key per block: the index of the first block with the block's key"""
    _, first, inv = np.unique(group, return_index=True, return_inverse=True)
    return first[inv]


def order_plain(C, PW, NP, w0_shift=0):
    """order_count + exclusive scan + order_len + order_fill of mm_symbolic.h (one row per group, RG = 1): key = (x NP + p) NG + g for row i = 8 g + x and
    panel p = w / PW; a block's place is its rank among the blocks of its row inside the panel.  w0_shift = 1: the panel's first word off by one."""
    nbr, W = C.nbr, (C.nbc + 31) // 32
    NG = (nbr + 7) // 8
    rows, cb = C.rows().astype(np.int64), np.arange(C.nblks)
    p = (C.col_i >> 5) // PW
    key = ((rows & 7) * NP + p) * NG + (rows >> 3)
    base = np.concatenate([[0], np.cumsum(np.bincount(key, minlength=8 * NP * NG))])
    per_x = base[(np.arange(8) + 1) * NP * NG] - base[np.arange(8) * NP * NG]
    length = (int(per_x.max()) + 3) & ~3
    w0 = np.minimum(p * PW + w0_shift, W)
    span = 32 * W + 64
    left_of_panel = np.searchsorted(rows * span + C.col_i, rows * span + 32 * w0) - C.row_p[rows]   # panel_rank: blocks of the row left of word w0
    rank = (cb - C.row_p[rows]) - left_of_panel
    order = np.full(8 * length + 64, -1, np.int64)
    dst = (rows & 7) * length + (base[key] - base[(rows & 7) * NP * NG]) + rank
    ok = (dst >= 0) & (dst < order.size)
    order[dst[ok]] = cb[ok]
    return order


def top3(sizes):
    hist = np.bincount(sizes, minlength=33)[:33]
    out, used = [], []
    for _ in range(3):
        best, bc = 0, 0
        for s in range(1, 33):
            if hist[s] > bc and s not in used:
                best, bc = s, hist[s]
        out.append(best)
        used.append(best if best else -1)
    return out


def order_classes(C, PW, NP):
    """class_ids, class_row_deal, order_count_cls, order_len_cls, order_fill_cls: ten segments, each eight streams padded to a common multiple of 32"""
    nbr = C.nbr
    R = (nbr + 7) // 8
    rank_of = lambda sizes: (lambda t: np.select([sizes == t[0], sizes == t[1], sizes == t[2]], [0, 1, 2], 3))(top3(sizes))
    rc, cc = rank_of(C.row_sizes), rank_of(C.col_sizes)
    vpos = np.empty(nbr, np.int64)
    vpos[np.argsort(rc, kind="stable")] = np.arange(nbr)   # rows numbered again, class after class in row order
    rows, cb = C.rows().astype(np.int64), np.arange(C.nblks)
    p = (C.col_i >> 5) // PW
    q = np.where(rc[rows] == 3, 3, cc[C.col_i])
    cls = np.where((rc[rows] < 3) & (q < 3), rc[rows] * 3 + q, 9)
    j = vpos[rows]
    key0 = (cls * 8 + (j & 7)) * NP * R
    key = key0 + p * R + (j >> 3)
    base = np.concatenate([[0], np.cumsum(np.bincount(key, minlength=10 * 8 * NP * R))])
    stream = base[(np.arange(80) + 1) * NP * R] - base[np.arange(80) * NP * R]
    lens = (stream.reshape(10, 8).max(axis=1) + 31) & ~31
    offs = np.concatenate([[0], np.cumsum(8 * lens)])
    # rank among the blocks of the same row, panel and class: blocks are sorted by (row, column), so sort by (row, panel, class) keeping that order
    g = (rows * NP + p) * 10 + cls
    srt = np.argsort(g, kind="stable")
    rank = np.empty(C.nblks, np.int64)
    rank[srt] = np.arange(C.nblks) - first_of_group(g[srt])
    order = np.full(int(offs[-1]) + 64, -1, np.int64)
    order[offs[cls] + (j & 7) * lens[cls] + (base[key] - base[key0]) + rank] = cb
    return order, lens


def is_permutation_with_padding(order, n):
    real = order[order >= 0]
    return real.size == n and np.array_equal(np.sort(real), np.arange(n)) and np.all(order[order < 0] == -1)


@pytest.mark.parametrize("name", ["panels_small-NN-f64-classes0-mb1", "wide-NT-f64", "empty_rows-NN-f64", "classes_panels-NN-f64-classes2-mb1"])
def test_launch_order_is_a_permutation_of_the_c_blocks(name):
    C = S.reference(S.BY_NAME[name]).C
    W = (C.nbc + 31) // 32
    for NP0 in (1, 3, W):
        PW = (W + NP0 - 1) // NP0
        NP = (W + PW - 1) // PW
        assert is_permutation_with_padding(order_plain(C, PW, NP), C.nblks), (name, NP)
        order, lens = order_classes(C, PW, NP)
        assert is_permutation_with_padding(order, C.nblks) and np.all(lens % 32 == 0), (name, NP)
    # the restatement is sharp: with the first word of a panel off by one (p PW + 1 for w0) blocks collide or leave their stream
    PW = (W + 2) // 3
    if C.nblks > 1000:
        assert not is_permutation_with_padding(order_plain(C, PW, (W + PW - 1) // PW, w0_shift=1), C.nblks)
