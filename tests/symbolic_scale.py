"""The symbolic phase at the block counts where its paths change: seeded multiplies of MANY SMALL BLOCKS (1 ... 3 elements per dimension; 5 / 13 / 23 for the
class cases), with the reference, the bar and the conditions on the inputs.  tests/test_symbolic_scale_cpu.py checks all of it without a GPU;
tests/test_gpu_symbolic_scale.py runs every case on the device.  Nothing here touches a GPU.

WHY.  dbcsr_amd/csrc/mm_symbolic.h and the set-up in dbcsr_amd_mm_symbolic_filtered choose their kernels by the number of block rows, block columns and C
blocks (mm_choose.h: choose_symbolic_pattern / choose_symbolic_count / choose_panels), and the scans and prefixes change their path at 4096 rows
(exclusive_scan's second chunk), 64 bitmap words (row_prefix's carry), 1 048 576 C blocks (scan_partials' second trip) and at B above the panel size
(several column panels).  None of that needs big matrices: 4267 block rows of 1 ... 2 elements are a 6400-row matrix the CPU oracle multiplies in 0.1 s.

THE REFERENCE.  Index (row_p, col_i, blk_p), flop and the product count: the oracle's (O.multiply), exact.  Values: the oracle's fp64 result, element by
element.  Complex data: the oracle on the real and imaginary parts (four real multiplies, real alpha and beta).

THE BAR, element-wise: |got - ref| <= 2 gamma (|alpha| (|A| |B|) + |beta| |C_in|).  gamma = (n + 8) u / (1 - (n + 8) u) with n the elements of the inner
dimension and u = 2^-53 (fp64) / 2^-24 (fp32), the bound of tests/option_sweep.py for a sum of n products in any order; complex128: sqrt(2) (2 n + 10) 2^-53.
The factor 2 because the reference is itself an fp64 sum within gamma.  The absolute-value product is an oracle multiply of |A|, |B|, |C_in| with |alpha|,
|beta| and no filter, looked up by block coordinate (its pattern contains the result's).  Derived, not measured: a case above it is a finding.

CONDITIONS.  conditions(case, shim, cls_mode) names what a case fails of: the path mm_choose.h gives for the oracle's counts is the one the case means to reach; the
sizes it claims (nbr > 4096, W > 64, ...) hold; C has blocks in the columns on both sides of the 64-word boundary; a filtered case drops at least 5 % and
keeps at least 5 % of its products.  A case that fails one is given another seed (`counter`), not skipped."""
import ctypes
import functools

import numpy as np

from oracle import oracle as O

F64, F32, Z64 = "float64", "float32", "complex128"
U = {F64: 2.0 ** -53, F32: 2.0 ** -24}
SCAN_CHUNK = 4096   # mm_workspace.h: kScanChunk

A12, B3 = [1, 1, 1, 2], [1, 3]
C3 = [1, 5, 1, 13, 1, 23]
SHAPES = {
    # name: M, N, K, (sparsity of A, B, C_in), block-size mixes of m, n, k
    "tall": (6400, 120, 200, (0.9, 0.5, 0.97), A12, B3, [1, 2, 1, 5]),                       # nbr 4267, nbc 40
    "wide": (120, 6400, 200, (0.5, 0.9, 0.97), B3, A12, [1, 2, 1, 5]),                       # nbr 40, nbc 4267, W 134
    "square_sparse": (6400, 6400, 150, (0.97, 0.97, 0.999), A12, A12, B3),                   # 4267 x 4267, C 4 % full
    "square_dense": (4500, 4500, 300, (0.8, 0.8, 0.9), [1, 2], [1, 2], [1, 2]),              # 2250 x 2250, 5 M C blocks
    "panels_small": (2600, 2600, 400, (0.7, 0.7, 0.9), [1, 5, 1, 3], [1, 5, 1, 3], [1, 4, 1, 7]),   # 650 x 650, B 2.5 MB
    "very_sparse": (3000, 6400, 150, (0.995, 0.995, 0.9998), A12, A12, B3),                  # nbr 2000, nbc 4267: the per-word kernels
    "classes_panels": (41 * 270, 41 * 270, 41 * 30, (0.985, 0.95, 0.99), C3, C3, C3),        # 810 x 810 of 5 / 13 / 23, B 5 MB
    "thr_2047": (3070, 3072, 150, (0.97, 0.97, 0.999), A12, A12, B3),
    "thr_2048": (3072, 3072, 150, (0.97, 0.97, 0.999), A12, A12, B3),
    "empty_rows": (450, 217, 90, (0.9, 0.8, 0.98), A12, A12, B3),                            # nbr 300, nbc 145 = 2 x 64 + 17
}
EMPTY_HEAD, EMPTY_TAIL = 3, 2   # block rows of A and C_in of "empty_rows" that are emptied


def _case(shape, t="NN", dtype=F64, alpha=-0.5, beta=1.5, retain=False, eps=0.0, cin="holes", env=None, counter=0, native=False, **expect):
    name = "%s-%s-%s" % (shape, t, {F64: "f64", F32: "f32", Z64: "z64"}[dtype])
    name += ("-retain" if retain else "") + ("-eps" if eps else "") + ("-empty_cin" if cin == "empty" else "")
    name += "".join("-%s%s" % (k.split("_")[-1].lower(), v) for k, v in sorted((env or {}).items()))
    return dict(name=name, shape=shape, ta=t[0], tb=t[1], dtype=dtype, alpha=alpha, beta=(0.0 if cin == "empty" else beta), retain=retain, eps=eps, cin=cin,
                env=dict(env or {}), counter=counter, native=native, expect=expect)


PANEL1 = {"DBCSR_AMD_MM_PANEL_MB": "1"}
# expect: the fields of last_symbolic() the case is there for (the whole line is predicted from mm_choose.h), and `claims`, evaluated by conditions()
CASES = [
    _case("tall", "NN", count="grid", rowp_chunks=2, claims=("nbr > 4096",), native=True),
    _case("tall", "TN", F32, alpha=1.0, beta=1.0, count="grid", rowp_chunks=2, claims=("nbr > 4096",)),
    _case("tall", "NN", retain=True, count="rows", rowp_chunks=2),   # (C keeps C_in's 5086 blocks: sparse)
    _case("wide", "NT", count="grid", claims=("W > 64",), native=True),
    _case("wide", "NN", F32, alpha=1.0, beta=-1.5, count="grid", claims=("W > 64",)),
    _case("square_sparse", "NN", bitmap="plain", count="rows", rowp_chunks=2, claims=("nbr > 4096", "W > 64"), native=True),
    _case("square_sparse", "TN", retain=True, count="rows", rowp_chunks=2),
    _case("square_sparse", "NT", cin="empty", count="rows", rowp_chunks=2),
    _case("square_sparse", "NN", Z64, count="rows", rowp_chunks=2, native=True),
    _case("square_sparse", "NN", eps=0.5, bitmap="rows_filtered", count="rows", rowp_chunks=2, claims=("nbr > 4096", "W > 64"), native=True),
    _case("square_dense", "NN", alpha=1.0, beta=1.0, count="grid", claims=("c_nblks > 1048576",)),
    # (without the size histograms B is sized by its largest block, 7 x 5: 4 MB, four panels of 6 words for W = 21)
    _case("panels_small", "NN", env=dict(PANEL1, DBCSR_AMD_MM_CLASSES="0"), count="grid", NP=4, PW=6, classes=0, claims=("NP > 1", "W % NP != 0"), native=True),
    _case("panels_small", "TN", env=PANEL1, count="grid", NP=3, PW=7, classes=1, claims=("NP > 1",)),
    # (counter: the seeds before it leave no C block in column 2047 or 2048)
    _case("very_sparse", "NN", counter=2, count="word", claims=("nbr < 2048", "nbc > 2048", "W > 64")),
    _case("very_sparse", "NT", cin="empty", counter=17, count="word"),
    _case("classes_panels", "NN", env=dict(PANEL1, DBCSR_AMD_MM_CLASSES="2"), classes=1, claims=("nbr >= 800", "NP >= 3", "W % NP != 0"), native=True),
    _case("thr_2047", "NN", count="grid", claims=("nbr == 2047",)),
    _case("thr_2048", "NN", count="rows", claims=("nbr == 2048",)),
    _case("thr_2047", "NN", eps=0.5, bitmap="filtered", count="grid"),
    _case("thr_2048", "NN", eps=0.5, bitmap="rows_filtered", count="rows", native=True),
    _case("thr_2048", "NN", eps=0.5, retain=True, bitmap="filtered", count="rows"),
    _case("empty_rows", "NN", count="grid", claims=("empty rows at both ends", "nbc % 64 in 1..31")),
    _case("empty_rows", "NN", eps=0.8, bitmap="filtered", count="grid", claims=("empty rows at both ends", "nbc % 64 in 1..31")),
]
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
NAMES = [c["name"] for c in CASES]


# ---- operands ---------------------------------------------------------------------------------------------------------------------------------------------
def bcsr(M, data):
    return O.Bcsr(M.row_sizes, M.col_sizes, M.row_p, M.col_i, M.blk_p, data)


def without_rows(M, rows):
    """M without the blocks of the given block rows (the others keep their order; the data area is packed again)"""
    keep = ~np.isin(M.rows(), rows)
    size = M.row_sizes[M.rows()].astype(np.int64) * M.col_sizes[M.col_i]
    cnt = np.bincount(M.rows()[keep], minlength=M.nbr)
    src = np.concatenate([np.arange(p, p + s) for p, s in zip(M.blk_p[keep], size[keep])]) if keep.any() else np.zeros(0, np.int64)
    blk_p = np.concatenate([[0], np.cumsum(size[keep])[:-1]]) if keep.any() else np.zeros(0, np.int64)
    return O.Bcsr(M.row_sizes, M.col_sizes, np.concatenate([[0], np.cumsum(cnt)]), M.col_i[keep], blk_p, M.data[src])


def empty_like(M):
    return O.Bcsr(M.row_sizes, M.col_sizes, np.zeros(M.nbr + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros(0, M.data.dtype))


def with_imag(M, seed):
    """uniform(-1, 1) imaginary parts laid over the oracle's real matrix"""
    im = np.random.default_rng(seed).uniform(-1.0, 1.0, M.data.size)
    return bcsr(M, (M.data + 1j * im).astype(np.complex128))


@functools.lru_cache(maxsize=None)
def _stored(shape, ta, tb, dtype, cin, counter):
    M, N, K, sp, mm, mn, mk = SHAPES[shape]
    rdt = np.float32 if dtype == F32 else np.float64
    sm, sn, sk = O.make_block_sizes(M, mm), O.make_block_sizes(N, mn), O.make_block_sizes(K, mk)
    c0 = O.RANDMAT_SEED_INIT + 10 * counter
    Cm = O.make_random_matrix(sm, sn, sp[2], c0 + 1, rdt)
    A = O.make_random_matrix(sk, sm, sp[0], c0 + 2, rdt) if ta != "N" else O.make_random_matrix(sm, sk, sp[0], c0 + 2, rdt)
    B = O.make_random_matrix(sn, sk, sp[1], c0 + 3, rdt) if tb != "N" else O.make_random_matrix(sk, sn, sp[1], c0 + 3, rdt)
    if shape == "empty_rows":
        gone = np.concatenate([np.arange(EMPTY_HEAD), np.arange(A.nbr - EMPTY_TAIL, A.nbr)])
        A, Cm = without_rows(A, gone), without_rows(Cm, gone)
    if cin == "empty":
        Cm = empty_like(Cm)
    if dtype == Z64:
        A, B, Cm = with_imag(A, 3 * counter + 1), with_imag(B, 3 * counter + 2), with_imag(Cm, 3 * counter + 3)
    return A, B, Cm


def operands(case):
    """(A, B, C_in) on the host as they are stored, in the case's data type: computed once per (shape, transposes, type), never written"""
    return _stored(case["shape"], case["ta"], case["tb"], case["dtype"], case["cin"], case["counter"])


def inner_elements(case):
    return SHAPES[case["shape"]][2]


def gamma_of(case):
    n = inner_elements(case)
    if case["dtype"] == Z64:
        return float(np.sqrt(2.0) * (2 * n + 10) * 2.0 ** -53)
    u = U[case["dtype"]]
    return (n + 8) * u / (1.0 - (n + 8) * u)


# ---- the reference ------------------------------------------------------------------------------------------------------------------------------------------
def _f64(M, data=None):
    return bcsr(M, np.ascontiguousarray(M.data if data is None else data, np.float64))


class Reference:
    """what reference() returns: C (the result: float64 values, complex128 for complex data), flop, nproducts, bar (one value per element of C.data:
    2 gamma x the absolute-value product at the element), nproducts_unfiltered"""


@functools.lru_cache(maxsize=None)
def _reference(name):
    case = BY_NAME[name]
    A, B, Cm = operands(case)
    ta, tb, al, be, kw = case["ta"], case["tb"], case["alpha"], case["beta"], dict(retain_sparsity=case["retain"], filter_eps=case["eps"])
    out = Reference()
    if case["dtype"] == Z64:
        assert case["eps"] == 0, "the complex reference has no filter"
        re_, im_ = (lambda M: _f64(M, M.data.real)), (lambda M: _f64(M, M.data.imag))
        x, info1 = O.multiply(ta, tb, al, re_(A), re_(B), be, re_(Cm), **kw)
        cr, info2 = O.multiply(ta, tb, -al, im_(A), im_(B), 1.0, x, **kw)
        y, _ = O.multiply(ta, tb, al, re_(A), im_(B), be, im_(Cm), **kw)
        ci, _ = O.multiply(ta, tb, al, im_(A), re_(B), 1.0, y, **kw)
        assert np.array_equal(cr.col_i, ci.col_i) and np.array_equal(cr.blk_p, ci.blk_p) and info1["flop"] == info2["flop"]
        out.C, info = bcsr(cr, cr.data + 1j * ci.data), info1
        flop = int(info["flop"])   # (counted as the reference counts it: 2 m n k per block product, whatever the data type)
    else:
        out.C, info = O.multiply(ta, tb, al, _f64(A), _f64(B), be, _f64(Cm), **kw)
        flop = int(info["flop"])
    out.flop, out.nproducts = flop, int(info["nproducts"])
    ab, binfo = O.multiply(ta, tb, abs(al), _f64(A, np.abs(A.data)), _f64(B, np.abs(B.data)), abs(be), _f64(Cm, np.abs(Cm.data)),
                           retain_sparsity=case["retain"])
    out.nproducts_unfiltered = int(binfo["nproducts"])
    # the absolute-value product at the result's blocks, by block coordinate
    key = lambda M: M.rows().astype(np.int64) * M.nbc + M.col_i
    at = np.searchsorted(key(ab), key(out.C))
    assert at.size == 0 or (at.max() < ab.nblks and np.array_equal(key(ab)[at], key(out.C))), "the absolute-value product lacks a block of the result"
    size = out.C.row_sizes[out.C.rows()].astype(np.int64) * out.C.col_sizes[out.C.col_i]
    start = np.concatenate([[0], np.cumsum(size)])
    within = np.arange(int(start[-1])) - np.repeat(start[:-1], size)
    bar = np.zeros(out.C.data.size)
    bar[np.repeat(out.C.blk_p, size) + within] = 2.0 * gamma_of(case) * ab.data[np.repeat(ab.blk_p[at], size) + within]
    out.bar = bar
    return out


def reference(case):
    return _reference(case["name"])


def compare(case, got, flop, nproducts):
    """None when the device result (a host Bcsr), its flop and product counts meet the reference, else a dict that says what differs.  Second value:
    the worst err / bar."""
    ref = reference(case)
    for f in ("row_p", "col_i", "blk_p"):
        if not np.array_equal(getattr(got, f), getattr(ref.C, f)):
            return {"what": f, "device": int(getattr(got, f).size), "reference": int(getattr(ref.C, f).size)}, 0.0
    if int(flop) != ref.flop:
        return {"what": "flop", "device": int(flop), "reference": ref.flop}, 0.0
    if nproducts is not None and int(nproducts) != ref.nproducts:   # (the C entry reports flop only)
        return {"what": "nproducts", "device": int(nproducts), "reference": ref.nproducts}, 0.0
    if got.data.size != ref.C.data.size:
        return {"what": "data size", "device": int(got.data.size), "reference": int(ref.C.data.size)}, 0.0
    err = np.abs(got.data.astype(ref.C.data.dtype) - ref.C.data)
    ratio = np.where(ref.bar > 0, err / np.where(ref.bar > 0, ref.bar, 1), np.where(err > 0, np.inf, 0.0))
    if ratio.size == 0:
        return None, 0.0
    w = int(np.argmax(np.where(np.isnan(ratio), np.inf, ratio)))
    worst = float(ratio[w])
    if not worst <= 1.0:
        return {"what": "values", "element": w, "error": float(err[w]), "bar": float(ref.bar[w]), "count_above_bar": int(np.sum(~(ratio <= 1.0)))}, worst
    return None, worst


# ---- what mm_choose.h chooses for a case ------------------------------------------------------------------------------------------------------------------------
SHIM = """
#include "mm_choose.h"
using namespace dbcsr_amd;
// in: nbr nbk nbc a_nblks b_nblks filtering retain forced c_nblks W b_bytes_est panel_bytes -> out: sparse_guess bitmap_rows grid rows NP PW
extern "C" void symbolic_choice(const long long* in, long long* out) {
  SymbolicSizes s;
  s.nbr = (int)in[0], s.nbk = (int)in[1], s.nbc = (int)in[2], s.a_nblks = in[3], s.b_nblks = in[4];
  s.filtering = in[5] != 0, s.retain = in[6] != 0, s.forced = (int)in[7];
  SymbolicChoice c = choose_symbolic_pattern(s);
  out[0] = c.sparse_guess, out[1] = c.bitmap_rows;
  c = choose_symbolic_count(s, c, in[8]);
  out[2] = c.grid_kernels, out[3] = c.rows_kernels;
  int NP = 0, PW = 0;
  choose_panels((int)in[9], in[10], in[11], &NP, &PW);
  out[4] = NP, out[5] = PW;
}
extern "C" long long panel_bytes(long long mb) { return panel_bytes_of_mb(mb); }
"""
FORCED = {None: 0, "word": 1, "grid": 2, "rows": 3}


def symbolic_choice(shim, nbr, nbk, nbc, a_nblks, b_nblks, c_nblks, filtering=False, retain=False, forced=None, b_bytes_est=0, panel_mb=256):
    """choose_symbolic_pattern + choose_symbolic_count + choose_panels of the host build of mm_choose.h, as a dict"""
    W = (nbc + 31) // 32
    a = (ctypes.c_longlong * 12)(nbr, nbk, nbc, a_nblks, b_nblks, int(filtering), int(retain), FORCED[forced], c_nblks, W, int(b_bytes_est),
                                 int(shim.panel_bytes(ctypes.c_longlong(panel_mb))))
    out = (ctypes.c_longlong * 6)()
    shim.symbolic_choice(a, out)
    return dict(zip(("sparse_guess", "bitmap_rows", "grid", "rows", "NP", "PW"), (int(v) for v in out)), W=W)


def b_bytes_est(B_op, use_classes=1):
    """dbcsr_amd_mm_symbolic_filtered: B's size from the mean block sizes when the histograms are at hand (sizes within 1 ... 32), else from the maxima"""
    ks, ns = B_op.row_sizes, B_op.col_sizes
    mean_k, mean_n = float(ks.max()), float(ns.max())
    if use_classes > 0 and ks.max() <= 32 and ns.max() <= 32 and ks.min() >= 1 and ns.min() >= 1:
        mean_k, mean_n = float(ks.astype(np.int64).sum()) / ks.size, float(ns.astype(np.int64).sum()) / ns.size
    return int(float(B_op.nblks) * mean_k * mean_n * 8.0)


def oriented(case):
    """(op(A), op(B), C_in): the operands as the symbolic phase sees them"""
    A, B, Cm = operands(case)
    return (O.transposed(A) if case["ta"] != "N" else A), (O.transposed(B) if case["tb"] != "N" else B), Cm


@functools.lru_cache(maxsize=None)
def _counts(name):
    case = BY_NAME[name]
    A, B, Cm = oriented(case)
    ref = reference(case)
    # C blocks the symbolic phase counts: before the final filter drops blocks (a filtered multiply that does not retain), so not the result's
    if case["eps"] > 0 and not case["retain"]:
        c_nblks = symbolic_blocks(case)
    else:
        c_nblks = ref.C.nblks
    return dict(nbr=A.nbr, nbk=A.nbc, nbc=B.nbc, a_nblks=A.nblks, b_nblks=B.nblks, c_nblks=int(c_nblks), b_bytes=b_bytes_est(B, int(case["env"].get("DBCSR_AMD_MM_CLASSES", "1"))))


def symbolic_blocks(case):
    """C blocks of a filtered multiply before its final filter: C_in's blocks and those that receive a product the on-the-fly filter keeps
    (oracle/dbcsr_oracle.c: fp32 block norms of fp64 sums, the row's eps = eps / max(1, blocks of A's row))"""
    A, B, Cm = oriented(case)
    na = np.add.reduceat(np.square(A.data.astype(np.float64)), A.blk_p).astype(np.float32) if A.nblks else np.zeros(0, np.float32)
    nb = np.add.reduceat(np.square(case["alpha"] * B.data.astype(np.float64)), B.blk_p).astype(np.float32) if B.nblks else np.zeros(0, np.float32)
    per_row = np.maximum(np.diff(A.row_p), 1).astype(np.float32)
    e = np.float32(case["eps"]) / per_row
    reps = (e * e).astype(np.float32)[A.rows()]
    cnt = np.diff(B.row_p)[A.col_i]
    ia = np.repeat(np.arange(A.nblks), cnt)
    start = np.concatenate([[0], np.cumsum(cnt)])
    ib = np.repeat(B.row_p[A.col_i].astype(np.int64), cnt) + (np.arange(int(start[-1])) - np.repeat(start[:-1], cnt))
    kept = ~((na[ia] * nb[ib]).astype(np.float32) < reps[ia])
    keys = A.rows()[ia][kept].astype(np.int64) * B.nbc + B.col_i[ib][kept]
    return int(np.union1d(keys, Cm.rows().astype(np.int64) * Cm.nbc + Cm.col_i).size)


def counts(case):
    return _counts(case["name"])


def predicted(case, shim, cls_mode, env=None):
    """the fields of last_symbolic() mm_choose.h gives for the oracle's counts of the case (env: the variant's switches instead of the case's own)"""
    env = case["env"] if env is None else env
    n = counts(case)
    ch = symbolic_choice(shim, n["nbr"], n["nbk"], n["nbc"], n["a_nblks"], n["b_nblks"], n["c_nblks"], filtering=case["eps"] > 0, retain=case["retain"],
                         forced=env.get("DBCSR_AMD_MM_SYMBOLIC"), b_bytes_est=n["b_bytes"], panel_mb=int(env.get("DBCSR_AMD_MM_PANEL_MB", "256")))
    return dict(bitmap="rows_filtered" if ch["bitmap_rows"] else ("filtered" if case["eps"] > 0 else "plain"),
                count="rows" if ch["rows"] else ("grid" if ch["grid"] else "word"), W=ch["W"], NP=ch["NP"], PW=ch["PW"], classes=int(cls_mode),
                rowp_chunks=(n["nbr"] + SCAN_CHUNK - 1) // SCAN_CHUNK)


def line_of(fields, plan="miss"):
    return "bitmap=%(bitmap)s count=%(count)s W=%(W)d NP=%(NP)d PW=%(PW)d classes=%(classes)d rowp_chunks=%(rowp_chunks)d" % fields + " plan=" + plan


def parse_line(line):
    return {k: (v if k in ("bitmap", "count", "plan") else int(v)) for k, v in (f.split("=") for f in line.split())}


def choice_query(case):
    """(case tuple, keyword facts) for `choose` of tests/test_numeric_choice.py: the numeric kernel and the class mode of the case (real data)"""
    M, N, K, sp, mm, mn, mk = SHAPES[case["shape"]]
    n, ref = counts(case), reference(case)
    unfiltered = max(1, n["c_nblks"])
    return (M, N, K, 0, 0, 0, mm, mn, mk), dict(c_nblks=unfiltered, products_per_block=ref.nproducts / unfiltered, fp64=case["dtype"] != F32,
                                                retain=bool(case["retain"]), filter_active=case["eps"] > 0)


# ---- conditions on the inputs --------------------------------------------------------------------------------------------------------------------------------
def conditions(case, shim, cls_mode):
    """the names of the conditions the case fails (empty: a good case)"""
    n, ref, got = counts(case), reference(case), predicted(case, shim, cls_mode)
    failed = []
    for k, v in case["expect"].items():
        if k != "claims" and got[k] != v:
            failed.append("mm_choose.h gives %s=%s, the case means %s" % (k, got[k], v))
    W, NP, nbr, nbc, c_nblks = got["W"], got["NP"], n["nbr"], n["nbc"], n["c_nblks"]
    C = ref.C
    for claim in case["expect"].get("claims", ()):
        if claim == "empty rows at both ends":
            per_row = np.diff(C.row_p)
            ok = C.nblks > 0 and not per_row[:EMPTY_HEAD].any() and not per_row[-EMPTY_TAIL:].any() and per_row[EMPTY_HEAD] > 0 and per_row[-EMPTY_TAIL - 1] > 0
        elif claim == "nbc % 64 in 1..31":
            ok = 1 <= nbc % 64 <= 31 and nbc % 32 != 0
        else:
            ok = bool(eval(claim, {}, dict(W=W, NP=NP, nbr=nbr, nbc=nbc, c_nblks=c_nblks)))
        if not ok:
            failed.append("the claim does not hold: " + claim)
    if W > 64 and not (np.any(C.col_i == 2047) and np.any(C.col_i == 2048)):
        failed.append("no C block in column 2047 or 2048 (the boundary of row_prefix's chunks of 64 words)")
    if case["eps"] > 0:
        kept = ref.nproducts / max(1, ref.nproducts_unfiltered)
        if not 0.05 <= kept <= 0.95:
            failed.append("the filter keeps %.1f %% of the products" % (100 * kept))
    return failed
