"""Block-sparse tensors restated in numpy, independently of dbcsr_amd/tensor.py: what the tests of the tensor interface compare against.

A tensor is a dict {block index tuple: nd array of the block's extents} plus, per dimension, the block sizes.  The semantics are those of dense numpy
arrays (the reference's sources are not at hand):

    dense_of / blocks_of          dict of blocks <-> dense nd array
    block_row_col, folded_sizes   the mapping formulas: block (i_0 ... i_{r-1}) lies in block row R = i_{map1[0]} + nb_{map1[0]} (i_{map1[1]} + ...), the first
                                  entry of map1 fastest, the block column likewise from map2; row / column block sizes are products of the sizes
    stored_block                  the stored form of a block: its Fortran array with the dimensions in the order map1 ++ map2
    matrix_of / blocks_of_matrix  dict of blocks <-> the packed matrix (row_p, col_i, blk_p, data) of the mapping
    contract_pattern              the pattern of a contraction as a boolean product
    contract_dense                the values by np.einsum in longdouble / clongdouble on dense arrays
    contract                      the contraction block by block as dbcsr_multiply runs it: kept products (the on-the-fly rule of tests/option_sweep.py's
                                  restate when filter_eps is given), the final filter, retain_sparsity, the flop count, the values and the bound of DESIGN 4c"""
import itertools

import numpy as np

LD, CLD = np.longdouble, np.clongdouble


def wide(dtype):
    return CLD if np.dtype(dtype).kind == "c" else LD


def starts(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, np.int64))])


def extents(index, blk_sizes):
    return tuple(int(blk_sizes[d][i]) for d, i in enumerate(index))


def dense_of(blocks, blk_sizes, dtype):
    off = [starts(s) for s in blk_sizes]
    D = np.zeros([int(o[-1]) for o in off], dtype)
    for index, blk in blocks.items():
        assert blk.shape == extents(index, blk_sizes)
        D[tuple(slice(int(off[d][i]), int(off[d][i + 1])) for d, i in enumerate(index))] = blk
    return D


def blocks_of(D, blk_sizes, indices):
    off = [starts(s) for s in blk_sizes]
    return {tuple(ix): D[tuple(slice(int(off[d][i]), int(off[d][i + 1])) for d, i in enumerate(ix))].copy() for ix in indices}


def block_row_col(index, nblks, map1, map2):
    """(R, C) of a block, by Horner from the slowest entry of each tuple down to the fastest"""
    out = []
    for dims in (map1, map2):
        lin = 0
        for d in reversed(dims):
            lin = lin * nblks[d] + index[d]
        out.append(lin)
    return tuple(out)


def index_of_row_col(R, Cc, nblks, map1, map2):
    index = [None] * len(nblks)
    for lin, dims in ((R, map1), (Cc, map2)):
        for d in dims:
            index[d] = lin % nblks[d]
            lin //= nblks[d]
    return tuple(index)


def folded_sizes(blk_sizes, dims):
    """the block sizes of the folded rows (or columns): entry R is the product of the sizes of the block indices that R stands for"""
    nblks = [len(blk_sizes[d]) for d in dims]
    out = np.zeros(int(np.prod(nblks)), np.int64)
    for combo in itertools.product(*[range(n) for n in reversed(nblks)]):
        combo = combo[::-1]   # combo[k]: the index along dims[k]
        lin, size = 0, 1
        for k in reversed(range(len(dims))):
            lin = lin * nblks[k] + combo[k]
            size *= int(blk_sizes[dims[k]][combo[k]])
        out[lin] = size
    return out


def stored_block(blk, map1, map2):
    """flat, as the matrix stores it: the Fortran array of the block with its dimensions in the order map1 ++ map2"""
    return np.transpose(blk, tuple(map1) + tuple(map2)).reshape(-1, order="F")


def canonical_block(flat, index, blk_sizes, map1, map2):
    order = tuple(map1) + tuple(map2)
    ext = extents(index, blk_sizes)
    return np.transpose(flat.reshape([ext[d] for d in order], order="F"), np.argsort(order))


def flat_canonical(blk):
    """a block as it crosses the interface: dimension 0 fastest"""
    return blk.reshape(-1, order="F")


def matrix_of(blocks, blk_sizes, map1, map2, dtype):
    """(row_sizes, col_sizes, row_p, col_i, blk_p, data, order): the packed matrix of the mapping; order: the block indices in the matrix' index order"""
    nblks = [len(s) for s in blk_sizes]
    rs, cs = folded_sizes(blk_sizes, map1), folded_sizes(blk_sizes, map2)
    order = sorted(blocks, key=lambda ix: block_row_col(ix, nblks, map1, map2))
    rc = [block_row_col(ix, nblks, map1, map2) for ix in order]
    row_p = np.zeros(len(rs) + 1, np.int32)
    for R, _ in rc:
        row_p[R + 1] += 1
    row_p = np.cumsum(row_p).astype(np.int32)
    col_i = np.array([c for _, c in rc], np.int32)
    flats = [stored_block(blocks[ix], map1, map2) for ix in order]
    sizes = np.array([f.size for f in flats], np.int64)
    blk_p = (np.cumsum(sizes) - sizes).astype(np.int64) if len(flats) else np.zeros(0, np.int64)
    data = np.concatenate(flats).astype(dtype) if flats else np.zeros(0, dtype)
    return rs, cs, row_p, col_i, blk_p, data, order


def blocks_of_matrix(row_p, col_i, blk_p, data, blk_sizes, map1, map2):
    nblks = [len(s) for s in blk_sizes]
    out = {}
    for R in range(len(row_p) - 1):
        for b in range(int(row_p[R]), int(row_p[R + 1])):
            ix = index_of_row_col(R, int(col_i[b]), nblks, map1, map2)
            n = int(np.prod(extents(ix, blk_sizes)))
            out[ix] = canonical_block(data[int(blk_p[b]):int(blk_p[b]) + n], ix, blk_sizes, map1, map2)
    return out


def permuted(blocks, order):
    """numpy.transpose on a dict of blocks: dimension j of the result is dimension order[j]"""
    return {tuple(ix[d] for d in order): np.transpose(blk, order) for ix, blk in blocks.items()}


# ---- contraction ----------------------------------------------------------------------------------------------------------------------------------------------
def _subscripts(rank_1, rank_2, rank_3, c1, n1, c2, n2, m1, m2):
    letters = iter("abcdefghijkl")
    s1, s2, s3 = [None] * rank_1, [None] * rank_2, [None] * rank_3
    for a, b in zip(c1, c2):
        s1[a] = s2[b] = next(letters)
    for a, b in zip(n1, m1):
        s1[a] = s3[b] = next(letters)
    for a, b in zip(n2, m2):
        s2[a] = s3[b] = next(letters)
    return "%s,%s->%s" % ("".join(s1), "".join(s2), "".join(s3))


def contract_pattern(P1, P2, c1, n1, c2, n2, m1, m2):
    """boolean nd array over tensor_3's blocks: where a block of tensor_1 meets a block of tensor_2 (the boolean product of the two patterns)"""
    rank_3 = len(m1) + len(m2)
    return np.einsum(_subscripts(P1.ndim, P2.ndim, rank_3, c1, n1, c2, n2, m1, m2), P1.astype(np.int64), P2.astype(np.int64)) > 0


def pattern_of(blocks, blk_sizes):
    P = np.zeros([len(s) for s in blk_sizes], bool)
    for ix in blocks:
        P[ix] = True
    return P


def contract_dense(alpha, D1, D2, beta, D3, c1, n1, c2, n2, m1, m2):
    """(R, bound): beta D3 + alpha sum D1 D2 and |beta| |D3| + |alpha| sum |D1| |D2|, dense, in longdouble / clongdouble"""
    w = wide(D3.dtype)
    sub = _subscripts(D1.ndim, D2.ndim, D3.ndim, c1, n1, c2, n2, m1, m2)
    R = beta * D3.astype(w) + alpha * np.einsum(sub, D1.astype(w), D2.astype(w))
    bound = abs(beta) * np.abs(D3).astype(LD) + abs(alpha) * np.einsum(sub, np.abs(D1).astype(LD), np.abs(D2).astype(LD))
    return R, bound


class Contracted:
    """what contract() returns: blocks (dict, wide type), bound (dict, longdouble), flop, nproducts, unfiltered (the index set without any filter),
    product_margins / block_margins (norm / threshold ratios, for the conditions on the filtered cases), n_inner (contracted elements)"""


def contract(alpha, B1, sizes1, B2, sizes2, beta, B3, sizes3, c1, n1, c2, n2, m1, m2, dtype, filter_eps=None, retain_sparsity=False):
    """The contraction block by block, as dbcsr_multiply runs it on any folding (the rules do not depend on the order inside the tuples): tensor_3 counts
    as empty unless beta != 0 or retain_sparsity; with retain_sparsity only blocks tensor_3 stores are computed; with filter_eps a block product is
    skipped on the fly iff fl32(fl32(||a||^2) fl32(|alpha|^2 ||b||^2)) < fl32(e e), e = fl32(eps) / fl32(stored blocks of tensor_1 with a's free indices),
    and -- unless retain_sparsity -- a result block with ||blk||^2 < eps^2 leaves the result (tests/option_sweep.py: restate)."""
    w = wide(dtype)
    eps = float(filter_eps or 0.0)
    keep_data = bool(retain_sparsity) or beta != 0
    rank_3 = len(m1) + len(m2)
    back = np.argsort(tuple(m1) + tuple(m2))
    norm2 = lambda blk: LD((np.abs(blk.astype(w)).astype(LD) ** 2).sum())
    row_count = {}
    for ix in B1:
        f1 = tuple(ix[d] for d in n1)
        row_count[f1] = row_count.get(f1, 0) + 1
    by_k = {}
    for ix, blk in B2.items():
        by_k.setdefault(tuple(ix[d] for d in c2), []).append((ix, blk))
    out = Contracted()
    R, bound = {}, {}
    if keep_data:
        for ix, blk in B3.items():
            R[ix] = beta * blk.astype(w)
            bound[ix] = abs(beta) * np.abs(blk).astype(LD)
    old = set(R)
    flop = nprod = 0
    out.unfiltered = set(old)
    out.product_margins = []
    nc = len(c1)
    for ix1, b1 in B1.items():
        k = tuple(ix1[d] for d in c1)
        f1 = tuple(ix1[d] for d in n1)
        a = np.transpose(b1, tuple(n1) + tuple(c1)).astype(w)
        for ix2, b2 in by_k.get(k, []):
            ix3 = [None] * rank_3
            for d, i in zip(m1, f1):
                ix3[d] = i
            for d, i in zip(m2, (ix2[d] for d in n2)):
                ix3[d] = i
            ix3 = tuple(ix3)
            if retain_sparsity and ix3 not in old:
                continue
            out.unfiltered.add(ix3)
            if eps > 0:
                e = np.float32(eps) / np.float32(max(row_count[f1], 1))
                row_eps = np.float32(e * e)
                na, nb = np.float32(norm2(b1)), np.float32((abs(alpha) ** 2) * norm2(b2))
                prod = np.float32(na * nb)
                out.product_margins.append(float(prod) / float(row_eps) if row_eps > 0 else np.inf)
                if prod < row_eps:
                    continue
            b = np.transpose(b2, tuple(c2) + tuple(n2)).astype(w)
            axes = (list(range(a.ndim - nc, a.ndim)), list(range(nc)))
            p = np.transpose(np.tensordot(a, b, axes=axes), back)
            pb = np.transpose(np.tensordot(np.abs(a).astype(LD), np.abs(b).astype(LD), axes=axes), back)
            if ix3 not in R:
                R[ix3] = np.zeros(p.shape, w)
                bound[ix3] = np.zeros(p.shape, LD)
            R[ix3] = R[ix3] + alpha * p
            bound[ix3] = bound[ix3] + abs(alpha) * pb
            nprod += 1
            flop += 2 * int(np.prod(a.shape)) * int(np.prod(b.shape[nc:]))
    out.block_margins = []
    if eps > 0 and not retain_sparsity:
        for ix in list(R):
            n2 = norm2(R[ix])
            out.block_margins.append(float(np.sqrt(n2)) / eps)
            if n2 < LD(eps) * LD(eps):
                del R[ix], bound[ix]
    out.blocks, out.bound, out.flop, out.nproducts = R, bound, int(flop), int(nprod)
    out.n_inner = max([int(np.prod([sizes1[d][ix[d]] for d in c1])) for ix in B1] + [1])
    out.n_inner_total = int(np.prod([int(np.sum(sizes1[d])) for d in c1]))
    return out
