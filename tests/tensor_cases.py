"""The inputs of the tensor tests, pure numpy: shared by tests/test_tensor_cpu.py (which checks the conditions they must meet) and tests/test_gpu_tensor.py
(which runs them).  Everything is seeded; nothing here imports torch or the library."""
import itertools

import numpy as np

from tests import tensor_ref as TR

F64, F32, Z64 = "float64", "float32", "complex128"
DTYPES = (F64, F32, Z64)

# the mappings of the put / get and copy tests
MAPPINGS = {
    2: [((0,), (1,)), ((1,), (0,))],
    3: [((0,), (1, 2)), ((0, 1), (2,)), ((1,), (2, 0)), ((2, 0), (1,)), ((2, 1), (0,))],
    4: [((0, 1), (2, 3)), ((3, 1), (0, 2)), ((2,), (3, 0, 1))],
}
ORDERS = {2: (1, 0), 3: (2, 0, 1), 4: (3, 1, 0, 2)}   # the non-trivial `order` of the copy tests
COPY_PAIRS = {
    2: [(a, b) for a in range(2) for b in range(2)],
    3: [(a, b) for a in range(5) for b in range(5)],
    4: [(0, 1), (1, 2), (2, 0), (1, 1)],
}
SIZE_POOL = (1, 2, 3, 5, 23, 32, 33)
MAX_ELEMENTS = 6_000_000   # of one test tensor (a condition on the seeds: tests stay quick)

# ---- the kernel through the C entry -------------------------------------------------------------------------------------------------------------------------
EXTENT_POOL = (1, 2, 3, 23, 32, 33, 65)
EXTENT_CLASSES = EXTENT_POOL
KERNEL_MAX_BLOCK = 300_000   # elements of one block of a kernel launch


def kernel_extents(rank, perm, seed):
    """the blocks of one launch: 23^rank-or-3 always, a block with a 1 in each position, every extent class as source-fastest and as written-fastest
    dimension, and random draws"""
    rng = np.random.default_rng(seed)
    out = [tuple([23] * min(rank, 3) + [1] * (rank - min(rank, 3)))]
    for pos in range(rank):
        e = [33, 5, 23, 2][:rank]
        e[pos] = 1
        out.append(tuple(e))
    for c in EXTENT_CLASSES:   # c as the source-fastest (dimension 0) and as the written-fastest (dimension perm[0]) extent
        for fast in (0, perm[0]):
            e = [int(rng.choice((2, 3, 5)))] * rank
            e[fast] = c
            other = (fast + 1) % rank
            e[other] = int(rng.choice((3, 23, 33)))
            out.append(tuple(e))
    while len(out) < 3 * len(EXTENT_CLASSES) + rank + 1:
        e = tuple(int(x) for x in rng.choice(EXTENT_POOL, rank))
        if int(np.prod(e)) <= KERNEL_MAX_BLOCK:
            out.append(e)
    return out


def kernel_layout(exts, itemsize, seed):
    """(src_off, dst_off, src_len, dst_len): odd source offsets; written windows that start at every 16-byte phase; room for canaries between and around"""
    V = max(16 // itemsize, 1)
    src_off, dst_off = [], []
    sp, dp = 9, 8
    for b, e in enumerate(exts):
        n = int(np.prod(e))
        sp |= 1
        src_off.append(sp)
        sp += n + 3
        while dp % V != b % V:
            dp += 1
        dst_off.append(dp)
        dp += n + 5
    return np.array(src_off, np.int64), np.array(dst_off, np.int64), sp + 16, dp + 16


def permutations(rank):
    return list(itertools.permutations(range(rank)))


# ---- random tensors ---------------------------------------------------------------------------------------------------------------------------------------------
def values(rng, shape, dtype):
    """magnitudes in [0.5, 1.5) with random signs (complex: both parts): no value is tiny, so block norms are away from any threshold"""
    def part():
        return (rng.random(shape) + 0.5) * rng.choice((-1.0, 1.0), shape)
    x = part() + 1j * part() if np.dtype(dtype).kind == "c" else part()
    return np.asarray(x).astype(dtype)


def random_tensor(seed, rank, dtype, pool=SIZE_POOL, nb_range=(3, 5), fill=0.5, nblks=None):
    """(blk_sizes, blocks): per dimension nb_range blocks of sizes from the pool, each block stored with probability fill"""
    rng = np.random.default_rng(seed)
    nb = nblks or [int(rng.integers(nb_range[0], nb_range[1] + 1)) for _ in range(rank)]
    sizes = [rng.choice(pool, n).astype(np.int64) for n in nb]
    blocks = {}
    for ix in itertools.product(*[range(n) for n in nb]):
        if rng.random() < fill:
            blocks[ix] = values(rng, TR.extents(ix, sizes), dtype)
    return sizes, blocks


def elements(blocks):
    return sum(b.size for b in blocks.values())


PUTGET_SEED = {2: 101, 3: 102, 4: 103}


def putget_tensor(rank, dtype):
    return random_tensor(PUTGET_SEED[rank], rank, dtype)


# ---- contractions -------------------------------------------------------------------------------------------------------------------------------------------------
CONTRACT_POOL = (1, 2, 3, 5, 7, 23)


class Contraction:
    def __init__(self, name, ranks, c1, n1, c2, n2, m1, m2, compatible, reversed_, foreign, t3_compatible, t3_foreign, seed, fills=(0.5, 0.6, 0.3),
                 nfree=(3, 4)):
        self.name, self.ranks = name, ranks
        self.c1, self.n1, self.c2, self.n2, self.m1, self.m2 = c1, n1, c2, n2, m1, m2
        # (mapping of tensor_1, mapping of tensor_2) per operand variant; mappings of tensor_3
        self.operands = {"compatible": compatible, "reversed": reversed_, "foreign": foreign}
        self.t3_compatible, self.t3_foreign = t3_compatible, t3_foreign
        self.seed, self.fills, self.nfree = seed, fills, nfree   # nfree: the range of the block counts of the free dimensions

    def sizes(self):
        """block sizes of the three tensors, the paired dimensions sharing theirs"""
        rng = np.random.default_rng(self.seed)
        r1, r2, r3 = self.ranks
        count = lambda d, free: int(rng.integers(self.nfree[0], self.nfree[1] + 1)) if free else int(rng.integers(3, 5))
        s1 = [rng.choice(CONTRACT_POOL, count(d, d in self.n1)).astype(np.int64) for d in range(r1)]
        s2, s3 = [None] * r2, [None] * r3
        for a, b in zip(self.c1, self.c2):
            s2[b] = s1[a]
        for b in self.n2:
            s2[b] = rng.choice(CONTRACT_POOL, count(b, True)).astype(np.int64)
        for a, b in zip(self.n1, self.m1):
            s3[b] = s1[a]
        for a, b in zip(self.n2, self.m2):
            s3[b] = s2[a]
        return s1, s2, s3

    def tensors(self, dtype, small_free_2=False):
        """(sizes, blocks) x 3.  small_free_2: the blocks of tensor_2 whose first free index is 0 are scaled by 1e-10 (the filtered cases: their products
        fall far below any threshold, everything else far above)"""
        s1, s2, s3 = self.sizes()
        rng = np.random.default_rng(self.seed + 1)

        def fill(sizes, p):
            out = {}
            for ix in itertools.product(*[range(len(s)) for s in sizes]):
                if rng.random() < p:
                    out[ix] = values(rng, TR.extents(ix, sizes), dtype)
            return out

        B1, B2, B3 = fill(s1, self.fills[0]), fill(s2, self.fills[1]), fill(s3, self.fills[2])
        if small_free_2:
            for ix in B2:
                if ix[self.n2[0]] == 0:
                    B2[ix] = (B2[ix] * 1e-10).astype(dtype)
        return (s1, B1), (s2, B2), (s3, B3)


CONTRACTIONS = {
    # (a) T3[i,j,l] = T1[i,j,k] T2[k,l]
    "a": Contraction("a", (3, 2, 3), (2,), (0, 1), (0,), (1,), (0, 1), (2,),
                     compatible=(((0, 1), (2,)), ((0,), (1,))), reversed_=(((2,), (0, 1)), ((1,), (0,))), foreign=(((0,), (1, 2)), ((0,), (1,))),
                     t3_compatible=((0, 1), (2,)), t3_foreign=((2, 0), (1,)), seed=201),
    # (b) T3[i,j] = T1[k,i,l] T2[l,j,k], over two dimensions
    "b": Contraction("b", (3, 3, 2), (0, 2), (1,), (2, 0), (1,), (0,), (1,),
                     compatible=(((1,), (2, 0)), ((0, 2), (1,))), reversed_=(((0, 2), (1,)), ((1,), (2, 0))), foreign=(((0,), (1, 2)), ((0,), (1, 2))),
                     t3_compatible=((0,), (1,)), t3_foreign=((1,), (0,)), seed=202, fills=(0.3, 0.3, 0.4), nfree=(5, 6)),
    # (c) T3[m,j,i,l] = T1[i,k,j] T2[l,m,k], over one
    "c": Contraction("c", (3, 3, 4), (1,), (0, 2), (2,), (0, 1), (2, 1), (3, 0),
                     compatible=(((2, 0), (1,)), ((2,), (0, 1))), reversed_=(((1,), (2, 0)), ((0, 1), (2,))), foreign=(((0, 1), (2,)), ((0,), (1, 2))),
                     t3_compatible=((1, 2), (3, 0)), t3_foreign=((0, 1), (2, 3)), seed=203),
    # (d) T3[i,m,j,l] = T1[i,j,k,l] T2[k,m]
    "d": Contraction("d", (4, 2, 4), (2,), (0, 1, 3), (0,), (1,), (0, 2, 3), (1,),
                     compatible=(((3, 0, 1), (2,)), ((0,), (1,))), reversed_=(((2,), (3, 0, 1)), ((1,), (0,))), foreign=(((0, 1), (2, 3)), ((1,), (0,))),
                     t3_compatible=((3, 0, 2), (1,)), t3_foreign=((0, 1), (2, 3)), seed=204),
    # (e) rank 2: a matrix multiply
    "e": Contraction("e", (2, 2, 2), (1,), (0,), (0,), (1,), (0,), (1,),
                     compatible=(((0,), (1,)), ((0,), (1,))), reversed_=(((1,), (0,)), ((1,), (0,))), foreign=None,
                     t3_compatible=((0,), (1,)), t3_foreign=((1,), (0,)), seed=205),
}
# permute launches the operands of a variant cost (tensor_1, tensor_2 of "foreign": only what is neither compatible nor reversed is remapped)
OPERAND_LAUNCHES = {("a", "foreign"): 1, ("b", "foreign"): 2, ("c", "foreign"): 2, ("d", "foreign"): 1}
TYPED_CASES = ("a", "b")     # float32 and complex128 run on these
FILTER_CASES = ("a", "b")
FILTER_EPS = 1e-4
SCALARS = {F64: (0.75, -1.5), F32: (0.75, -1.5), Z64: (0.75 - 0.5j, 1.5 + 0.25j)}


def contract_args(c):
    return dict(contract_1=c.c1, notcontract_1=c.n1, contract_2=c.c2, notcontract_2=c.n2, map_1=c.m1, map_2=c.m2)


def reference(c, dtype, alpha, beta, filter_eps=None, retain_sparsity=False):
    (s1, B1), (s2, B2), (s3, B3) = c.tensors(dtype, small_free_2=filter_eps is not None)
    return TR.contract(alpha, B1, s1, B2, s2, beta, B3, s3, c.c1, c.n1, c.c2, c.n2, c.m1, c.m2, dtype, filter_eps=filter_eps,
                       retain_sparsity=retain_sparsity)
