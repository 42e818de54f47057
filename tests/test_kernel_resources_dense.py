"""The kernels of the dense conversion (dbcsr_amd/csrc/mm_dense.h: dense_gather, dense_scatter, dense_block_norms, dense_emit), read from the code object of
the shipping build (no GPU needed).  DESIGN 3.13 claims: the three typed kernels are there once per data type, the index kernel once; none uses scratch;
none needs more registers than what the build shows rounded up to the allocation granule of 8 -- 72 / 88 / 56 for dense_gather (float64, float32,
complex128), 56 / 96 / 40 for dense_scatter, 24 for dense_block_norms -- all at most 128, so registers allow at least four waves per SIMD (float32, whose
packs hold four elements, needs the most); the transposing kernels hold one tile of 32 x 33 elements in LDS: 8448 / 4224 / 16896 bytes, at most 32 KB."""
import pytest

from tests.test_kernel_resources import demangle, kernels_of_library

ALL = ("double", "float", "dbcsr_amd::z64")
TYPED = ("dense_gather", "dense_scatter", "dense_block_norms")
VGPRS = {("dense_gather", "double"): 72, ("dense_gather", "float"): 88, ("dense_gather", "dbcsr_amd::z64"): 56,
         ("dense_scatter", "double"): 56, ("dense_scatter", "float"): 96, ("dense_scatter", "dbcsr_amd::z64"): 40,
         ("dense_block_norms", "double"): 24, ("dense_block_norms", "float"): 24, ("dense_block_norms", "dbcsr_amd::z64"): 24}
TILE_BYTES = {"double": 32 * 33 * 8, "float": 32 * 33 * 4, "dbcsr_amd::z64": 32 * 33 * 16}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    ks = kernels_of_library(tmp_path_factory.mktemp("dense_kernels"))
    pretty = demangle(sorted(ks))
    return {pretty[n]: k for n, k in ks.items()}


def the_one(kernels, name, t):
    mine = [k for n, k in kernels.items() if n.startswith("void dbcsr_amd::%s<%s>(" % (name, t))]
    assert len(mine) == 1, sorted(n for n in kernels if "dense_" in n)
    return mine[0]


@pytest.mark.parametrize("t", ALL)
@pytest.mark.parametrize("name", TYPED)
def test_dense_kernel_fits_its_registers_without_scratch(kernels, name, t):
    k = the_one(kernels, name, t)
    print(name, t, {f: k[f] for f in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
    assert k["private_segment_fixed_size"] == 0
    assert k["vgpr_count"] <= VGPRS[(name, t)] <= 128, k
    if name == "dense_block_norms":
        assert k["group_segment_fixed_size"] == 0, k
    else:
        assert k["group_segment_fixed_size"] == TILE_BYTES[t] <= 32 * 1024, k


def test_nothing_else_of_the_dense_conversion_ships(kernels):
    assert len([n for n in kernels if "dbcsr_amd::dense_" in n]) == len(TYPED) * len(ALL) + 1
    emit = [k for n, k in kernels.items() if n.startswith("dbcsr_amd::dense_emit(")]
    assert len(emit) == 1 and emit[0]["private_segment_fixed_size"] == 0 and emit[0]["vgpr_count"] <= 16 and emit[0]["group_segment_fixed_size"] == 0


def test_the_other_kernels_keep_their_counts(kernels):
    """no new kernel carries a name that the earlier resource tests count by, or begins with the name of an earlier kernel"""
    dense_names = [n for n in kernels if "dbcsr_amd::dense_" in n]
    for word in ("algebra", "diag_", "block_inverse", "block_diag"):
        assert not [n for n in dense_names if word in n], word
    assert len([n for n in kernels if "block_inverse_" in n]) == 2 * len(ALL)
    assert len([n for n in kernels if "block_diag_" in n]) == len(ALL) + 1
    assert len([n for n in kernels if "algebra_matvec" in n]) == 3 * len(ALL)
    assert len([n for n in kernels if "algebra_multivec" in n]) == 3 * len(ALL)
    assert len([n for n in kernels if "algebra_rank_update" in n]) == 2 * len(ALL)
    assert len([n for n in kernels if "algebra_col_sums<" in n]) == len(ALL)
    for name in ("diag_get<", "diag_set<", "diag_fill<", "diag_shift<"):
        assert len([n for n in kernels if n.startswith("void dbcsr_amd::" + name)]) == len(ALL), name
