"""The option sweep on the device: every case of tests/option_sweep.py (complex128 with 'C' transposes and filter_eps, limits, operands and products with
symmetry, fp32 blocks above 32 and blocks above 80) through the dbcsr_multiply mirror AND through the C entry (dbcsr_amd_multiply, _z, _symmetric_c,
_symmetric_c_klimits, _symmetric_c_z), each held to the same dense long-double reference: index and flop exact, every element inside the window within
gamma (|alpha| (|op A| |op B|) + |beta| |C_in|) -- gamma derived in tests/option_sweep.py, not measured --, every kept bit outside the window unchanged.
The two entries are not compared with each other (they may choose different k passes).  The kernel family of last_kernel() is the one the host build
of mm_choose.h predicts for the real cases without product symmetry, and z64 for every complex case.  tests/test_option_sweep_cpu.py shows on the host
that the inputs meet their conditions and that the reference notices a dropped conjugation, a crop bound off by one and a norm from the real part alone.

The worst err / bar per stratum and entry is printed by the last test (and written to the file DBCSR_AMD_OPTSWEEP_REPORT names): a record, not a
threshold."""
import os

import pytest
import torch

from dbcsr_amd.multiply import MultiplyEngine, dbcsr_multiply
from tests import option_sweep as S
from tests.gpu_util import dev_to_bcsr, native_multiply_any, to_dev
from tests.test_numeric_choice import choose, shims  # noqa: F401  (the host build of mm_choose.h, a module-scoped fixture)

pytestmark = pytest.mark.gpu

if not S.LONG_DOUBLE_OK:
    pytest.skip("np.longdouble has no 63-bit mantissa here: the reference of the option sweep needs one", allow_module_level=True)

LIMIT_NAMES = ("first_row", "last_row", "first_column", "last_column", "first_k", "last_k")
SWITCHES = ("DBCSR_AMD_MM_CLASSES", "DBCSR_AMD_MM_SYMBOLIC", "DBCSR_AMD_MM_WG_WAVES", "DBCSR_AMD_MM_HOT", "DBCSR_AMD_MM_KCHUNKS")
WORST = {}   # (stratum, entry) -> (worst err / bar, case number)


def params(name):
    out = []
    for i in range(S.count(name)):
        out.append(pytest.param(i, "mirror", id="%d-mirror" % i))
        if S.runs_both_entries(S.case(name, i)):
            out.append(pytest.param(i, "native", id="%d-native" % i))
    return out


def through_the_mirror(c, A, B, Cm, eng):
    dA, dB, dC = to_dev(A), to_dev(B), to_dev(Cm)
    dA.symmetry, dB.symmetry, dC.symmetry = c["symm_a"], c["symm_b"], c["symm_c"]
    flop = [0]
    limits = dict(zip(LIMIT_NAMES, c["limits"])) if c["limits"] is not None else {}
    dbcsr_multiply(c["ta"], c["tb"], c["alpha"], dA, dB, c["beta"], dC, retain_sparsity=c["retain"], filter_eps=c["eps"] or None, flop=flop, engine=eng,
                   **limits)
    torch.cuda.synchronize()
    return dev_to_bcsr(dC), flop[0]


def through_the_c_entry(c, A, B, Cm, eng):
    return native_multiply_any(eng, c["ta"], c["tb"], c["alpha"], A, B, c["beta"], Cm, limits=c["limits"], retain=c["retain"], eps=c["eps"],
                               symm_c=c["symm_c"], klimits=(0, 0) if c["klimits"] else None)


def run(name, i, entry, monkeypatch, shims):  # noqa: F811
    c = S.case(name, i)
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    eng = MultiplyEngine()   # a fresh engine: it reads the switches when it is made
    got, flop = (through_the_mirror if entry == "mirror" else through_the_c_entry)(c, *S.operands(name, i), eng)
    bad, worst = S.compare(name, i, got, flop)
    print("%s %d %s: err / bar %.3f" % (name, i, entry, worst))
    assert bad is None, (bad, c)
    WORST[(name, entry)] = max(WORST.get((name, entry), (0.0, -1)), (worst, i))
    # the kernel family (a multiply without a kept block product launches no block-product kernel: nothing to name)
    if S.reference(name, i).nproducts > 0:
        q = S.choice_case(name, i)
        if c["dtype"] == S.Z64:
            assert S.family(eng.last_kernel()) == "z64", eng.last_kernel()
        elif q is not None:
            assert S.family(eng.last_kernel()) == S.family(choose(shims, c["env"], q[0], **q[1])[0]), (eng.last_kernel(), c)


@pytest.mark.parametrize("i,entry", params("complex"))
def test_complex(i, entry, monkeypatch, shims):  # noqa: F811
    run("complex", i, entry, monkeypatch, shims)


@pytest.mark.parametrize("i,entry", params("limits"))
def test_limits(i, entry, monkeypatch, shims):  # noqa: F811
    run("limits", i, entry, monkeypatch, shims)


@pytest.mark.parametrize("i,entry", params("symmetry"))
def test_symmetry(i, entry, monkeypatch, shims):  # noqa: F811
    run("symmetry", i, entry, monkeypatch, shims)


@pytest.mark.parametrize("i,entry", params("sizes"))
def test_sizes(i, entry, monkeypatch, shims):  # noqa: F811
    run("sizes", i, entry, monkeypatch, shims)


@pytest.mark.parametrize("limits", [dict(first_row=1, last_row=1), dict(first_column=2), dict(first_k=1, last_k=1)], ids=lambda d: "-".join(d))
def test_limits_with_a_product_with_symmetry_are_refused_before_anything_is_written(limits):
    name, i = "symmetry", 3
    c = S.case(name, i)
    assert c["symm_c"] != "N" and c["M"] >= 2
    A, B, Cm = S.operands(name, i)
    dC = to_dev(Cm)
    dC.symmetry = c["symm_c"]
    tensors = (dC.row_p, dC.col_i, dC.blk_p, dC.data)
    bits = [t.cpu().numpy().tobytes() for t in tensors]
    with pytest.raises(NotImplementedError):
        dbcsr_multiply(c["ta"], c["tb"], c["alpha"], to_dev(A), to_dev(B), c["beta"], dC, engine=MultiplyEngine(), **limits)
    torch.cuda.synchronize()
    assert all(now is was for now, was in zip((dC.row_p, dC.col_i, dC.blk_p, dC.data), tensors))   # the same objects ...
    assert [t.cpu().numpy().tobytes() for t in tensors] == bits                                     # ... with the same bits


def test_report_the_worst_ratios():
    """for the record (profiles/option_sweep.txt): the worst err / bar per stratum and entry of this run"""
    lines = ["%-9s %-7s worst err / bar %.3f (case %d)" % (name, entry, w, i) for (name, entry), (w, i) in sorted(WORST.items())]
    print("\n".join(lines))
    path = os.environ.get("DBCSR_AMD_OPTSWEEP_REPORT")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
