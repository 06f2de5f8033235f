"""GPU: the arithmetic headers as gfx950 device code -- csrc/hdr_math.hpp, df32_math.hpp, qd_math.hpp, bla_math.hpp and the double-word
helpers of csrc/dw_math.hpp with the fused multiply-add toward -infinity -- bit for bit against the exact model of
tests/_ieee_model.py on the committed edge cases of tests/_arith_cases.py (the cases of tests/test_arith_edges_cpu.py, plus the
device-only families).  tests/arith/arith_device.hip is compiled once with the product's render flags and run once: one launch per
op family, one case per lane.

The packed forms hang on the same pin: df32x2 and hr_add2 equal scalar df32 (tests/test_gpu_df32x2.py), scalar df32 equals the
model here, and hr_add2 is sent through the boundary gaps explicitly (family hr_add2).

Times on an MI355X machine: the fixture 2.5 s (compiling arith_device.hip 1.0 s, compiling and running the host program, modelling
the 36 000 cases, the GPU process 0.3 s); each test below 0.01 s, a comparison of a few thousand rows of eight words."""
import os
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _arith_cases as C      # noqa: E402
from _arith_run import build_device, build_host, run_host, words_equal, describe  # noqa: E402

# a handful of sub-millisecond launches after the runtime's start-up
RUN_LIMIT_S = 60


@pytest.fixture(scope="module")
def device(tmp_path_factory):
    """(cases, family -> rows, device words per row, host words per row).  One compile, one GPU process; a failure here is cached
    for the module, so after a fault, an abort or a time limit no test starts another GPU process."""
    d = tmp_path_factory.mktemp("arith_device")
    t0 = time.time()
    exe = build_device(d)
    t1 = time.time()
    cases, where = C.all_cases()
    host_out = run_host(build_host(d), d, cases)
    cf, of = os.path.join(str(d), "cases.bin"), os.path.join(str(d), "device_out.bin")
    C.write_case_file(cf, cases)
    t2 = time.time()
    # the environment is inherited unchanged
    p = subprocess.run(["timeout", "-k", "10", str(RUN_LIMIT_S), exe, cf, of], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    t3 = time.time()
    print("arith_device: compile %.1f s, run %.1f s, %d cases" % (t1 - t0, t3 - t2, len(cases)))
    assert p.returncode == 0, "arith_device exit status %d\n%s" % (p.returncode, p.stdout)
    return cases, where, C.read_out_file(of, len(cases)), host_out


def _add2_equal(case, got):
    """hr_add2: bit for bit hr_add / hr_sub of both parts wherever `rare` is not reported; `rare` only for a zero result (the
    committed cases have no non-finite ones) -- what the straight line returns next to it is its caller's to discard"""
    rare = got[6]
    if rare not in (0, 1):
        return False
    if rare:
        return case.out_words[6] == 1
    return list(got[:7]) == list(case.out_words[:7])


@pytest.mark.parametrize("family", list(C.FAMILIES))
def test_device_equals_model(device, family):
    cases, where, out, host_out = device
    same = _add2_equal if family == "hr_add2" else (lambda c, got: words_equal(c, got, c.out_words))
    rows = where[family]
    assert len(rows) >= 500
    bad = [describe(cases[i], out[i], host_out[i] if cases[i].op.host else None) for i in rows if not same(cases[i], out[i])]
    assert not bad, "%d of %d cases differ, first:\n%s" % (len(bad), len(rows), "\n".join(bad[:10]))


def test_hr_add2_covers_what_it_claims(device):
    """`rare` is the exception: the boundary-gap cases with a non-zero result are all covered by the straight line"""
    cases, where, out, _ = device
    rows = where["hr_add2"]
    rare = sum(1 for i in rows if out[i][6])
    zero = sum(1 for i in rows if cases[i].out_words[6])
    assert rare == zero and rare * 2 < len(rows), (rare, zero, len(rows))
