"""CPU: the arithmetic headers (csrc/hdr_math.hpp, df32_math.hpp, qd_math.hpp, bla_math.hpp) under g++ with the host input builders'
flags, bit for bit against the exact model of tests/_ieee_model.py on the committed edge cases of tests/_arith_cases.py; which
model arms those cases reach; and value checks of the results against exact rational arithmetic (tests/_arith_values.py).

Model time on the build machine, per family (the whole case set of a family, modelled once per session and shared):
hdr_f32 0.07 s, hdr_f64 0.07 s, hdr_df32 0.2 s, df32 0.12 s, qd_f32 0.35 s, qd_f64 0.3 s, bla 0.04 s, dw 0.16 s, fma_down 0.03 s,
hr_add2 0.03 s; the value checks (Fractions) take longer than the model, a few seconds for the largest family."""
import math
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _arith_cases as C      # noqa: E402
import _arith_values as V     # noqa: E402
import _ieee_model as M       # noqa: E402
from _arith_run import build_host, run_host, words_equal, describe  # noqa: E402

# the families with entries the host program evaluates (dw, fma_down and hr_add2 are device code only)
HOST_FAMILIES = [n for n in C.FAMILIES if n not in ("dw", "fma_down", "hr_add2")]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """(all cases, family -> row indices, host result words per row): one build, one run"""
    d = tmp_path_factory.mktemp("arith_host")
    exe = build_host(d)
    cases, where = C.all_cases()
    return exe, cases, where, run_host(exe, d, cases)


def test_op_table_matches_the_header(host):
    """the ids, names and word counts of arith_ops.hpp are those of the Python table (the device-only entries are not listed by the
    host program; a wrong id there fails the GPU test)"""
    listed = subprocess.run([host[0], "--list"], stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")
    rows = sorted(tuple(r.split()) for r in listed if r.strip())
    mine = sorted((str(o.id), o.name, str(o.words_in), str(o.words_out)) for o in C.OPS.values() if o.host)
    assert rows == mine


def test_build_recipe_sees_the_double_word_header():
    """csrc/dw_math.hpp is one of the headers whose content the render library's stamps hash, and the low-precision kernels get
    their double-word helpers from it"""
    from fractalshark_amd import _build
    assert os.path.join(_build.CSRC, "dw_math.hpp") in _build._render_headers()
    unit = open(os.path.join(_build.CSRC, "kernels_direct_lp.hip")).read()
    assert '#include "dw_math.hpp"' in unit and "dw_add(dw<T> a" not in unit


@pytest.mark.parametrize("family", HOST_FAMILIES)
def test_host_equals_model(host, family):
    _, cases, where, out = host
    bad = [describe(cases[i], out[i]) for i in where[family] if cases[i].op.host and not words_equal(cases[i], out[i], cases[i].out_words)]
    assert not bad, "%d of %d cases differ, first:\n%s" % (len(bad), len(where[family]), "\n".join(bad[:10]))


@pytest.mark.parametrize("family", list(C.FAMILIES))
def test_redraws_stay_below_one_percent(family):
    C.build(family)
    f = C.FAMILIES[family]
    assert f.draws >= 500 and f.redraws * 100 <= f.draws, (f.draws, f.redraws)
    print("%s: %d cases, %d of %d draws redrawn" % (family, len(f.cases), f.redraws, f.draws))


def test_case_counts():
    """the committed set: per family and per class (a generator that silently yields nothing would show here)"""
    for name in C.FAMILIES:
        cases = C.build(name)
        classes = {c for c, _ in C.FAMILIES[name].gens}
        seen = {c.cls for c in cases}
        assert seen == classes, (name, classes - seen)
        assert len(cases) <= 8000, name


# ------------------------------------------------------------------------------------------------ the base operation, independently
def test_base_operation_against_the_host_fpu():
    """The model's single IEEE operation against this machine's binary64 arithmetic (add, sub, mul, div, sqrt: correctly rounded
    by IEEE 754), and its binary32 form against the same operation made in binary64 and rounded to binary32 -- for p = 24 inside
    p' = 53 >= 2 p + 2 that double rounding is innocuous for + - * / sqrt (Figueroa).  Operands: normal, subnormal, near ties."""
    import random
    import struct
    rng = random.Random(77)
    r32 = lambda x: struct.unpack("<f", struct.pack("<f", x))[0]
    same = lambda x, y: struct.pack("<d", x) == struct.pack("<d", y)
    for _ in range(4000):
        a, b = C.rfloat(rng, M.F64, -40, 40), C.rfloat(rng, M.F64, -40, 40)
        if rng.random() < 0.2:
            a, b = C.rsub(rng, M.F64), C.rfloat(rng, M.F64, -1022, -1000)
        if rng.random() < 0.2:
            a, b = C.near_tie_quotient(rng, M.F64)
        assert same(M.add(M.F64, a, b), a + b) and same(M.sub(M.F64, a, b), a - b)
        assert same(M.mul(M.F64, a, b), a * b) and same(M.div(M.F64, a, b), a / b)
        assert same(M.sqrt(M.F64, abs(a)), math.sqrt(abs(a)))
        x, y = C.rfloat(rng, M.F32, -30, 30), C.rfloat(rng, M.F32, -30, 30)
        if rng.random() < 0.2:
            x, y = C.rsub(rng, M.F32), C.rfloat(rng, M.F32, -126, -100)
        if rng.random() < 0.2:
            x, y = C.near_tie_quotient(rng, M.F32)
        assert same(M.add(M.F32, x, y), r32(x + y)) and same(M.sub(M.F32, x, y), r32(x - y))
        assert same(M.mul(M.F32, x, y), r32(x * y)) and same(M.div(M.F32, x, y), r32(x / y))
        assert same(M.sqrt(M.F32, abs(x)), r32(math.sqrt(abs(x))))
        r, rd = C.near_tie_radicand(rng, M.F32), C.near_tie_radicand(rng, M.F64)
        assert same(M.sqrt(M.F32, r), r32(math.sqrt(r))) and same(M.sqrt(M.F64, rd), math.sqrt(rd))
    # signs of zero and the directed rounding, by the standard's rules
    z, nz = 0.0, -0.0
    assert same(M.add(M.F32, 1.5, -1.5), z) and same(M.add(M.F32, nz, nz), nz) and same(M.add(M.F32, z, nz), z)
    assert same(M.add(M.F32, 1.5, -1.5, down=True), nz) and same(M.mul(M.F32, nz, 3.0), nz) and same(M.div(M.F32, nz, -3.0), z)
    assert same(M.fma(M.F32, 2.0, 3.0, -6.0), z) and same(M.fma_down(M.F32, 2.0, 3.0, -6.0), nz)
    assert same(M.fma(M.F32, nz, 3.0, nz), nz) and same(M.fma(M.F32, nz, 3.0, z), z) and same(M.fma_down(M.F32, nz, 3.0, z), nz)
    assert same(M.fma_down(M.F32, 1.0, 1.0, 2.0 ** -30), 1.0) and same(M.fma(M.F32, 1.0, 1.0 + 2.0 ** -23, 2.0 ** -24), 1.0 + 2.0 ** -22)
    assert same(M.fma_down(M.F32, -1.0, 1.0, -2.0 ** -30), -(1.0 + 2.0 ** -23)) and same(M.fma_down(M.F32, 2.0 ** -100, 2.0 ** -100, z), z)
    assert same(M.fma_down(M.F32, -2.0 ** -100, 2.0 ** -100, z), -M.F32.tiny) and same(M.mul(M.F32, 2.0 ** -100, 2.0 ** -50), z)
    assert same(M.mul(M.F32, 2.0 ** -100, -1.5 * 2.0 ** -50), -M.F32.tiny) and M.mul(M.F32, 2.0 ** 100, 2.0 ** 100) == math.inf
    assert same(M.sqrt(M.F64, nz), nz)


# ------------------------------------------------------------------------------------------------ arm coverage
# Every arm the model can report, reached by the committed cases.  The list cannot shrink silently: it is compared for equality.
# All four gap arms and the zero reset of hr_add / hr_sub, the four arms of hc_add / hc_add_real, the early returns of the reduces,
# both arms of q_split(double) and all eight zero-test outcomes of q_renorm<double> (q_renorm<float> has none: one arm) are in it;
# no arm of the model is left out.
_F = ("f32", "f64", "df32")
EXPECTED_ARMS = sorted(
    [("hr_add_" + f, a) for f in _F for a in ("a_dominates_early_return", "scale_b", "scale_a", "b_dominates", "zero_resets_exponent")] +
    [("hr_sub_" + f, a) for f in _F for a in ("a_dominates_early_return", "scale_b", "scale_a", "b_dominates", "zero_resets_exponent")] +
    [(fn + f, a) for fn in ("hc_add_", "hc_add_real_") for f in _F for a in ("a_dominates_early_return", "scale_b", "scale_a", "b_dominates")] +
    [("hr_reduce_" + f, a) for f in ("f32", "f64") for a in ("zero_keeps_exponent", "normal", "subnormal")] +
    [("hr_reduce_df32", a) for a in ("zero_keeps_exponent", "tail_saturates", "tail_shifted")] +
    [("hc_reduce_" + f, a) for f in ("f32", "f64") for a in ("zero_keeps_exponent", "reduced", "both_subnormal_or_zero")] +
    [("hc_reduce_df32", a) for a in ("zero_keeps_exponent", "reduced")] +
    [("hr_from_number_" + f, a) for f in ("f32", "f64") for a in ("zero", "nonzero")] +
    [("hr2_from_float", a) for a in ("zero", "nonzero")] +
    [("multiplier_" + f, a) for f in ("f32", "f64") for a in ("zero", "pow2", "type_max")] +
    [("multiplier_df32", a) for a in ("zero_low", "pow2", "zero_high")] +
    [("multiplier_neg_" + f, a) for f in _F for a in ("zero", "pow2")] +
    [("clamp_exp", a) for a in ("clamped", "kept")] +
    [("fabs_bits_df32", a) for a in ("negated", "kept")] +
    [("bla_sqrt_" + f, a) for f in ("f32", "f64") for a in ("odd_exponent", "even_exponent")] +
    [("q_quick_two_sum_f32", "full"), ("q_two_sum_f32", "full"), ("q_split_f32", "plain"), ("q_renorm_f32", "no_zero_tests")] +
    [("q_quick_two_sum_f64", a) for a in ("full", "zero_shortcut")] + [("q_two_sum_f64", a) for a in ("full", "zero_shortcut")] +
    [("q_split_f64", a) for a in ("plain", "scaled_above_2^996")] +
    [("q_renorm_f64", a) for a in ("s1!=0,s2!=0,s3!=0", "s1!=0,s2!=0,s3==0", "s1!=0,s2==0,then s2!=0", "s1!=0,s2==0,then s2==0",
                                   "s1==0,then s1!=0,s2!=0", "s1==0,then s1!=0,s2==0", "s1==0,then s1==0,then s1!=0",
                                   "s1==0,then s1==0,then s1==0")] +
    [("q_le_" + f, "decided_%s_at_word_%d" % (w, k)) for f in ("f32", "f64") for w in ("less", "greater") for k in range(3)] +
    [("q_le_" + f, "decided_at_last_word") for f in ("f32", "f64")] +
    [("q_le_scalar_" + f, a) for f in ("f32", "f64") for a in ("head_less", "head_equal_y_decides", "head_greater")])
# an arm must be taken by more than a stray case
MIN_PER_ARM = 4


def test_arm_coverage():
    arms = {}
    for name in C.FAMILIES:
        C.build(name)
        for k, v in C.FAMILIES[name].arms.items():
            arms[k] = arms.get(k, 0) + v
    assert sorted(arms) == EXPECTED_ARMS, (sorted(set(EXPECTED_ARMS) - set(arms)), sorted(set(arms) - set(EXPECTED_ARMS)))
    thin = {k: v for k, v in arms.items() if v < MIN_PER_ARM}
    assert not thin, thin


# ------------------------------------------------------------------------------------------------ value checks
def _result_words(host, i):
    """the host's words where the host program evaluates the entry, the model's for the device-only entries (the GPU test holds the
    device to those bit for bit)"""
    return host[3][i] if host[1][i].op.host else host[1][i].out_words


@pytest.mark.parametrize("family", ["hdr_f32", "hdr_f64", "bla"])
def test_values_within_the_derived_bounds(host, family):
    """hreal / hcplx with F = float or double, and the square-root users: |result - exact| within the bound derived from the number
    of roundings (the derivations stand beside the bounds, tests/_arith_values.py)"""
    _, cases, where, _ = host
    checked, bad = {}, []
    for i in where[family]:
        b = V.bound(cases[i], _result_words(host, i))
        if b is None:
            continue
        checked[cases[i].op.name] = checked.get(cases[i].op.name, 0) + 1
        if b[0] > b[1]:
            bad.append(describe(cases[i], _result_words(host, i)) + " | error %.3e allowed %.3e" % (float(b[0]), float(b[1])))
    assert not bad, "%d results out of bound, first:\n%s" % (len(bad), "\n".join(bad[:10]))
    print(family, checked)
    want = {"hdr_f32": 13, "hdr_f64": 13, "bla": 4}[family]
    assert len(checked) == want and min(checked.values()) >= 20, checked


# Worst relative error of the double-word / expansion results over the committed cases (classes without cancellation: "pairs",
# "expansions", "two_sum_and_squares"; additions with operands of one sign), measured on the model's results, as log2.  Nobody has a
# proven bound for these sequences; the assertion is the measured figure plus one binade.
MEASURED_LOG2 = {
    "df32_add": -47.7, "df32_mul": -46.9,
    # +-60 binades of binary32 put the cross terms of the small products into the subnormal range: the squares' h * t, rounded on
    # its own, costs the most
    "dw_add_f32": -48.5, "dw_mul_f32": -43.6, "dw_sqr_f32": -30.0,
    "dw_add_f64": -106.6, "dw_mul_f64": -105.2, "dw_sqr_f64": -105.2,
    "q_add_f32": -100.1, "q_mul_scalar_f32": -98.7, "q_mul_f32": -95.4, "q_sqr_f32": -96.5,
    "q_add_f64": -215.6, "q_mul_scalar_f64": -214.7, "q_mul_f64": -212.1, "q_sqr_f64": -212.9,
}


@pytest.mark.parametrize("family", ["df32", "dw", "qd_f32", "qd_f64"])
def test_double_word_and_expansion_errors(host, family):
    _, cases, where, _ = host
    worst = {}
    for i in where[family]:
        r = V.relerr(cases[i], _result_words(host, i))
        if r is None:
            continue
        k = cases[i].op.name
        n, w = worst.get(k, (0, 0))
        worst[k] = (n + 1, max(w, r))
    figures = {k: (n, math.log2(w) if w else -math.inf) for k, (n, w) in worst.items()}
    print(family, {k: "%d cases, 2^%.1f" % v for k, v in figures.items()})
    mine = {k for k in MEASURED_LOG2 if C.OPS[k] in {c.op for c in C.build(family)}}
    assert set(figures) == mine, (sorted(figures), sorted(mine))
    for k, (n, lg) in figures.items():
        assert n >= 50, (k, n)
        assert lg <= MEASURED_LOG2[k] + 1.0, (k, lg, MEASURED_LOG2[k])
