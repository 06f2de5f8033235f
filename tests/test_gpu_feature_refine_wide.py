"""features.refine_found(wide=True) on the GPU: found points refined to nuclei by the secant loop of exact.refine_points with
fs_exact_eval_points_wide as its evaluator, past the lane path's 758 fractional bits -- View 11's 2 550 and View 14's 21 829 among
them -- against the same loop on Python integers (tests/_point_model.py).  Equalities of integers only."""
from fractions import Fraction

import pytest

import _point_model as model
from fractalshark_amd import GPURenderer, exact, features

pytestmark = pytest.mark.gpu

OFFSET = "1e-3"
ROUNDS = 24  # (with the default 16 the two deepest precisions end as "rounds": the secant loop gains about 1.6 times the bits a round)
KEYS = ("status", "c", "atom", "evaluations", "converged", "log2")


@pytest.fixture(scope="module")
def renderer(native_libs):
    assert GPURenderer.TestCudaIsWorking() != 0, "no usable HIP device: the product path has no CPU fallback"
    r = GPURenderer(0)
    yield r
    r.close()


def _decimal(q):
    """A Fraction with a power-of-ten denominator as a decimal string."""
    digits = 40
    v = q * 10 ** digits
    assert v.denominator == 1
    s = str(abs(v.numerator)).rjust(digits + 1, "0")
    return ("-" if q < 0 else "") + s[:-digits] + "." + s[-digits:]


def _scaled(text, F):
    """value * 2^F of a finite decimal string of any length, which must be an integer (Python reads no more than 4300 digits into
    an int in one go)."""
    neg = text.startswith("-")
    whole, _, frac = text.lstrip("-").partition(".")
    digits, n = whole + frac, 0
    for i in range(0, len(digits), 4000):
        chunk = digits[i:i + 4000]
        n = n * 10 ** len(chunk) + int(chunk)
    q, rem = divmod(n << F, 10 ** len(frac))
    assert rem == 0
    return -q if neg else q


def _found():
    """Periods 1 .. 5 as found-point dicts next to their nuclei, the offset as their intrinsic radius."""
    o = Fraction(OFFSET)
    return [{"cx": _decimal(Fraction(x) + o), "cy": _decimal(Fraction(y) + o / 2), "period": p, "intrinsic_radius": OFFSET}
            for p, x, y in model.SMALL_NUCLEI]


@pytest.mark.parametrize("F", [790, 2550, 4118, 21829])
def test_small_nuclei_beyond_the_lane_path(renderer, F):
    """25, 80, 129 and 683 limbs: every field the model's, every point fixed and converged with atom == period."""
    assert exact.limbs_for(F) == {790: 25, 2550: 80, 4118: 129, 21829: 683}[F]
    found = _found()
    got = features.refine_found(renderer, found, frac_bits=F, rounds=ROUNDS, wide=True)
    assert len(got) == len(found)
    for pt, g in zip(found, got):
        c0, delta, p = model.fixture_point(pt, F)
        want = model.refine(c0, delta, p, F, rounds=ROUNDS)
        assert {k: g[k] for k in KEYS} == {k: want[k] for k in KEYS}, (F, p, g["status"], want["status"], g["evaluations"])
        assert g["period"] == p and g["status"] == "fixed" and g["converged"] and g["atom"] == p
        assert (_scaled(g["cx"], F), _scaled(g["cy"], F)) == g["c"]
    print("F %5d: evaluations %s" % (F, [g["evaluations"] for g in got]))


def test_the_two_paths_agree(renderer):
    """At 246 bits, where both paths run: field for field the same."""
    found = _found()
    lane = features.refine_found(renderer, found, frac_bits=246, wide=False)
    wide = features.refine_found(renderer, found, frac_bits=246, wide=True)
    assert wide == lane and all(g["converged"] for g in wide)
    with pytest.raises(ValueError):
        features.refine_found(renderer, found, frac_bits=exact.MAX_WIDE_FRAC_BITS + 1, wide=True)
    with pytest.raises(ValueError):  # (without the keyword the limit is where it was)
        features.refine_found(renderer, found, frac_bits=exact.MAX_FRAC_BITS + 1)
