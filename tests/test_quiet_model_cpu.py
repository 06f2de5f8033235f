"""The plain model of the tuned LAv2 loop's orbit companions (tests/_quiet_model.py) against what the bounds are FOR, without a GPU.
tests/test_gpu_quiet_orbit.py holds the device's tables to this model bit for bit; here the model itself is held, on every orbit of
tests/_quiet_orbits.py:

  (a) Definition.  Every entry j with a block bound is started from states with max(max|dz|, max|dc|) ON the bound -- the corner and
      seeded random states of the NDZ test, each row scaled so that its largest component is exactly the bound -- and stepped four times
      in binary32 as the full form steps (s = fl(fma(w, 2^E, 2Z)) evaluated in binary64 and rounded once, two products and a sum per
      part, then + dc): every arrival's max|dz| is within the own bound of the entry it arrives at.  The same for the words of zqb
      against the blocks they license (check_zqb), and for the sixteen-step chain as FS_FAST_LOOP_FD16P tests it (a body that starts
      with the state at entry j reads zqb[j + 1]; its blocks are licensed by .w of entry j, then .x / .y / .z of that record against
      the states after 4 / 8 / 12 steps): wherever all four tests pass, all sixteen arrivals pass theirs.  Started ON the first bound
      and 2^-12, 2^-24 below it, and not vacuous: bodies pass all four tests on every orbit that has block bounds.
  (b) Purpose.  At every arrival of (a), and for dz ON the own bound of every entry that has one, |Z + dz|^2 >= |dz|^2 (no rebase) and
      |Z + dz|^2 < 256 (no escape), decided exactly (a binary64 evaluation where its error bound leaves no doubt, fractions.Fraction
      elsewhere); for the scaled kernels' M / 4, |z|^2 >= 3.3 |dz|^2 and |z|^2 < 115.
  (c) Teeth.  Three mutants of the model fail (a):
        growth constant 3.8 -> 1.0          caught on view5_edges_ramp alone (the block that starts on its exact zero: dz' = dz^2 + dc reaches
                                            2 G^2 + G where the first arrival decides the bound; on the views' own orbits a later arrival
                                            decides it and the worst case of one step cannot repeat in the next);
        arrival index bound[j + k]          caught on every orbit that has block bounds (view5_64x36, view3_64x36, shallow_1e-12,
                                            period3_bulb_50 and every crafted one);
        zqb offsets 4, 8, 12, 16            caught by check_zqb on view5_64x36, view3_64x36, shallow_1e-12 and every orbit crafted from
                                            View 5, by the sixteen-step chain too on all of those but shallow_1e-12; NOT on
                                            period3_bulb_50 (period 3: neighbouring block bounds agree to within the bounds' slack).
  (d) Fixture.  tests/golden/quiet_orbit_counts.json (tests/golden/make_quiet_orbit_counts.py writes it from this model) holds per orbit
      the entries with an own bound, a block bound and NDZ bounds: the model reproduces it, every orbit meant to have bounds has more than
      zero of each, and the orbits that cannot are listed with the reason."""
import json

import numpy as np
import pytest

import _quiet_model as qm
import _quiet_orbits as qo

MUTANTS = {"growth": dict(growth=1.0), "arrival": dict(arrival_shift=0), "zqb": dict(zqb_offsets=(4, 8, 12, 16))}
# which orbit is held to catch which mutant (the docstring says why); every other pair is free to
CATCHES = {"growth": ["view5_edges_ramp"],
           "arrival": ["view5_64x36", "view3_64x36", "shallow_1e-12", "period3_bulb_50", "view5_edges_ramp"],
           "zqb": ["view5_64x36", "view3_64x36", "shallow_1e-12", "view5_edges_ramp"]}


def _states():
    return qm.on_the_bound(qm.start_states(np.random.default_rng(9)))


_prepared = {}


def _prep(name):
    if name not in _prepared:
        _prepared[name] = qm.prepared(qo.orbit(name).entries())
        _prepared[name].setflags(write=False)
    return _prepared[name]


def _violations(t, st, purpose=None):
    """(a) on the tables t -> (violations by check, blocks started, bodies x rows passing all four tests)"""
    blocks, bad = qm.check_blocks(t.second, t.block, 0, st, purpose)
    _, bad_q = qm.check_zqb(t.second, t.zqb, st)
    passed, bad_16 = qm.check_bodies16(t.second, t.zqb, st)
    return {"blocks": bad, "zqb": bad_q, "bodies16": bad_16}, blocks, passed


@pytest.mark.parametrize("name", qo.ALL)
def test_definition_and_purpose(native_libs, name):
    t = qm.Tables(_prep(name))
    st = _states()
    c = t.counts()
    bad, blocks, passed = _violations(t, st, qm.own_purpose)
    print("quiet-model %-26s entries %d  own %d  block %d  ndz %d  bodies x rows through all four tests %d"
          % (name, t.n, c["own"], c["block"], c["ndz"], passed))
    assert not any(bad.values()), {k: v[:6] for k, v in bad.items()}
    assert blocks == c["block"]
    assert (passed > 0) == (c["block"] > 0)
    assert qm.check_own_purpose(t.second, st) == c["own"]
    # the structural identities
    assert np.array_equal(qm.bits(t.zs2[:t.n]), qm.bits(t.second[:, :2]))
    assert qm.check_zqb(t.second, t.zqb, st)[0] == 0
    assert (qm.bits(t.zs2[t.n:]) == 0).all() and (qm.bits(t.zqb[t.n:]) == 0).all() and (qm.bits(t.znz[t.n:]) == qm.NEVER).all()
    # NDZ bounds come in pairs and only where both block bounds of the body exist
    assert np.array_equal(qm.is_never(t.znz[:, 0]), qm.is_never(t.znz[:, 1]))
    has = ~qm.is_never(t.znz[:t.n, 0])
    assert not (has & qm.is_never(t.block)).any()


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_mutants_fail_the_definition(native_libs, mutant):
    st = _states()
    for name in CATCHES[mutant]:
        bad, _, _ = _violations(qm.Tables(_prep(name), **MUTANTS[mutant]), st)
        n = {k: len(v) for k, v in bad.items()}
        print("quiet-model mutant %-8s on %-20s violations %s" % (mutant, name, n))
        assert sum(n.values()) > 0, (mutant, name)
        if mutant == "zqb":
            assert n["zqb"] > 0 and n["blocks"] == 0, n
            if name != "shallow_1e-12":
                assert n["bodies16"] > 0, n
        else:
            assert n["blocks"] > 0, n


def test_purpose_is_decided_exactly_on_its_edges():
    """where binary64 cannot tell (|Z + dz|^2 on |dz|^2 or on the cap, and an ulp of binary32 either side) fractions.Fraction does"""
    from fractions import Fraction
    t = 2.0 ** -30
    #                      on the ratio      just inside       just outside      on the cap   just below it       far inside
    zx = np.array([1.0, 1.0, 1.0, 16.0, 16.0 - 2.0 ** -20, 1.0])
    ux = np.array([-0.5, -0.5 + t, -0.5 - t, 0.0, 0.0, 0.25])
    zero = np.zeros_like(zx)
    bad, exact = qm.purpose_violations(zx, zero, ux, zero, Fraction(1), 256)
    assert bad == [(2,), (3,)] and exact >= 3
    # the scaled kernels' ratio: |z|^2 = 3.3 |dz|^2 is not representable, so either side of it
    z = np.array([1.0, 1.0])
    u = np.array([-0.355, -0.356])   # |1 + u|^2 / u^2 = 3.3012.., 3.2724..
    bad, _ = qm.purpose_violations(z, 0 * z, u, 0 * z, Fraction(33, 10), 115)
    assert bad == [(1,)]


@pytest.mark.parametrize("name", qo.SCALED)
def test_scaled_word_purpose(native_libs, name):
    _, f = qo.scaled_pair(name)
    words = qm.scaled_words(f)
    usable, bad = qm.check_scaled_purpose(f, words, _states())
    print("quiet-model scaled %-20s entries %d  with a bound %d  bad %d" % (name, len(f), usable, int((f["bad"] != 0).sum())))
    assert not bad, bad[:6]
    assert usable > 0
    never = words == qm.bits(np.array([-1.0], np.float32))[0]
    assert never[-1] and never[f["bad"] != 0].all()
    if name != "view5_64x36":
        assert (f["bad"] != 0).any()


def test_counts_fixture(native_libs):
    golden = json.load(open(qo.GOLDEN))
    assert sorted(golden["orbits"]) == sorted(qo.ALL)
    for name in qo.ALL:
        assert qm.Tables(_prep(name)).counts() == {k: golden["orbits"][name][k] for k in ("own", "block", "ndz")}, name
        if name in golden["without_bounds"]:
            assert golden["orbits"][name] == dict(golden["orbits"][name], own=0, block=0, ndz=0) and golden["without_bounds"][name]
        else:
            assert min(golden["orbits"][name][k] for k in ("own", "block", "ndz")) > 0, name
    assert sorted(golden["without_bounds"]) == ["period2_centre"]
