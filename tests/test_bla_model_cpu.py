"""CPU: the plain model of the BLA lookup and of the device's derived tables (tests/_bla_model.py), before any GPU is involved.

1. The model's lookup_backwards is pinned to the golden-pinned text: the oracle's LookupBackwards (oracle/cpu_ref.cpp, the function
   its Cpu32PerturbedBLAHDR / Cpu64PerturbedBLAHDR frames call), exported through liboracle.so, answers the whole question set of
   every table exactly as the model does.
2. On the model's own derived tables, the walk over Q and the heap -- and the walk over the ladder and the pre-test keys -- gives
   lookup_backwards' answer for every question: the model reads the layouts correctly.
3. The question set reaches every class of lookup (printed per M; run with -s to see the counts).

One class is empty and is asserted to be empty, not dropped: "a miss that passes the pre-test and runs out of levels".  The
pre-test key of an index is the largest r2 among exactly the records the walk at that index probes (the walk depends on m alone),
so z2 below it means z2 is below the r2 of the record that owns the maximum, and that probe -- or an earlier one -- holds.  The
class could only be reached at an index whose walk would leave a level (key INT64_MAX), which lies beyond the orbit's last entry
(k < count - 1 keeps k >> L inside level L for every L) and which the reference-layout lookups cannot be asked.  That it stays
empty on tables read back from the device is what shows that no pre-test key there is too large."""
import numpy as np
import pytest

import _bla_model as bm
import _oracle

VIEWS = (19, 5)


def _cases_of(view_n, is64):
    # (+ a table no builder makes, in which the gate of the first index decides: see _bla_model._table_edit_wide_first_elements)
    return [bm.case(view_n, M, is64) for M in bm.M_SET] + [bm.case(view_n, M, is64, "wide_first") for M in (33, 1025)]


def test_inputs_have_the_shapes_the_case_set_was_chosen_for(native_libs):
    for view_n in VIEWS:
        got = [(bm.case(view_n, M).tab.n_levels, bm.case(view_n, M).tab.lm2) for M in (1, 2, 3, 4, 5)]
        assert got == [(1, 0), (2, 0), (3, 1), (3, 1), (4, 2)]
        assert bm.case(view_n, 4099).tab.sizes == [0, 0, 1025, 513, 257, 129, 65, 33, 17, 9, 5, 3, 2, 1]      # ragged at every level
        assert bm.case(view_n, 1024).tab.sizes == [0, 0, 256, 128, 64, 32, 16, 8, 4, 2, 1]                    # ragged nowhere


@pytest.mark.parametrize("is64", [False, True])
@pytest.mark.parametrize("view_n", VIEWS)
def test_model_lookup_equals_the_oracles_lookup_on_every_question(native_libs, view_n, is64):
    asked = 0
    for c in _cases_of(view_n, is64):
        if c.tab.n_levels <= bm.FIRST_LEVEL:
            # (the reference's text reads the first record of level 2, which such a table does not have: never looked up in)
            assert all(not bm.probes(c.tab.lm2, m) for m in range(c.orbit.count))
            continue
        m, z2 = bm.pack_questions(c.questions, is64)
        assert np.array_equal(_oracle.bla_lookup(c.bla, m, z2), c.answers), c.M
        # the walk's list of probes is the lookup's: the first that holds is its answer
        for (mm, z), a in zip(c.questions, c.answers):
            pr = bm.probes(c.tab.lm2, mm)
            first = next(((L, ix) for (L, ix) in pr if z < c.tab.r2[L][ix]), None)
            if mm == 1 and not z < c.tab.r2[2][0]:
                first = None
            assert (tuple(int(x) for x in a) if a[0] != 0xFFFFFFFF else None) == first
        asked += len(m)
    assert asked > 40000


@pytest.mark.parametrize("view_n", VIEWS)
def test_walks_over_the_models_own_tables_answer_as_the_lookup(native_libs, view_n):
    for c in _cases_of(view_n, False):
        if c.tab.n_levels <= bm.FIRST_LEVEL:
            continue
        d = c.derived
        assert not d.bad
        for (m, z), a in zip(c.questions, c.answers):
            want = tuple(int(x) for x in a) if a[0] != 0xFFFFFFFF else None
            zk = bm.zkey_of(z)
            p = bm.walk_native(d.ladder, d.pretest, d.level_off, d.tab.lm2, m, zk)
            assert (None if p is None else bm.native_level_ix(d.level_off, d.level_n, p)) == want, (c.M, m, z)
            if d.H:
                slow = lambda mm, kk: pytest.fail("a Q entry of level 0 inside the orbit")
                assert bm.walk_heap(d.q, d.heap_ladder, d.H, m, zk, slow) == want, (c.M, m, z)


def test_every_class_of_lookup_is_reached(native_libs):
    total = dict.fromkeys(bm.CLASSES, 0)
    for view_n in VIEWS:
        for c in _cases_of(view_n, False):
            if c.tab.n_levels <= bm.FIRST_LEVEL:
                continue
            n = dict.fromkeys(bm.CLASSES, 0)
            for (m, z) in c.questions:
                for k in bm.classify(c.tab, m, z):
                    n[k] += 1
            print("view %2d M %4d: %6d questions  " % (view_n, c.M, len(c.questions)) +
                  " ".join("%s=%d" % (k, n[k]) for k in bm.CLASSES))
            if c.M < 1025:
                assert n["hit_round_3"] == 0  # (needs a start level of 10)
            for k in bm.CLASSES:
                total[k] += n[k]
    print("all: " + " ".join("%s=%d" % (k, total[k]) for k in bm.CLASSES))
    for k in bm.CLASSES:
        if k == "miss_passes_pretest":
            assert total[k] == 0, "unreachable by the argument of this module's docstring"
        else:
            assert total[k] > 0, k


def test_poison_classes_of_the_derived_tables_are_reached(native_libs):
    """What tests/test_gpu_bla_tables.py compares byte for byte holds an element of every poison class that an orbit can reach.
    Not reachable: a coefficient mantissa beyond 2^30.  Every coefficient of a level from 2 up is the reduced result of a merge
    (bla_math.hpp: |mantissa| < 2), or -- the single-step record a ragged end carries up -- an orbit mantissa times one or the
    constants 1 and 0; Orbit.scale_entries / scale_parts move exponents only.  (A coefficient exponent at or below -2^26 IS
    reached: the exact zero of a record on the real axis.)"""
    seen = dict.fromkeys(("leaves", "last_entry", "arrival_high", "arrival_low", "exponent", "q_level_0", "zb_0", "zb_1", "zb_2"),
                         0)
    for c in [bm.case(19, M) for M in bm.M_SET] + [bm.case(19, M, False, "window") for M in (17, 65, 257)]:
        if c.tab.n_levels <= bm.FIRST_LEVEL or not c.derived.H:
            continue
        d = c.derived
        for k in ("leaves", "last_entry", "arrival_high", "arrival_low", "exponent"):
            seen[k] += int(d.reasons[k].sum())
        assert not d.reasons["mantissa"].any()
        seen["q_level_0"] += int((d.q["lvl"] == 0).sum())
        for kind in range(3):
            seen["zb_%d" % kind] += int((d.zb_kind == kind).sum())
    print(seen)
    assert all(v > 0 for v in seen.values()), seen
