"""The add-free back-off of FS_FAST_LOOP_FDU that follows what happened (csrc/scaled_runs.hpp: kNdBackoffEntry, kNdBackoffVerdict,
nd_backoff_refused; the run entry in csrc/kernels_lav2_hdr32.hip).

After an entry vote that refused the add-free form, or a verdict that failed, a wave sits out `pen` runs before it asks again: pen
starts at 0 (it asks at the very next run), doubles with every further refusal or failure in a row (1, 2, 4, ..), is capped at 8 runs
after a refused vote and 32 after a failed verdict, and goes back to 0 when an add-free invocation with steps passes its verdict.  The
parent commit sat out 8 / 32 runs after the first refusal / failure.  Which form a run takes changes no result.  What is held here:

  1. the frames are what they were: tuned == literal variant == CPU oracle on View 5 at 64x36 (both stage-test directions), View 3 and
     the generated shallow views, no replay mismatch;
  2. a shallow view does not pay for the quicker asking: at a width of 1e-6 no add-free step is taken and no verdict fails; at 1e-12 no
     add-free invocation is accepted with steps, and the failed verdicts stay within the doubling schedule's bound -- per wave
     ceil(log2 cap) on the way up and one per cap runs after that, cap = kNdBackoffVerdict = 32, summed over the launch's waves with the
     run count of the counting launch itself (word 13: runs started, per wave);
  3. on View 5 at 64x36 the statement's full-form wave-steps taken while a wave was backing off (word 36; word 37 = those among them
     whose entry vote would have passed) are fewer than all its full-form wave-steps, and the full form's share is not above the
     parent's 149 032 of 838 004 (profiles/r08_ndz_ab.json).

Statistics words (fs_read_stats_raw): 8 = four-step blocks taken inside the statement, 13 = runs started (per wave), 30 = add-free
wave-steps, 32 = failed ND verdicts, 33 = replay mismatches, 34 = invocations replayed, 36 / 37 see above."""
import math

import numpy as np
import pytest

import test_gpu_lav2_ndz as base
from fractalshark_amd import GPURenderer, LAV2_FULL, PARITY_CPU, PARITY_CPU_GPUSTAGE

pytestmark = pytest.mark.gpu

W_BLOCKS, W_WAVE_RUNS, W_ND, W_FAIL, W_MISMATCH, W_REPLAYED, W_BACKED_OFF, W_BACKED_OFF_OK = 8, 13, 30, 32, 33, 34, 36, 37
BACKOFF_VERDICT_CAP = 32  # kNdBackoffVerdict
PARENT_STATEMENT, PARENT_FULL = 838004, 149032  # View 5, 64x36, parity cpu: profiles/r08_ndz_ab.json (838 004 - 688 972 add-free)


@pytest.fixture(scope="module")
def renderer(native_libs):
    assert GPURenderer.TestCudaIsWorking() != 0, "no usable HIP device: the product path has no CPU fallback"
    r = GPURenderer(0)
    yield r
    r.enable_step_count(False)
    r.set_kernel_variant(0)
    r.close()


_counted = {}


def _counting(r, name, parity):
    if (name, parity) not in _counted:
        _counted[(name, parity)] = base._render(r, name, LAV2_FULL, parity, counting=True)
    return _counted[(name, parity)]


@pytest.mark.parametrize("name,parity", [("view5_64x36", PARITY_CPU), ("view5_64x36", PARITY_CPU_GPUSTAGE), ("view3_64x36", PARITY_CPU)] +
                         [(n, PARITY_CPU) for n in base.SHALLOW])
def test_frames_are_what_they_were(renderer, native_libs, name, parity):
    tuned, _ = base._render(renderer, name, LAV2_FULL, parity)
    lit, _ = base._render(renderer, name, LAV2_FULL, parity, literal=True)
    assert np.array_equal(tuned, lit), (name, parity, int((tuned != lit).sum()))
    ref = base._oracle_frame(name, LAV2_FULL, base._st(parity))
    assert np.array_equal(tuned, ref), (name, parity, int((tuned != ref).sum()))
    counted, raw = _counting(renderer, name, parity)
    assert np.array_equal(counted, tuned), (name, parity)
    statement = 4 * raw[W_BLOCKS]
    print("nd-backoff %-14s statement wave-steps %d  add-free %d  full form %d (backed off %d, vote would have passed %d)  "
          "failed verdicts %d  replayed %d  mismatches %d"
          % (name, statement, raw[W_ND], statement - raw[W_ND], raw[W_BACKED_OFF], raw[W_BACKED_OFF_OK], raw[W_FAIL], raw[W_REPLAYED],
             raw[W_MISMATCH]))
    assert raw[W_MISMATCH] == 0, (name, raw[W_MISMATCH])
    assert raw[W_ND] == 0 or raw[W_REPLAYED] > 0
    assert raw[W_BACKED_OFF_OK] <= raw[W_BACKED_OFF] <= statement - raw[W_ND], (raw[W_BACKED_OFF_OK], raw[W_BACKED_OFF], statement, raw[W_ND])


def test_shallow_1e6_takes_no_add_free_step(renderer, native_libs):
    _, raw = _counting(renderer, "shallow_1e-6", PARITY_CPU)
    assert raw[W_ND] == 0 and raw[W_FAIL] == 0, (raw[W_ND], raw[W_FAIL])
    assert 4 * raw[W_BLOCKS] > 0  # the full form carries the statement's steps


def test_shallow_1e12_failed_verdicts_stay_within_the_doubling_schedule(renderer, native_libs):
    name = "shallow_1e-12"
    v, _, _ = base._inputs(name)
    _, raw = _counting(renderer, name, PARITY_CPU)
    assert raw[W_ND] == 0, raw[W_ND]  # none accepted with steps
    # one wave per 64 pixels of a 32 x 8 tile; its back-off state lives as long as it does
    waves = ((v.width + 31) // 32) * ((v.height + 7) // 8) * 4
    runs = raw[W_WAVE_RUNS]
    bound = waves * math.ceil(math.log2(BACKOFF_VERDICT_CAP)) + runs / BACKOFF_VERDICT_CAP
    print("nd-backoff %s: %d waves, %d runs started, %d failed verdicts (bound %.1f)" % (name, waves, runs, raw[W_FAIL], bound))
    assert raw[W_FAIL] <= bound, (raw[W_FAIL], bound, waves, runs)


def test_view5_backed_off_steps_and_full_form_share(renderer, native_libs):
    _, raw = _counting(renderer, "view5_64x36", PARITY_CPU)
    statement = 4 * raw[W_BLOCKS]
    full = statement - raw[W_ND]
    print("View 5 64x36: statement wave-steps %d, full form %d (%.2f %%; parent %.2f %%), backed off %d, of those with a passing vote %d"
          % (statement, full, 100.0 * full / max(1, statement), 100.0 * PARENT_FULL / PARENT_STATEMENT, raw[W_BACKED_OFF],
             raw[W_BACKED_OFF_OK]))
    assert statement > 0 and raw[W_BACKED_OFF] < full, (raw[W_BACKED_OFF], full)
    assert full * PARENT_STATEMENT <= PARENT_FULL * statement, (full, statement)
