"""The orbits of tests/test_quiet_model_cpu.py, tests/test_gpu_quiet_orbit.py and tests/golden/make_quiet_orbit_counts.py, by name (64x36: the
orbit does not depend on the frame size).  The views and the three crafted orbits of the NDZ tests come from
test_gpu_lav2_ndz_tight._inputs, so a suite builds them once; the edge orbits are View 5's entries with a handful of them rewritten in
its middle, 48 entries apart (no window of the tables -- at most 19 entries -- sees two edits; the ramp's are consecutive), handed to the
renderer as they are."""
import functools
import os
from decimal import Decimal, getcontext

import numpy as np

from fractalshark_amd import inputs

REAL = ["view5_64x36", "view3_64x36", "shallow_1e-12", "period2_centre", "period3_bulb_50"]
NDZ_CRAFTED = ["view5_64x36_crafted", "view5_64x36_crafted_mild", "view5_64x36_nearaxis"]
EDGES = ["view5_edges_bound", "view5_edges_exponent", "view5_edges_never_behind", "view5_edges_ramp"]
ALL = REAL + NDZ_CRAFTED + EDGES
TINY = {"period2_centre": ("-1.0", "0.0", "1e-5", 40), "period3_bulb_50": ("-0.1225", "0.7448", "1e-4", 50)}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quiet_orbit_counts.json")
KMIN = -268435456   # the exponent of an exact zero
SPACING = 48
F = np.float32


class ArrayOrbit:
    """Entries as a numpy array in the place of an inputs.Orbit (GPURenderer.InitializePerturb takes anything with data_ptr / count /
    period)."""
    is64 = compressed = False

    def __init__(self, entries, edited):
        self._e = np.ascontiguousarray(entries)
        self.count, self.period, self.edited = len(entries), 0, edited

    @property
    def data_ptr(self):
        return self._e.ctypes.data

    def entries(self):
        return self._e.copy()


def _below(v):
    return float(np.nextafter(F(v), F(0)))


def _edits(name):
    """[(mx, ex, my, ey)]: what the edited entries become, in order"""
    half = 0.5
    if name == "view5_edges_bound":
        return [
            # the larger part just below 5.6 and on it (5.6 = 0.7 * 2^3 = 1.4 * 2^2 in binary32, either way of writing the mantissa)
            (_below(0.7), 3, half, 0), (float(F(0.7)), 3, half, 0), (half, 0, -_below(1.4), 2), (half, 0, -float(F(1.4)), 2),
            # zmax on 2^-40 and a binade below
            (half, -39, half, -41), (half, -40, half, -41),
            # min part / max part on 2^-40 and a binade beyond
            (-half, 0, half, -40), (half, -41, -half, 0),
            # an exponent above 2: the poison of the first companion (4 is within the bound, 16 is not)
            (half, 3, half, 1), (half, 5, half, 5)]
    if name == "view5_edges_exponent":
        return [
            # below the clamp of the bounds (-200) and of .w (-1000); .w overflows from e = -60 down, 2^126 at -59
            (half, -250, half, -251), (half, -1100, -half, -1100), (half, -2000, half, -1001), (half, -60, half, -62),
            (half, -59, half, -59), (half, -126, half, -130), (half, -150, half, -151),
            # an exact zero mid-orbit: nothing may arrive at it, a run may start there
            (0.0, KMIN, 0.0, KMIN),
            # one part an exact zero
            (half, 0, 0.0, KMIN), (0.0, KMIN, -half, -3)]
    if name == "view5_edges_never_behind":
        # isolated entries nothing may arrive at: every window that holds one at any distance 1 .. 19 is taken
        return [(half, -60 - k, half, -61) for k in range(8)]
    assert name == "view5_edges_ramp"
    # CONSECUTIVE entries: an exact zero, then |Z| doubling from 2^-4.  The block that starts on the zero is the one whose bound the
    # FIRST arrival decides (own[j + 1] / g_j is the smallest quotient), with dz' = dz^2 + dc: max|dz'| reaches 2 G^2 + G, which the
    # constant 3.8 = 2 * 1.4 + 1 of the growth is there for
    return [(0.0, KMIN, 0.0, KMIN)] + [(half, k - 3, -half, k - 3) for k in range(4)]


def _tiny_view(cx, cy, w, n, W=64, H=36):
    getcontext().prec = 50
    cx, cy, w = Decimal(cx), Decimal(cy), Decimal(w)
    h = w * H / W
    return inputs.View(str(cx - w / 2), str(cy - h / 2), str(cx + w / 2), str(cy + h / 2), W, H, num_iterations=n)


@functools.lru_cache(maxsize=None)
def orbit(name):
    """-> an inputs.Orbit or an ArrayOrbit"""
    if name in TINY:
        return inputs.Orbit(_tiny_view(*TINY[name]))
    import test_gpu_lav2_ndz_tight as tight
    if name not in EDGES:
        return tight._inputs(name)[1]
    e = tight._inputs("view5_64x36")[1].entries()
    ed = _edits(name)
    at = len(e) // 2 + (1 if name == "view5_edges_ramp" else SPACING) * np.arange(len(ed))
    for i, (mx, ex, my, ey) in zip(at, ed):
        e[i] = (mx, ex, ey, my)
    return ArrayOrbit(e, at)


# ---- the scaled kernels' orbit pair (PerturbExtras::Bad): the HDRFloat<float> entries with their flags and the binary32 copy
HDR32_BAD = np.dtype([("bad", "<u4"), ("padding", "<u4"), ("mx", "<f4"), ("ex", "<i4"), ("ey", "<i4"), ("my", "<f4")])
F32_BAD = np.dtype([("bad", "<u4"), ("padding", "<u4"), ("x", "<f4"), ("y", "<f4")])
SCALED = ["view5_64x36", "view5_scaled_edges", "view14_64x36"]


@functools.lru_cache(maxsize=None)
def scaled_pair(name):
    """-> (HDR32_BAD array, F32_BAD array) as fs_upload_orbit_scaled takes them.  view5_scaled_edges: View 5's pair with `bad` flags set
    and the larger part of binary32 entries put on the edges of [2^-40, 5.6) in its middle; view14_64x36 has `bad` entries of its own."""
    import ctypes as C
    import test_gpu_lav2_ndz as base
    ob = base._inputs("view5_64x36" if name == "view5_scaled_edges" else name)[1]
    t = np.frombuffer((C.c_uint8 * (ob.count * HDR32_BAD.itemsize)).from_address(ob.bad_data_ptr), HDR32_BAD).copy()
    f = np.frombuffer((C.c_uint8 * (ob.count * F32_BAD.itemsize)).from_address(ob.bad_f32_data_ptr), F32_BAD).copy()
    if name == "view5_scaled_edges":
        mid = ob.count // 2
        for k, (x, y) in enumerate([(_below(5.6), 1.0), (float(F(5.6)), 1.0), (-1.0, -_below(5.6)), (0.5, float(F(5.6))),
                                    (2.0 ** -40, 0.0), (2.0 ** -41, 2.0 ** -50), (0.0, -2.0 ** -40), (0.0, 0.0), (-0.0, 2.0 ** -140),
                                    (float("inf"), 1.0), (1.0, float("nan"))]):
            f["x"][mid + 3 * k], f["y"][mid + 3 * k] = x, y
        for i in (mid - 7, mid - 6, 1, ob.count - 2):
            t["bad"][i] = f["bad"][i] = 1
    return t, f
