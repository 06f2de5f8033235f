"""fs_feature_eval_resident: the Feature Finder's PT evaluator on an orbit held as waypoints on the device.  The contract: the same
SimpleCompression orbit uploaded expanded (E) and as waypoints only (S) gives the same records, byte for byte, in every batch
of a whole scan -- the period search, every Newton round, the final passes -- and hence the same found points."""
import numpy as np
import pytest

from fractalshark_amd import GPURenderer, LAV2_FULL, PARITY_CPU, T_HDR32, T_HDR64, _capi, features, inputs
from fractalshark_amd.renderer import FS_ERR_UNSUPPORTED
from test_feature_finder_cpu import known_view
from test_gpu_feature_finder import rabbit_nucleus

pytestmark = pytest.mark.gpu

FS_ERR_6 = 10005
HIP_INVALID_VALUE = 1
CAP = 1 << 17
# (name, T, compression_exp, grid, sparse, diverges, finds).  "rabbit <half-width>": the generated views of
# test_gpu_feature_finder.py, around the period-3 nucleus, on the 12 x 12 grid and on that file's 13 x 13 one, whose middle point
# is the only one with the nucleus inside its search disc: at 12 x 12 every candidate is rejected in the search round.  Their
# orbits end at the period, four entries.  "view5": View 5, 16 046 entries.
#   sparse:   a fourth of the entries at most are waypoints, so the iterate-forward arm of the cursor's step carries most steps
#   diverges: the scan's records hold two or more distinct periods and at least one candidate is rejected or takes the Direct
#             fallback, so lanes leave lockstep, rebase at different steps and their cursors part
#   finds:    the scan goes past the search round, through Newton rounds and the final passes, and returns points
# All three were established on the host (inputs.Orbit, and the scan through the CPU checker of tests/feature) and are asserted.
CASES = [("rabbit 1e-8", T_HDR32, 20, 12, False, False, False), ("rabbit 1e-30", T_HDR32, 20, 12, False, False, False),
         ("rabbit 1e-70", T_HDR64, 20, 12, False, False, False),
         ("rabbit 1e-8", T_HDR32, 20, 13, False, False, True), ("rabbit 1e-30", T_HDR32, 20, 13, False, False, True),
         ("rabbit 1e-70", T_HDR64, 20, 13, False, False, True),
         ("view5", T_HDR32, 12, 12, True, True, True), ("view5", T_HDR64, 20, 12, True, True, True)]


def renderer_for(orbit, iter_bytes, waypoints):
    r = GPURenderer(0)
    assert r.orbit_form == 0
    assert r.InitializeMemory(64, 32, 1, None, 0, 0, 0, False) == 0
    assert r.set_compressed_orbit_mode(waypoints) == 0
    assert r.InitializePerturb(1, orbit, iter_bytes=iter_bytes) == 0
    assert r.orbit_form == (2 if waypoints else 1)
    return r


_inputs = {}


def case_inputs(name, T, cexp):
    """(view, SimpleCompression orbit) of a case, built once."""
    key = (name, T, cexp)
    if key not in _inputs:
        v = inputs.View.builtin(5, 192, 108) if name == "view5" else known_view(rabbit_nucleus(), name.split()[1], iterations=CAP)
        _inputs[key] = (v, inputs.Orbit(v, is64=(T == T_HDR64), compression_exp=cexp))
    return _inputs[key]


def scan_both(E, S, view, orbit, T, iter_bytes, grid, batches):
    """A whole scan with every batch evaluated by S through fs_feature_eval_resident and by E through both entries: all three
    byte for byte equal.  Returns the found points; appends each batch's (mode, records) to `batches`."""
    _, dout, _ = features.records(T == T_HDR64)

    def evaluate(mode, radius, cap, rin, rout):
        e, er, s = (np.zeros(len(rin), dout) for _ in range(3))
        assert E.FeatureEval(T, iter_bytes, mode, radius, cap, rin, e) == 0
        assert E.FeatureEvalResident(T, iter_bytes, mode, radius, cap, rin, er) == 0
        assert S.FeatureEvalResident(T, iter_bytes, mode, radius, cap, rin, s) == 0
        assert er.tobytes() == e.tobytes()
        assert s.tobytes() == e.tobytes(), "mode %d: records differ at %s" % (mode, np.nonzero(s != e)[0][:8])
        batches.append((mode, e.copy()))
        rout[:] = s

    return features.scan(view, orbit, evaluate, grid, grid, iter_bytes, CAP)


@pytest.mark.parametrize("iter_bytes", [4, 8])
@pytest.mark.parametrize("name,T,cexp,grid,sparse,diverges,finds", CASES)
def test_waypoint_scan_equals_expanded_scan(name, T, cexp, grid, sparse, diverges, finds, iter_bytes):
    v, ob = case_inputs(name, T, cexp)
    assert ob.compressed and ob.compressed_count >= 2
    if sparse:
        assert ob.compressed_count * 4 <= ob.count
    E, S = renderer_for(ob, iter_bytes, False), renderer_for(ob, iter_bytes, True)
    assert 0 < S.orbit_device_bytes < E.orbit_device_bytes
    batches = []
    found = scan_both(E, S, v, ob, T, iter_bytes, grid, batches)
    modes = [m for m, _ in batches]
    assert modes[0] == features.FIND and len(batches[0][1]) == grid * grid
    if finds:
        assert modes.count(features.FIXED) >= 2 and found  # Newton rounds and the final passes
    # the found points (strings, periods, residuals) through the library's own choice of entry
    assert features.find_periodic_points(S, v, ob, grid, grid, T, iter_bytes, CAP) == found
    if diverges:
        ok = [o[o["status"] != features.REJECTED] for _, o in batches]
        assert len(set(np.concatenate([o["period"] for o in ok]).tolist())) >= 2
        assert any((o["status"] == features.REJECTED).any() or (o["status"] == features.OK_DIRECT).any() for _, o in batches)
    E.close()
    S.close()


def test_cursor_state_crosses_slices():
    """37 steps a launch: the cursor (value, next waypoint and its index) is carried by the lane record across every launch
    boundary, never sought again.  View 5's search round: the longest period found is 122 975 (asserted: 100 launches and more
    -- it is 3 324), and the lanes have long left lockstep by then."""
    name, T, cexp, grid = CASES[6][:4]
    v, ob = case_inputs(name, T, cexp)
    E, S = renderer_for(ob, 4, False), renderer_for(ob, 4, True)
    _, dout, _ = features.records(False)
    recs = []

    def grab(mode, radius, cap, rin, rout):
        recs.append((mode, radius.copy(), cap, rin.copy()))
        rout["status"] = features.REJECTED  # ends the scan after its first round

    features.scan(v, ob, grab, grid, grid, 4, CAP)
    mode, radius, cap, rin = recs[0]
    assert mode == features.FIND
    whole, sliced = np.zeros(len(rin), dout), np.zeros(len(rin), dout)
    assert E.FeatureEval(T, 4, mode, radius, cap, rin, whole) == 0
    assert S._lib.fs_set_feature_slice(S._h, 37) == 0
    assert S.FeatureEvalResident(T, 4, mode, radius, cap, rin, sliced) == 0
    assert sliced.tobytes() == whole.tobytes()
    ok = whole["status"] == features.OK
    assert int(whole["period"][ok].max()) >= 100 * 37
    # ... and a fixed-period evaluation at a few of those periods (the Direct fallback is the same loop in both kernels)
    fixed = rin[ok][:3].copy()
    fixed["period"] = whole["period"][ok][:3]
    a, b = np.zeros(len(fixed), dout), np.zeros(len(fixed), dout)
    assert E.FeatureEval(T, 4, features.FIXED, radius, cap, fixed, a) == 0
    assert S.FeatureEvalResident(T, 4, features.FIXED, radius, cap, fixed, b) == 0
    assert b.tobytes() == a.tobytes()
    E.close()
    S.close()


def test_refusals_and_orbit_form():
    name, T, cexp = CASES[0][:3]
    v, ob = case_inputs(name, T, cexp)
    rin, rout = np.zeros(1, features.FEATURE_IN_HDR32), np.zeros(1, features.FEATURE_OUT_HDR32)
    radius = np.zeros(1, features.REAL_HDR32)
    rin64, rout64 = np.zeros(1, features.FEATURE_IN_HDR64), np.zeros(1, features.FEATURE_OUT_HDR64)
    radius64 = np.zeros(1, features.REAL_HDR64)
    for waypoints in (False, True):
        r = GPURenderer(0)
        assert r.InitializeMemory(64, 32, 1, None, 0, 0, 0, False) == 0
        assert r.orbit_form == 0
        assert r.FeatureEvalResident(T_HDR32, 4, features.FIND, radius, 16, rin, rout) == FS_ERR_6  # no orbit
        assert r.set_compressed_orbit_mode(waypoints) == 0
        assert r.InitializePerturb(1, ob) == 0
        assert r.orbit_form == (2 if waypoints else 1)
        assert r.FeatureEvalResident(T_HDR64, 4, features.FIND, radius64, 16, rin64, rout64) == FS_ERR_6  # none of this type
        for other in (0, 1, 2, 5, 6):
            assert r.FeatureEvalResident(other, 4, features.FIND, radius, 16, rin, rout) == FS_ERR_UNSUPPORTED
        assert r.FeatureEvalResident(T_HDR32, 4, 2, radius, 16, rin, rout) == FS_ERR_UNSUPPORTED  # LA mode
        assert r.FeatureEvalResident(T_HDR32, 2, features.FIND, radius, 16, rin, rout) == FS_ERR_UNSUPPORTED
        assert r.FeatureEvalResident(T_HDR32, 4, features.FIND, radius, 16, rin[:0], rout[:0]) == 0  # n = 0
        call = r._lib.fs_feature_eval_resident
        p = (radius.ctypes.data, rin.ctypes.data, rout.ctypes.data)
        for k in range(3):  # NULL radius / in / out
            q = [None if j == k else p[j] for j in range(3)]
            assert call(r._h, T_HDR32, 4, features.FIND, q[0], 16, q[1], q[2], 1) == HIP_INVALID_VALUE
        # the old entry keeps its refusal of the waypoint form
        assert r.FeatureEval(T_HDR32, 4, features.FIND, radius, 16, rin, rout) == (FS_ERR_UNSUPPORTED if waypoints else 0)
        r.close()
    # a waypoint orbit of 2^32 entries and more: 64-bit positions only.  (Three waypoints are all that is resident.)
    wp = np.zeros(3, np.dtype([("idx", "<u8"), ("mx", "<f4"), ("ex", "<i4"), ("ey", "<i4"), ("my", "<f4")]))  # fs_orbit_hdr32_rc
    assert wp.dtype.itemsize == 24
    wp["idx"] = [0, 100, (1 << 32) + 5]
    wp["mx"][1:], wp["my"][1:] = 0.75, -0.5
    low = np.zeros(2, features.REAL_HDR32)
    low["m"], low["e"] = [-1.25, 1.5], [-1, -3]
    r = GPURenderer(0)
    assert r.InitializeMemory(64, 32, 1, None, 0, 0, 0, False, iter_bytes=8) == 0
    assert r.set_compressed_orbit_mode(True) == 0
    assert r._lib.fs_upload_orbit_compressed(r._h, 0, T_HDR32, 8, wp.ctypes.data, len(wp), (1 << 32) + 50, 0,
                                             low[0:1].ctypes.data, low[1:2].ctypes.data) == 0
    assert r.orbit_form == 2
    assert r.FeatureEvalResident(T_HDR32, 4, features.FIND, radius, 16, rin, rout) == FS_ERR_UNSUPPORTED
    assert r.FeatureEvalResident(T_HDR32, 8, features.FIND, radius, 16, rin, rout) == 0  # (sixteen steps from waypoint 0 at most)
    r.close()


def test_waypoint_scan_leaves_frame_state_alone():
    v = inputs.View.builtin(5, 64, 36)
    ob = inputs.Orbit(v, compression_exp=20)
    la = inputs.LATable(ob)
    r = GPURenderer(0)
    assert r.InitializeMemory(64, 36, 1, None, 0, 0, 0, False) == 0
    assert r.set_compressed_orbit_mode(True) == 0
    assert r.InitializePerturb(1, ob, 0, None, la) == 0
    assert r.orbit_form == 2
    co = [(float(c["m"]), int(c["e"])) for c in v.coords_perturb_hdr32(ob)]

    def frame():
        assert r.RenderPerturbLAv2(None, None, None, *co, v.num_iterations, T=T_HDR32, Mode=LAV2_FULL, parity=PARITY_CPU) == 0
        out = r.new_iter_buffer()
        assert r.RenderCurrent(v.num_iterations, out, None, _capi.Reduction()) == 0
        assert r.SyncComputeStream() == 0
        return out.tobytes()

    before = frame()
    held = r.orbit_device_bytes
    assert features.find_periodic_points(r, v, ob, nx=4, ny=4, max_iters=1 << 16) is not None
    # the same generation numbers: a second InitializePerturb finds orbit and table cached and uploads nothing
    assert r.InitializePerturb(1, ob, 0, None, la) == 0
    assert r.orbit_form == 2 and r.orbit_device_bytes == held
    assert frame() == before
    r.close()
