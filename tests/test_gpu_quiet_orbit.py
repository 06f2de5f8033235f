"""What an orbit's upload leaves on the device for the tuned loops -- the prepared orbit, the two companions, zs2 / zqb of the 16-step body,
the NDZ bounds znz with their slack (k_prepare_orbit_hdr32, k_make_quiet_orbit, in csrc/kernels_orbit_prep.hip; k_decompress_orbit_hdr32 in csrc/kernels_decompress.hip), the
HDRFloat<double> prepared orbit and the scaled kernels' bound word (k_scaled_bounds) -- read back (fs_read_quiet_orbit) and held BIT FOR
BIT against the plain model tests/_quiet_model.py, which tests/test_quiet_model_cpu.py holds against what the bounds are for.  Compared
as uint32 patterns, so "never" (-0.0) and +inf are patterns like any other.  On every orbit of tests/_quiet_orbits.py:

  1. every array equals the model's, slack included; the first differing entry and field is reported;
  2. the structural identities on the device's arrays alone: zs2 == the second companion's .xy, zqb[i] == its .w at i + 3, i + 7, i + 11,
     i + 15 ("never" past the end), the first companion's .xy == the prepared orbit's;
  3. the counts of entries with an own bound, a block bound and NDZ bounds equal tests/golden/quiet_orbit_counts.json;
  4. a compressed orbit (compression_exp = 20): what the decompress kernel writes, .w included, is the model's prepared orbit of the
     host-expanded entries, and the companions follow from it;
  5. HDRFloat<double> (View 5): zref64 equals the model;
  6. the scaled kernels' bound words after fs_upload_orbit_scaled (the upload RenderPerturbBLAScaled does): View 5, View 5 with `bad` flags
     and edge values, View 14 (`bad` entries of its own).

No frame is rendered: every test is an upload and a copy."""
import json

import numpy as np
import pytest

import _quiet_model as qm
import _quiet_orbits as qo
from fractalshark_amd import GPURenderer, T_HDR32, inputs

pytestmark = pytest.mark.gpu

FIELDS = {"prepared": ("re", "im", "e", "w"), "first": ("re", "im", "s", "w"), "second": ("2Z.re", "2Z.im", "own bound", "block bound"),
          "zs2": ("2Z.re", "2Z.im"), "zqb": ("block bound of i + 3", "of i + 7", "of i + 11", "of i + 15"),
          "znz": ("bound on max|dz|", "bound on max|dc|")}


@pytest.fixture(scope="module")
def renderer(native_libs):
    assert GPURenderer.TestCudaIsWorking() != 0, "no usable HIP device: the product path has no CPU fallback"
    r = GPURenderer(0)
    assert r.InitializeMemory(64, 36, 1, None, 0, 0, 0, False) == 0
    yield r
    r.close()


def _assert_equal(what, name, got, want):
    """bit equality of two float32 arrays, a row per entry; the first differing entry and field in the message"""
    assert got.shape == want.shape, (what, name, got.shape, want.shape)
    g, w = qm.bits(got).reshape(got.shape), qm.bits(want).reshape(want.shape)
    if not np.array_equal(g, w):
        i, c = (int(x[0]) for x in np.nonzero(g != w))
        raise AssertionError("%s of %s: entry %d of %d, field %d (%s): device 0x%08x, model 0x%08x; %d words differ"
                             % (what, name, i, got.shape[0], c, FIELDS[what][c], int(g[i, c]), int(w[i, c]), int((g != w).sum())))


def _check_companions(name, got, prep):
    """everything derived from the prepared orbit `prep` against the model, then the identities on the device's arrays alone"""
    want = qm.Tables(prep).parts()
    for what in ("prepared", "first", "second", "zs2", "zqb", "znz"):
        _assert_equal(what, name, got[what], want[what])
    n = got["prepared"].shape[0]
    assert np.array_equal(qm.bits(got["zs2"][:n]), qm.bits(got["second"][:, :2]))
    blk = np.concatenate([qm.bits(got["second"][:, 3]), np.full(16, qm.NEVER, np.uint32)])
    for c, off in enumerate((3, 7, 11, 15)):
        assert np.array_equal(qm.bits(got["zqb"][:n, c]), blk[np.arange(n) + off]), (name, c)
    assert np.array_equal(qm.bits(got["first"][:, :2]), qm.bits(got["prepared"][:, :2]))


@pytest.mark.parametrize("name", qo.ALL)
def test_read_back_equals_the_model(renderer, native_libs, name):
    ob = qo.orbit(name)
    assert renderer.InitializePerturb(0, ob, 0, None, None) == 0
    got = renderer.read_quiet_orbit()
    assert got["prepared"].shape == (ob.count + 2, 4) and got["zqb"].shape == (ob.count + 2 + qm.SLACK, 4)
    _check_companions(name, got, qm.prepared(ob.entries()))
    golden = json.load(open(qo.GOLDEN))["orbits"][name]
    assert dict(entries=ob.count + 2, **qm.counts(got)) == golden, (name, qm.counts(got), golden)


@pytest.mark.parametrize("name", ["view5_64x36", "view3_64x36"])
def test_decompressed_orbit_equals_the_model_of_the_expanded_one(renderer, native_libs, name):
    ob = inputs.Orbit(qo.orbit(name).view, compression_exp=20)
    assert ob.compressed and 0 < ob.compressed_count < ob.count
    assert renderer.InitializePerturb(0, ob, 0, None, None) == 0
    got = renderer.read_quiet_orbit()
    assert got["prepared"].shape == (ob.count + 2, 4)
    _check_companions(name + " compressed", got, qm.prepared(ob.entries()))
    assert min(qm.counts(got).values()) > 0


def test_hdr64_prepared_orbit_equals_the_model(renderer, native_libs):
    ob = inputs.Orbit(qo.orbit("view5_64x36").view, is64=True)
    assert renderer.InitializePerturb(0, ob, 0, None, None) == 0
    got, want = renderer.read_prepared_orbit64(), qm.prepared64(ob.entries())
    assert got.dtype == want.dtype and got.shape == want.shape == (ob.count + 2,)
    for f in ("re", "im", "e", "pad", "w"):
        g, w = (np.ascontiguousarray(a[f]).view(np.uint64 if a[f].dtype.itemsize == 8 else np.uint32) for a in (got, want))
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, "zref64: entry %d of %d, field %s: device 0x%x, model 0x%x; %d differ" % (
            int(bad[0]), got.shape[0], f, int(g[bad[0]]), int(w[bad[0]]), bad.size)
    # (the HDRFloat<float> tables are not this orbit's: their read-back refuses)
    with pytest.raises(RuntimeError):
        renderer.read_quiet_orbit()


@pytest.mark.parametrize("name", qo.SCALED)
def test_scaled_bound_words_equal_the_model(renderer, native_libs, name):
    t, f = qo.scaled_pair(name)
    assert renderer._lib.fs_upload_orbit_scaled(renderer._h, T_HDR32, 4, t.ctypes.data, f.ctypes.data, len(f), 0) == 0
    got = renderer.read_scaled_orbit()
    assert got.shape == f.shape
    for c in ("bad", "x", "y"):   # the entries themselves are as uploaded
        assert got[c].tobytes() == f[c].tobytes(), (name, c)
    want = qm.scaled_words(f)
    bad = np.nonzero(got["padding"] != want)[0]
    assert bad.size == 0, "scaled bound word of %s: entry %d of %d (bad %d, x %r, y %r): device 0x%08x, model 0x%08x; %d differ" % (
        name, int(bad[0]), len(f), int(f["bad"][bad[0]]), float(f["x"][bad[0]]), float(f["y"][bad[0]]), int(got["padding"][bad[0]]),
        int(want[bad[0]]), bad.size)
    never = want == qm.bits(np.array([-1.0], np.float32))[0]
    assert 0 < int(never.sum()) < len(f)
