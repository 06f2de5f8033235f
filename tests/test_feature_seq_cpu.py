"""CPU-only: what fs_feature_eval_resident adds to the C ABI, the cursor header on its own, and the compiled kernels' resources --
moving the waypoint cursor into csrc/seq_orbit.hpp and the step loop into a shared body left the kernels that had them as the
compiler made them before (tests/golden/feature_seq_parent_resources.json, read off the parent commit's library with
tools/kernel_resources.py), and the new kernels need no scratch."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import pytest

from fractalshark_amd import _build, _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "feature_seq_parent_resources.json")


def test_capi_declares_the_new_entries(native_libs):
    lib = _capi.render_lib()
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    ev = lib.fs_feature_eval_resident
    assert ev.restype is u32 and list(ev.argtypes) == [vp, C.c_int, u32, C.c_int, vp, u64, vp, vp, u64]
    assert list(ev.argtypes) == list(lib.fs_feature_eval.argtypes)  # the records and arguments of fs_feature_eval
    assert lib.fs_orbit_form.restype is C.c_int and list(lib.fs_orbit_form.argtypes) == [vp]
    assert {"fs_feature_eval_resident", "fs_orbit_form"} <= set(_capi.RENDER_SYMBOLS)
    public = open(os.path.join(ROOT, "include", "fsmi355.h")).read()
    assert re.search(r"uint32_t fs_feature_eval_resident\(fs_renderer \*r, int type_tag, uint32_t iter_bytes, int mode, "
                     r"const void \*radius,\s+uint64_t max_iters, const void \*in, void \*out, uint64_t n\);", public)
    assert "int fs_orbit_form(const fs_renderer *r);" in public


def test_cursor_header_is_hashed_and_builds_alone(tmp_path):
    """csrc/seq_orbit.hpp is one of the headers the build's stamps hash, there is one text of the cursor, and the header and
    kernels.h each compile as the first include of a translation unit (device pass, gfx950)."""
    hdr = os.path.join(_build.CSRC, "seq_orbit.hpp")
    assert hdr in _build._render_headers()
    texts = {os.path.basename(p): open(p).read() for p in _build._render_units() + _build._render_headers()}
    assert [n for n, t in texts.items() if "struct SeqOrbit" in t] == ["seq_orbit.hpp"]
    for first in ("seq_orbit.hpp", "kernels.h"):
        src = tmp_path / ("alone_%s.hip" % first.split(".")[0])
        src.write_text('#include "%s"\n#include "seq_orbit.hpp"\n'
                       "__global__ void k(const fs_orbit_hdr32_rc *wp, fs::hcplx<float> *out)\n"
                       "{\n    fs::SeqOrbit<float, uint64_t> s;\n    s.wp = wp, s.n_wp = 2u;\n    s.cx = s.cy = fs::hr_zero<float>();\n"
                       "    s.rewind();\n    s.step();\n    out[0] = s.value();\n}\n" % first)
        _build._run([_build._hipcc(), *_build._render_flags(), "--cuda-device-only", "-fsyntax-only", "-I" + _build.CSRC,
                     str(src)])


@pytest.fixture(scope="module")
def resources(native_libs):
    """{mangled kernel name: {vgpr, sgpr, scratch, lds}} of the built library (tools/kernel_resources.py --json)."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "--json"],
                         stdout=subprocess.PIPE, text=True, check=True).stdout
    table = json.loads(out)
    assert len(table) > 100
    return table


def test_moved_code_compiles_as_before(resources):
    """k_feature_step (four instantiations), the waypoint-resident instantiations of k_lav2_lit (kSeq, eighteen) and the cursor
    probe (four): VGPRs, SGPRs, scratch and LDS as on the parent commit."""
    parent = json.load(open(GOLDEN))["kernels"]
    assert sum("k_feature_stepI" in k for k in parent) == 4
    assert sum("k_lav2_litI" in k for k in parent) == 18 and sum("k_seq_cursor_probeI" in k for k in parent) == 4
    # (the golden file's keys are the names' first 90 characters, which tell these kernels apart)
    mine = {k[:90]: v for k, v in resources.items() if "k_feature_stepI" in k or "k_seq_cursor_probeI" in k or
            re.search(r"k_lav2_litI\w+Lb1EEv", k)}
    assert sorted(mine) == sorted(parent)  # these are all there are of them
    for name, want in parent.items():
        assert mine[name] == want, (name, mine[name], want)


def test_new_kernels_use_no_scratch(resources):
    step = [k for k in resources if "k_feature_step_seqI" in k]
    init = [k for k in resources if "k_feature_initI" in k and "FsFeatSeqLane" in k]
    assert len(step) == 4 and len(init) == 4  # HDRFloat<float | double> x 32- / 64-bit positions
    for k in step + init:
        assert resources[k]["scratch"] == 0 and resources[k]["lds"] == 0, (k, resources[k])
