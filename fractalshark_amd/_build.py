"""Build recipes for the native libraries (in-tree, so the .so files travel to the GPU box).

  csrc/libfsmi355.so   hipcc --offload-arch=gfx950: HIP kernels + the C ABI of include/fsmi355.h  (the product)
  host/libfsinputs.so  g++ + GMP: host-side input builders of include/fs_inputs.h (view / orbit / LA / BLA), every host/*.cpp

`-ffp-contract=off` is part of the numerical contract (see csrc/hdr_math.hpp): the parity target is the
reference's CPU build, which has no FMA.

Up-to-date checks compare a CONTENT hash of the sources + flags with a stamp written next to each output (file
times do not survive the snapshot that carries the tree to the GPU box; a stale time there would start a compiler
under a profiler).  Translation units are compiled to objects in parallel and only the changed ones are rebuilt.
"""
import glob
import hashlib
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
HOST = os.path.join(HERE, "host")
OBJ = os.path.join(CSRC, "build")
LIB_RENDER = os.path.join(CSRC, "libfsmi355.so")
LIB_INPUTS = os.path.join(HOST, "libfsinputs.so")

GMP_PREFIX = os.environ.get("FS_GMP_PREFIX", "/opt/conda")


def _run(cmd):
    # compilers never inherit a profiler's preload (rocprofv3 injects a library that initialises the GPU; exec'ing
    # clang / cc1plus / ld from such a process tree is what the GPU pool forbids)
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD" and not k.startswith(("ROCP_", "ROCPROF"))}
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    if p.returncode != 0:
        raise RuntimeError("build failed: %s\n%s" % (" ".join(cmd), p.stdout))
    return p.stdout


def _digest(paths, flags):
    h = hashlib.sha256()
    h.update("\0".join(flags).encode())
    for p in sorted(paths):
        h.update(os.path.basename(p).encode() + b"\0")
        with open(p, "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def _stamp_ok(target, digest):
    try:
        return os.path.exists(target) and open(target + ".stamp").read().strip() == digest
    except OSError:
        return False


def _write_stamp(target, digest):
    with open(target + ".stamp", "w") as f:
        f.write(digest + "\n")


def _render_units():
    """Translation units of libfsmi355.so: every csrc/*.hip plus the host side of the C ABI, every csrc/*.cpp."""
    return sorted(glob.glob(os.path.join(CSRC, "*.hip"))) + sorted(glob.glob(os.path.join(CSRC, "*.cpp")))


def _render_headers():
    return sorted(glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.hpp")) +
                  [os.path.join(ROOT, "include", f) for f in ("fsmi355.h", "fsmi355_internal.h", "fs_layout.h")])


# Build-time switches of the probe and verification builds that tools/ make (environment variable = 1 -> -D<name>); never set
# for the product build
_PROBE_SWITCHES = (
    "FS_PROFILE_CYCLES",      # the instrumented (step-counting) kernel variants also report shader-clock cycles per phase (tools/cycle_probe.py)
    "FS_VERIFY_BLOCK_BOUND",  # tools/block_bound_check.py: the untested loop off, violations counted
    "FS_TRACE_WAVES",         # tools/wave_trace.py: per-wave start / end / SIMD records
    "FS_VERIFY_FLOOR",        # tools/floor_check.py: the every-second-state floor form, trips whose untested first state is below the every-state floor counted
    "FS_BLA_FAST_PROBE",      # tools/bla_fast_check.py: how often the hand-written BLA loop is left (statistics words 20..23)
    "FS_2X32_PROBE",          # counts the 2x32 perturbation loop's literal steps (statistics word 12)
)


def _render_flags(env=None):
    env = os.environ if env is None else env
    extra = ["-D" + name for name in _PROBE_SWITCHES if env.get(name) == "1"]
    return ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", *extra]


# Per-unit flags.  kernels_scaled.hip: the scalar float expressions of the reference's scaled kernel are written out
# operation by operation; the SLP vectorizer pairs them into packed instructions with register shuffles around them, which
# costs more than the two-operand scalar forms it replaces (the pairs that pay are written as float2 in the source).
_UNIT_FLAGS = {"kernels_scaled.hip": ["-fno-slp-vectorize"]}


def _unit_flags(src):
    return _UNIT_FLAGS.get(os.path.basename(src), [])


def _unit_digest(src, hdr_digest, extra=()):
    return _digest([src], [hdr_digest, *_unit_flags(src), *extra])


def _hip_lang(src):
    # csrc/*.cpp (renderer*.cpp, group.cpp) are host-only C++ that include HIP runtime headers: compiled by hipcc as HIP so
    # that <hip/hip_runtime.h> types (float4, hipStream_t) match the kernels' launchers
    return [] if src.endswith(".hip") else ["-x", "hip"]


def _hipcc():
    return shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _compile_all(jobs, force=False, cc=None, lang=_hip_lang):
    """jobs: (src, obj, flags, digest) -- each object is compiled (by cc, default hipcc; lang(src) = its language options) unless
    its stamp already matches its digest."""
    cc = cc or _hipcc()

    def one(job):
        src, obj, flags, d = job
        if force or not _stamp_ok(obj, d):
            _run([cc, *flags, *_unit_flags(src), "-c", *lang(src), src, "-o", obj])
            _write_stamp(obj, d)
        return obj

    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        return list(ex.map(one, jobs))


def _link(lib, objs):
    # RCCL (the multi-GPU gather behind fs_group_*) is resolved at run time with dlopen, so the library loads on hosts
    # without it; -ldl only
    _run([_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib, *objs, "-ldl", "-lpthread"])


def _inputs_units():
    """Translation units of libfsinputs.so: every host/*.cpp (they share host/inputs_state.hpp)."""
    return sorted(glob.glob(os.path.join(HOST, "*.cpp")))


def _inputs_headers():
    return sorted(glob.glob(os.path.join(HOST, "*.hpp"))) + [
        os.path.join(CSRC, "hdr_math.hpp"), os.path.join(CSRC, "la_math.hpp"), os.path.join(CSRC, "df32_math.hpp"),
        os.path.join(CSRC, "bla_math.hpp"), os.path.join(ROOT, "include", "fs_inputs.h"), os.path.join(ROOT, "include", "fs_layout.h")]


def _inputs_sources():
    return _inputs_units() + _inputs_headers()


_INPUTS_FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fPIC"]


def _render_digest(units, headers, flags):
    return _digest(units + headers, flags + [repr(sorted(_UNIT_FLAGS.items()))])


def up_to_date():
    """True when both libraries exist and were built from the current sources (no compiler is started)."""
    units = [u for u in _render_units() if os.path.exists(u)]
    return (_stamp_ok(LIB_RENDER, _render_digest(units, _render_headers(), _render_flags())) and
            _stamp_ok(LIB_INPUTS, _digest(_inputs_sources(), _INPUTS_FLAGS)))


def build_render(force=False):
    units = [u for u in _render_units() if os.path.exists(u)]
    headers = _render_headers()
    flags = _render_flags()
    digest = _render_digest(units, headers, flags)
    if not force and _stamp_ok(LIB_RENDER, digest):
        return LIB_RENDER
    os.makedirs(OBJ, exist_ok=True)
    hdr_digest = _digest(headers, flags)
    jobs = [(src, os.path.join(OBJ, os.path.basename(src) + ".o"), flags, _unit_digest(src, hdr_digest)) for src in units]
    _link(LIB_RENDER, _compile_all(jobs, force))
    _write_stamp(LIB_RENDER, digest)
    return LIB_RENDER


def build_variant(name, units, defs):
    """build/ab/libfsmi355_<name>.so: the product with the translation units named in `units` (base names) compiled with the extra
    flags `defs` (and the probe switches of the environment); select it at run time with FSMI355_LIB.  Writes under build/ab/ only:
    the other units come from the product's objects where their stamps say they were built from the current sources with the
    product's flags, else they are compiled into build/ab/<name>/.  Returns the path."""
    out_dir = os.path.join(ROOT, "build", "ab", name)
    os.makedirs(out_dir, exist_ok=True)
    headers = _render_headers()
    flags, product_flags = _render_flags(), _render_flags({})
    hdr_digest, product_hdr_digest = _digest(headers, flags), _digest(headers, product_flags)
    jobs = []
    for src in _render_units():
        base = os.path.basename(src)
        if base in units:
            jobs.append((src, os.path.join(out_dir, base + ".o"), [*flags, *defs], _unit_digest(src, hdr_digest, defs)))
            continue
        d = _unit_digest(src, product_hdr_digest)
        obj = os.path.join(OBJ, base + ".o")
        if not _stamp_ok(obj, d):
            obj = os.path.join(out_dir, base + ".o")
        jobs.append((src, obj, product_flags, d))
    lib = os.path.join(ROOT, "build", "ab", "libfsmi355_%s.so" % name)
    _link(lib, _compile_all(jobs))
    return lib


def build_inputs(force=False):
    srcs = _inputs_sources()
    digest = _digest(srcs, _INPUTS_FLAGS)
    if not force and _stamp_ok(LIB_INPUTS, digest):
        return LIB_INPUTS
    obj_dir = os.path.join(HOST, "build")
    os.makedirs(obj_dir, exist_ok=True)
    flags = [*_INPUTS_FLAGS, "-I" + os.path.join(GMP_PREFIX, "include")]
    hdr_digest = _digest(_inputs_headers(), flags)
    jobs = [(src, os.path.join(obj_dir, os.path.basename(src) + ".o"), flags, _unit_digest(src, hdr_digest))
            for src in _inputs_units()]
    objs = _compile_all(jobs, force, cc="g++", lang=lambda src: [])
    _run(["g++", "-shared", "-fPIC", "-o", LIB_INPUTS, *objs, "-L" + os.path.join(GMP_PREFIX, "lib"), "-lgmp",
          "-Wl,-rpath," + os.path.join(GMP_PREFIX, "lib")])
    _write_stamp(LIB_INPUTS, digest)
    return LIB_INPUTS


def build_all(force=False):
    return build_render(force), build_inputs(force)


def status2_test_variant():
    """build/ab/libfsmi355_h64st2.so: the library with k_lav2_hdr64's hand-written statements taking their rarest exit (status 2) on
    EVERY step (-DFS_H64_ASM_TINY=1e300) -- what tests/test_gpu_hdr64_statement_exits.py renders with.  Built (build_variant) when its
    content stamp does not match the sources; returns the path."""
    defs = ["-DFS_H64_ASM_TINY=1e300"]
    lib = os.path.join(ROOT, "build", "ab", "libfsmi355_h64st2.so")
    # (by content, as the product's own stamp: file times mean nothing on a freshly copied tree)
    digest = _digest(_render_units() + _render_headers(), _render_flags() + defs)
    if not _stamp_ok(lib, digest):
        build_variant("h64st2", ["kernels_hdr64.hip"], defs)
        _write_stamp(lib, digest)
    return lib


if __name__ == "__main__":
    print(build_all(force=True))
