"""Building and running the two small programs of tests/arith, and comparing their result words with the model's."""
import math
import os
import subprocess
import sys

import _arith_cases as C
import _ieee_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
ARITH = os.path.join(HERE, "arith")


def build_host(out_dir, extra=()):
    """arith_host, with the product's host-input flags (taken from the build recipe, not retyped)"""
    from fractalshark_amd import _build
    exe = os.path.join(str(out_dir), "arith_host")
    cmd = ["g++", *_build._INPUTS_FLAGS, *extra, "-o", exe, os.path.join(ARITH, "arith_host.cpp")]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    return exe


def run_host(exe, out_dir, cases):
    cf, of = os.path.join(str(out_dir), "cases.bin"), os.path.join(str(out_dir), "host_out.bin")
    C.write_case_file(cf, cases)
    p = subprocess.run([exe, cf, of], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    return C.read_out_file(of, len(cases))


def build_device(out_dir):
    """arith_device, with exactly the product's render flags: a product translation unit that loses -ffp-contract=off or gains a
    fast-math switch through _render_flags() takes this program with it"""
    from fractalshark_amd import _build
    exe = os.path.join(str(out_dir), "arith_device")
    _build._run([_build._hipcc(), *_build._render_flags(), "-o", exe, os.path.join(ARITH, "arith_device.hip")])
    return exe


def _is_nan_word(t, words, k):
    """is the float that word k of a result of type t belongs to a NaN?"""
    flat = []

    def walk(t):
        if t in "ib":
            flat.append(None)
        elif t == "f":
            flat.append(("f", len(flat)))
        elif t == "d":
            flat.extend((("d", len(flat)), ("d", len(flat))))
        elif t == "D":
            walk("f"), walk("f")
        elif t[0] == "h":
            walk(t[1]), walk("i")
        elif t[0] == "c":
            walk(t[1]), walk(t[1]), walk("i")
        elif t[0] == "q":
            [walk(t[1]) for _ in range(4)]
        elif t[0] == "p":
            walk(t[1]), walk(t[1])
        elif t == "A":
            walk("hD"), walk("hD"), walk("b")
    walk(t)
    if flat[k] is None:
        return False
    kind, first = flat[k]
    if kind == "f":
        return math.isnan(M.F32.from_bits(words[first]))
    return math.isnan(M.F64.from_bits(words[first] | (words[first + 1] << 32)))


def words_equal(case, got, want):
    """every result word equal (-0 is not +0); a NaN equals any NaN"""
    n = case.op.words_out
    for k in range(n):
        if got[k] != want[k] and not (_is_nan_word(case.op.out, got, k) and _is_nan_word(case.op.out, want, k)):
            return False
    return True


def describe(case, got, host_words=None):
    hx = lambda w: " ".join("%08x" % x for x in w)
    s = "%s [class %s] operands %s | model %s | got %s" % (case.op.name, case.cls, hx(case.in_words[:case.op.words_in]),
                                                          hx(case.out_words), hx(got[:case.op.words_out]))
    if host_words is not None:
        s += " | host %s" % hx(host_words[:case.op.words_out])
    return s
