#!/usr/bin/env python3
"""Every product of the host input builders (fractalshark_amd/host/, C ABI include/fs_inputs.h) as `name  byte_count  fnv1a64`
lines, for built-in views 0 (shallow), 5 (the headline one), 14 (the deepest) and 17 (a long period) at 64 x 36.

    tools/dump_host_inputs.py                     this tree's host/*.cpp
    tools/dump_host_inputs.py --tree DIR          the host/*.cpp of another checkout (say the parent commit's)
    tools/dump_host_inputs.py --sanitize          built with AddressSanitizer + UndefinedBehaviorSanitizer at -O1

Two trees build the same inputs exactly when their outputs are equal line for line (`diff`); with -ffp-contract=off the
sanitized build must print the same lines too.  tests/host_inputs/inputs_dump.cpp (always this tree's: it uses the C ABI alone)
is compiled with plain g++ together with the host units into build/host_inputs_dump/ and run as a child process per view; the
library is never loaded into Python.
"""
import argparse
import glob
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GMP_PREFIX = os.environ.get("FS_GMP_PREFIX", "/opt/conda")
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fPIC"]  # fractalshark_amd/_build.py _INPUTS_FLAGS
SANITIZE_FLAGS = ["-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fPIC", "-fsanitize=address,undefined",
                  "-fno-sanitize-recover=undefined"]
WIDTH, HEIGHT = 64, 36
# view -> (iteration cap, long-orbit cap).  View 14 works at 21 829 bits: at the cap of 50 000 that the other views get, its
# orbits alone take a minute, so its cap is 5 000.  The long orbit (HDRFloat<float>, no periodicity) is what reaches the
# multi-threaded stage-0 scan of the LAv2 builder, which starts at 100 000 orbit entries (2 chunks on view 5, 8 on view 17).
VIEWS = {0: (50000, 0), 5: (50000, 150000), 14: (5000, 0), 17: (50000, 450000)}


def build(tree=ROOT, sanitize=False, out_dir=None):
    """Compiles inputs_dump.cpp + <tree>/fractalshark_amd/host/*.cpp (into build/host_inputs_dump/<kind>/ unless out_dir says
    otherwise), returns the program's path."""
    flags = SANITIZE_FLAGS if sanitize else FLAGS
    kind = ("san" if sanitize else "plain") + ("" if os.path.samefile(tree, ROOT) else "_other")
    out_dir = out_dir or os.path.join(ROOT, "build", "host_inputs_dump", kind)
    os.makedirs(out_dir, exist_ok=True)
    units = sorted(glob.glob(os.path.join(tree, "fractalshark_amd", "host", "*.cpp")))
    if not units:
        raise SystemExit("no host/*.cpp under %s" % tree)
    units.append(os.path.join(ROOT, "tests", "host_inputs", "inputs_dump.cpp"))

    def one(src):
        obj = os.path.join(out_dir, os.path.basename(src) + ".o")
        subprocess.run(["g++", *flags, "-I" + os.path.join(GMP_PREFIX, "include"), "-c", src, "-o", obj], check=True)
        return obj

    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        objs = list(ex.map(one, units))
    exe = os.path.join(out_dir, "inputs_dump")
    # (libstdc++ is linked statically: the GMP prefix may carry an older one, which its -L and rpath would put first)
    link = ["-static-libstdc++"] + (["-fsanitize=address,undefined"] if sanitize else [])
    subprocess.run(["g++", *link, "-o", exe, *objs, "-L" + os.path.join(GMP_PREFIX, "lib"), "-lgmp",
                    "-Wl,-rpath," + os.path.join(GMP_PREFIX, "lib")], check=True)
    return exe


def run(exe, view, cap, long_cap=0, width=WIDTH, height=HEIGHT):
    """The program's lines for one built-in view (a child process; a sanitizer report or a crash raises)."""
    with open(os.path.join(ROOT, "fractalshark_amd", "data", "views.json")) as f:
        v = json.load(f)[str(view)]
    cmd = [exe, v["minX"], v["minY"], v["maxX"], v["maxY"], str(width), str(height), str(cap)]
    if long_cap:
        cmd.append(str(long_cap))
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, check=True)
    return ["view%d.%s" % (view, line) for line in p.stdout.splitlines()]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tree", default=ROOT, help="checkout whose fractalshark_amd/host/*.cpp are built (default: this one)")
    ap.add_argument("--sanitize", action="store_true", help="-O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined")
    args = ap.parse_args()
    exe = build(os.path.abspath(args.tree), args.sanitize)
    for view, (cap, long_cap) in VIEWS.items():
        print("\n".join(run(exe, view, cap, long_cap)))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
