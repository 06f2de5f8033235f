#!/usr/bin/env python3
"""Build an A/B variant of libfsmi355.so: the named translation units recompiled with extra -D flags, linked with the product's
other objects, into build/ab/libfsmi355_<name>.so (git-ignored, but it travels to the GPU box with the snapshot).  The product
library and its objects are never rebuilt (fractalshark_amd/_build.py: build_variant).  Select it at run time with
FSMI355_LIB=build/ab/libfsmi355_<name>.so (fractalshark_amd/_capi.py prints the path it loads).

  python tools/build_variant.py <name> <unit.hip>[,<unit2.hip>] -DFOO=1 [-DBAR ...]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fractalshark_amd import _build  # noqa: E402


def main():
    name, units, defs = sys.argv[1], sys.argv[2].split(","), sys.argv[3:]
    print(_build.build_variant(name, units, defs))


if __name__ == "__main__":
    main()
