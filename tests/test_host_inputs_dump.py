"""CPU-only: tests/host_inputs/inputs_dump.cpp -- the stand-alone program that prints one `name  byte_count  fnv1a64` line per
product of the host input builders (tools/dump_host_inputs.py compares two builds of fractalshark_amd/host/ with it) -- still
compiles against the C ABI of include/fs_inputs.h together with host/*.cpp, prints every product, and prints the same twice.

No hash value is pinned here: whether another machine's libm gives the same last bit everywhere is not known.  The names are:
tests/golden/host_inputs_dump_view0_names.txt holds those of view 0 at 64 x 36 with the iteration cap 2 000 (an empty product
prints no line; regenerate the file from the program's output when a product is added to it)."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _wrapper():
    spec = importlib.util.spec_from_file_location("dump_host_inputs", os.path.join(ROOT, "tools", "dump_host_inputs.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_covers_every_product_and_repeats(tmp_path):
    dump = _wrapper()
    exe = dump.build(out_dir=str(tmp_path))  # no sanitizers
    first = dump.run(exe, 0, 2000)
    with open(os.path.join(ROOT, "tests", "golden", "host_inputs_dump_view0_names.txt")) as f:
        expected = ["view0." + line.strip() for line in f if line.strip()]
    fields = [line.split() for line in first]
    assert all(len(f) == 3 for f in fields), [line for line, f in zip(first, fields) if len(f) != 3]
    names = [f[0] for f in fields]
    assert len(set(names)) == len(names), "a product name is printed twice"
    assert set(names) == set(expected), (sorted(set(expected) - set(names)), sorted(set(names) - set(expected)))
    for name, byte_count, digest in fields:
        assert int(byte_count) > 0, name
        assert len(digest) == 16 and int(digest, 16) >= 0, name
    assert dump.run(exe, 0, 2000) == first
