"""CPU-only: the compare of the wide point-run kernels' period rule (csrc/exact_wide_math.hpp: block_order, less_from_masks), built
for the host with g++ (tests/exact/exact_wide_points_host.cpp, 64 lanes in a loop) and compared with Python integers: "strictly
less" between two unsigned numbers of 128 blocks, the highest differing block deciding.  Then the one refusal of
exact.eval_points(wide=True) that needs no device."""
import ctypes as C
import os
import random
import subprocess

import pytest

from fractalshark_amd import exact

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "exact", "exact_wide_points_host.cpp")
HDRS = [os.path.join(os.path.dirname(HERE), "fractalshark_amd", "csrc", f) for f in ("exact_wide_math.hpp", "exact_math.hpp")]
SO = os.path.join(HERE, "exact", "libexact_wide_points_host.so")
FULL = (1 << 64) - 1


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(SO) or max(os.path.getmtime(p) for p in [SRC] + HDRS) > os.path.getmtime(SO):
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", SO, SRC], check=True)
    h = C.CDLL(SO)
    h.exwp_less_from_masks.argtypes = [C.c_uint64] * 4
    return h


def _arr(v, n):
    assert 0 <= v < 1 << (32 * n)
    return (C.c_uint32 * n)(*[(v >> (32 * i)) & 0xFFFFFFFF for i in range(n)])


def _pairs(M, rng):
    """Pairs of unsigned numbers of 128 blocks of M limbs: the cases the rule meets, and random ones."""
    n = 128 * M
    limb = lambda i: 1 << (32 * i)
    top = limb(n - 1)
    rand = lambda: rng.getrandbits(32 * n)
    out = []
    for _ in range(6):  # equal
        v = rand()
        out.append((v, v))
    out += [(0, 0), ((1 << (32 * n)) - 1, (1 << (32 * n)) - 1)]
    for _ in range(6):  # different only in limb 0
        v = rand() & ~0xFFFFFFFF
        lo = rng.sample(range(1 << 32), 2)
        out.append((v | lo[0], v | lo[1]))
    out += [(0, 1), (1, 0)]
    for _ in range(6):  # different only in the top limb
        v = rand() % top
        hi = rng.sample(range(1 << 32), 2)
        out.append((v + hi[0] * top, v + hi[1] * top))
    out += [(top, 0), (0, top), (top | 5, top | 5)]
    # different only in the last limb of a block and the first limb of the next: the higher block decides, whatever the lower says
    for k in sorted({0, 1, 62, 63, 64, 126, rng.randrange(2, 62), rng.randrange(65, 126)}):
        last, first = k * M + M - 1, (k + 1) * M
        v = rand() & ~(0xFFFFFFFF << (32 * last)) & ~(0xFFFFFFFF << (32 * first))
        for (a_last, b_last), (a_first, b_first) in (((9, 3), (3, 9)), ((3, 9), (9, 3)), ((9, 3), (7, 7)), ((7, 7), (3, 9)),
                                                      ((0xFFFFFFFF, 0), (0, 1)), ((0, 0xFFFFFFFF), (1, 0))):
            out.append((v | a_last * limb(last) | a_first * limb(first), v | b_last * limb(last) | b_first * limb(first)))
    # one all zero above a low block, as near a nucleus
    for k in (0, 1, 5, 63, 64):
        small, small2 = rng.getrandbits(32 * M * (k + 1)), rng.getrandbits(32 * M * (k + 1))
        out += [(small, rand()), (rand(), small), (small, small2), (small, small), (small, 0), (0, small), (small, small + 1),
                (small, small | limb(M * (k + 1)))]
    out += [(rand(), rand()) for _ in range(60)]  # random
    for _ in range(30):  # random, equal above a random limb
        cut = rng.randrange(1, n)
        v = rand()
        keep = v >> (32 * cut) << (32 * cut)
        out.append((keep | rng.getrandbits(32 * cut), keep | rng.getrandbits(32 * cut)))
    return out


@pytest.mark.parametrize("M", [1, 2, 11])
def test_strictly_less_equals_python(lib, M):
    rng = random.Random(40 + M)
    n = 128 * M
    pairs = _pairs(M, rng)
    assert any(a == b for a, b in pairs) and any(a < b for a, b in pairs) and any(a > b for a, b in pairs)
    for a, b in pairs:
        for p, q in ((a, b), (b, a)):
            assert lib.exwp_below(M, _arr(p, n), _arr(q, n)) == (1 if p < q else 0), (M, hex(p)[:40], hex(q)[:40], (p > q) - (p < q))
    for a, _ in pairs[:20]:  # false on equality, whatever the value
        assert lib.exwp_below(M, _arr(a, n), _arr(a, n)) == 0


@pytest.mark.parametrize("M", [1, 2, 11])
def test_block_order_equals_python(lib, M):
    """One lane's part: 0 equal, 1 greater, 2 less, the highest differing limb of the block deciding."""
    rng = random.Random(50 + M)
    full = (1 << (32 * M)) - 1
    pairs = [(0, 0), (full, full), (0, full), (full, 0), (1, 0), (0, 1), (1 << (32 * M - 1), (1 << (32 * M - 1)) - 1)]
    pairs += [(rng.getrandbits(32 * M), rng.getrandbits(32 * M)) for _ in range(200)]
    for i in range(M):  # one limb differs, the others are equal
        v = rng.getrandbits(32 * M) & ~(0xFFFFFFFF << (32 * i))
        pairs += [(v | (5 << (32 * i)), v | (6 << (32 * i))), (v | (0x80000000 << (32 * i)), v | (0x7FFFFFFF << (32 * i)))]
    for a, b in pairs:
        assert lib.exwp_block_order(M, _arr(a, M), _arr(b, M)) == (0 if a == b else 1 if a > b else 2), (M, hex(a), hex(b))
    assert lib.exwp_block_order(12, None, None) == -1 and lib.exwp_below(0, None, None) == -1


def test_mask_decision(lib):
    """The highest differing block decides; no differing block: not less."""
    rng = random.Random(60)
    f = lib.exwp_less_from_masks
    assert f(0, 0, 0, 0) == 0
    assert f(0, 0, 1, 1) == 1 and f(0, 0, 1, 0) == 0
    assert f(1, 0, FULL, FULL) == 0 and f(1, 1, FULL, 0) == 1
    assert f(1 << 63, 1 << 63, 0, 0) == 1 and f(1 << 63, 0, 0, 0) == 0
    assert f(3, 1, 0, 0) == 0 and f(3, 2, 0, 0) == 1
    for _ in range(2000):
        ne = rng.getrandbits(128) & rng.getrandbits(128) & (rng.getrandbits(128) if rng.random() < 0.5 else (1 << 128) - 1)
        lt = rng.getrandbits(128) & ne
        want = 0 if ne == 0 else (lt >> (ne.bit_length() - 1)) & 1
        assert f(ne >> 64, lt >> 64, ne & FULL, lt & FULL) == want, (hex(ne), hex(lt))


def test_eval_points_wide_refuses_beyond_704_limbs():
    """No device is reached: frac_bits 22 519 needs 705 limbs."""
    assert exact.MAX_WIDE_FRAC_BITS == 22518 and exact.limbs_for(22519) == 705
    with pytest.raises(ValueError):
        exact.eval_points(None, [0], [0], [1], 22519, wide=True)
    with pytest.raises(ValueError):  # (the default is what it was)
        exact.eval_points(None, [0], [0], [1], exact.MAX_FRAC_BITS + 1)
