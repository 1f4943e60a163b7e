"""The G1 endomorphism chain of the RLC scalars (csrc/bls_g1_endo.h) on the CPU: a host build of the header with
the digit form's column, value and subtraction checks compiled in (tests/hostcheck_endo), against the Python oracle.

The batch reads its 64 random bits as r = a + b lambda mod r (a the low, b the high 32 bits, lambda = -x^2 mod r
the eigenvalue of phi(x, y) = (beta x, y) on G1), so g1q_mul_endo(A, a, b) must equal [(a + b lambda) mod r] A.
"""
import ctypes
import os
import random
import subprocess

from oracle import bls_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "hostcheck_endo")
LIB = os.path.join(DIR, "libhostcheck_endo.so")
INC = os.path.join(os.path.dirname(HERE), "eth-consensus-specs_amd", "csrc")

LAMBDA = (-O.X * O.X) % O.R
M32 = 2 ** 32 - 1
CORNERS = [(1, 0), (0, 1), (1, 1), (0, 0), (M32, 0), (0, M32), (M32, M32), (2 ** 31, 2 ** 31)]

_lib = None


def lib():
    global _lib
    if _lib is None:
        deps = [os.path.join(DIR, f) for f in ("hostcheck_endo.cpp", "Makefile")]
        deps += [os.path.join(INC, f) for f in os.listdir(INC) if f.endswith(".h")]
        if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(d) for d in deps):
            subprocess.check_call(["make", "-C", DIR], timeout=2400)
        _lib = ctypes.CDLL(LIB)
        _lib.hc_endo_mul.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_char_p]
        _lib.hc_endo_beta.argtypes = [ctypes.c_char_p]
    return _lib


def fp_b(v):
    return (v % O.P).to_bytes(48, "big")


def endo_mul(proj, a, b):
    """g1q_mul_endo on the projective point (X, Y, Z); the affine result, or None for the identity"""
    out = ctypes.create_string_buffer(96)
    lib().hc_endo_mul(b"".join(fp_b(c) for c in proj), a, b, out)
    if out.raw == bytes(96):
        return None
    return (int.from_bytes(out.raw[:48], "big"), int.from_bytes(out.raw[48:], "big"))


def beta():
    out = ctypes.create_string_buffer(48)
    lib().hc_endo_beta(out)
    return int.from_bytes(out.raw, "big")


def test_phi_is_lambda():
    """phi(G) = (beta G.x, G.y) == [lambda] G for the library's FP_BETA, beta a primitive cube root of one"""
    b = beta()
    assert b != 1 and pow(b, 3, O.P) == 1
    assert (LAMBDA * LAMBDA + LAMBDA + 1) % O.R == 0
    gx, gy = O.G1_GEN
    assert (b * gx % O.P, gy) == O.g1_mul(O.G1_GEN, LAMBDA)


def test_mul_endo_matches_oracle():
    """g1q_mul_endo(A, a, b) == [(a + b lambda) mod r] A: the generator, a random multiple, a point given with
    Z != 1 and the identity, on the corner pairs and seeded random pairs"""
    rng = random.Random(0xE1D0)
    pairs = CORNERS + [(rng.getrandbits(32), rng.getrandbits(32)) for _ in range(40)]
    # sparse pairs: long runs of zero digits, and digits of one kind only
    pairs += [(1 << rng.randrange(32), 1 << rng.randrange(32)) for _ in range(4)]
    pairs += [(v, v) for v in (rng.getrandbits(32), 0xAAAAAAAA)] + [(0xAAAAAAAA, 0x55555555)]
    q = O.g1_mul(O.G1_GEN, rng.randrange(1, O.R))
    s = O.g1_mul(O.G1_GEN, rng.randrange(1, O.R))
    z = rng.randrange(2, O.P)
    points = [
        (O.G1_GEN, (O.G1_GEN[0], O.G1_GEN[1], 1)),
        (q, (q[0], q[1], 1)),
        (s, (s[0] * z % O.P, s[1] * z % O.P, z)),  # homogeneous projective, Z != 1
        (None, (0, 1, 0)),
    ]
    for aff, proj in points:
        for a, b in pairs:
            k = (a + b * LAMBDA) % O.R
            assert endo_mul(proj, a, b) == O.g1_mul(aff, k), (proj, a, b)


def test_scalar_map_nonzero_and_injective():
    """(a, b) -> a + b lambda mod r is zero only at (0, 0) and collision-free: a few thousand seeded pairs plus the
    corner pairs.  (In general: a - b x^2 is an integer of magnitude below 2^160 < r, and a < 2^32 < x^2.)"""
    rng = random.Random(0x5EED)
    pairs = set(CORNERS) | {(rng.getrandbits(32), rng.getrandbits(32)) for _ in range(4000)}
    # near-collisions: pairs that differ in one half only, and by one
    base = [(rng.getrandbits(32), rng.getrandbits(32)) for _ in range(200)]
    pairs |= {((a + 1) & M32, b) for a, b in base} | {(a, (b + 1) & M32) for a, b in base} | set(base)
    seen = {}
    for a, b in pairs:
        k = (a + b * LAMBDA) % O.R
        assert (k == 0) == ((a, b) == (0, 0)), (a, b)
        assert seen.setdefault(k, (a, b)) == (a, b), (a, b, seen[k])
    assert len(seen) == len(pairs)
