"""The Miller loop's G2 line steps (csrc/bls_miller_lines.h: ln_dbl, ln_add -- homogeneous projective doubling and
mixed addition with the line coefficients) on the CPU: a host build of the header with the digit form's column,
value and subtraction checks compiled in (tests/hostcheck_mlines), against the Python oracle.

For Q = [k] hash_to_G2(..) the 68 steps of the loop over |x| must keep T, as an affine point, equal to the oracle's
running multiple of Q, and each step's record (l0, l2, l3) must be the affine line's coefficients times one
non-zero Fp2 factor:
    doubling at T = (x, y):       (y^2 - 3 b' : 3 x^2 : 2 y)
    addition of Q to T = (x, y):  (theta x_Q - lambda y_Q : theta : lambda),  theta = y - y_Q, lambda = x - x_Q
(the accumulation evaluates l0 + l2 (-x_P) v + l3 y_P v w; the Fp2 factor dies in the final exponentiation).

The same host build runs the mixed Jacobian addition of the signature subgroup chain (csrc/bls_fq_g2.h:
j2q_add_aff, Z2 = 1): [|x|] sigma against the oracle's g2_mul, single additions against g2_add, and the exceptional
inputs (h = 0, Z = 0, and the chain on a point of order 13), which must raise exc.
"""
import ctypes
import os
import subprocess

import pytest

from oracle import bls_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "hostcheck_mlines")
LIB = os.path.join(DIR, "libhostcheck_mlines.so")
INC = os.path.join(os.path.dirname(HERE), "eth-consensus-specs_amd", "csrc")

NSTEPS = 68
REC = 577

_lib = None


def lib():
    global _lib
    if _lib is None:
        deps = [os.path.join(DIR, f) for f in ("hostcheck_mlines.cpp", "Makefile")]
        deps += [os.path.join(INC, f) for f in os.listdir(INC) if f.endswith(".h")]
        if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(d) for d in deps):
            subprocess.check_call(["make", "-C", DIR], timeout=2400)
        _lib = ctypes.CDLL(LIB)
        _lib.hc_ml_steps.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
        _lib.hc_ml_steps.restype = ctypes.c_int
        _lib.hc_sig_xabs.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
        _lib.hc_sig_xabs.restype = ctypes.c_int
        _lib.hc_madd.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p]
        _lib.hc_madd.restype = ctypes.c_int
    return _lib


def _f2_b(a):
    return a[0].to_bytes(48, "big") + a[1].to_bytes(48, "big")


def _f2(b):
    return (int.from_bytes(b[:48], "big"), int.from_bytes(b[48:96], "big"))


def steps(q):
    """[(kind, (X, Y, Z), (l0, l2, l3))] for the 68 steps on the affine point q"""
    out = ctypes.create_string_buffer(NSTEPS * REC)
    assert lib().hc_ml_steps(_f2_b(q[0]) + _f2_b(q[1]), out) == NSTEPS
    res = []
    for k in range(NSTEPS):
        r = out.raw[REC * k: REC * k + REC]
        v = [_f2(r[1 + 96 * j: 97 + 96 * j]) for j in range(6)]
        res.append((r[0], tuple(v[:3]), tuple(v[3:])))
    return res


def _proportional(rec, line):
    """rec = c line for one non-zero c in Fp2, by cross-multiplication"""
    assert any(w != O.F2_ZERO for w in rec), "zero record"
    for i in range(3):
        for j in range(i + 1, 3):
            assert O.f2_mul(rec[i], line[j]) == O.f2_mul(rec[j], line[i]), (i, j)
    # the factor is non-zero: a zero record word only where the line's is zero
    for w, l in zip(rec, line):
        assert (w == O.F2_ZERO) == (l == O.F2_ZERO)


THREE_B = O.f2_muls(O.B2, 3)


@pytest.mark.parametrize("seed,k", [(1, 1), (2, 0x1234567), (3, O.R - 5)])
def test_steps_follow_the_oracle(seed, k):
    q = O.g2_mul(O.hash_to_g2(b"miller line steps %d" % seed), k)
    t = q
    bits = [(O.X_ABS >> b) & 1 for b in range(62, -1, -1)]
    want = []
    for bit in bits:
        want.append(0)
        if bit:
            want.append(1)
    got = steps(q)
    assert [g[0] for g in got] == want
    for kind, (X, Y, Z), rec in got:
        x, y = t
        if kind == 0:
            line = (O.f2_sub(O.f2_sqr(y), THREE_B), O.f2_muls(O.f2_sqr(x), 3), O.f2_muls(y, 2))
            t = O.g2_add(t, t)
        else:
            theta, lam = O.f2_sub(y, q[1]), O.f2_sub(x, q[0])
            line = (O.f2_sub(O.f2_mul(theta, q[0]), O.f2_mul(lam, q[1])), theta, lam)
            t = O.g2_add(t, q)
        _proportional(rec, line)
        assert Z != O.F2_ZERO
        zi = O.f2_inv(Z)
        assert (O.f2_mul(X, zi), O.f2_mul(Y, zi)) == t
    assert t == O.g2_mul(q, O.X_ABS)


# ---- the mixed Jacobian addition of the [|x|] sigma chain ------------------------------------------------------
def _jac_to_affine(raw):
    X, Y, Z = (_f2(raw[96 * j: 96 * j + 96]) for j in range(3))
    if Z == O.F2_ZERO:
        return None
    zi = O.f2_inv(Z)
    zi2 = O.f2_sqr(zi)
    return (O.f2_mul(X, zi2), O.f2_mul(Y, O.f2_mul(zi2, zi)))


def sig_xabs(q):
    out = ctypes.create_string_buffer(288)
    exc = lib().hc_sig_xabs(_f2_b(q[0]) + _f2_b(q[1]), out)
    return exc, _jac_to_affine(out.raw)


def madd(p_jac, q):
    out = ctypes.create_string_buffer(288)
    exc = lib().hc_madd(b"".join(_f2_b(c) for c in p_jac), _f2_b(q[0]) + _f2_b(q[1]), out)
    return exc, _jac_to_affine(out.raw)


def _e2_point(x0):
    """a point of E2(Fp2) with x = (x0, 1), any order"""
    x = x0
    while True:
        X = (x, 1)
        y = O.f2_sqrt(O.f2_add(O.f2_mul(O.f2_sqr(X), X), O.B2))
        if y is not None:
            return (X, y)
        x += 1


# the G2 cofactor
H2 = 0x5D543A95414E7F1091D50792876A202CD91DE4547085ABAA68A205B2E5A7DDFA628F1CB4D9E82EF21537E293A6691AE1616EC6E786F0C70CF1C38E31C7238E5


def _small_order_e2(q):
    """a point of E2 of order q, q = 13 or 23 (q^2 divides the G2 cofactor and E2's q-part has exponent q)"""
    x = 1
    while True:
        Q = O.g2_mul(_e2_point(x), H2 * O.R // (q * q))
        if Q is not None:
            assert O.g2_mul(Q, q) is None
            return Q
        x += 1


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_sig_chain_matches_oracle(seed):
    """[|x|] sigma for sigma in G2 and for a point of E2 outside G2 (large order: no exceptional step either)"""
    s = O.g2_mul(O.hash_to_g2(b"sigma %d" % seed), 0xABCDEF + seed)
    for pt in (s, _e2_point(seed)):
        exc, got = sig_xabs(pt)
        assert exc == 0
        assert got == O.g2_mul(pt, O.X_ABS)


def test_mixed_addition_matches_oracle_and_flags_exceptions():
    s = O.g2_mul(O.hash_to_g2(b"madd"), 77)
    t = O.g2_mul(s, 5)
    z = (0x1234567, 0x89ABCDE)
    z2 = O.f2_sqr(z)
    t_jac = (O.f2_mul(t[0], z2), O.f2_mul(t[1], O.f2_mul(z2, z)), z)  # Z != 1
    exc, got = madd(t_jac, s)
    assert exc == 0 and got == O.g2_add(t, s)
    one = (1, 0)
    assert madd((s[0], s[1], one), s)[0] == 1                      # h = 0: T = Q
    assert madd((s[0], O.f2_neg(s[1]), one), s)[0] == 1            # h = 0: T = -Q
    s_jac = (O.f2_mul(s[0], z2), O.f2_mul(s[1], O.f2_mul(z2, z)), z)
    assert madd(s_jac, s)[0] == 1                                  # h = 0 with Z != 1
    assert madd((one, one, O.F2_ZERO), s)[0] == 1                  # Z = 0: T the identity


def _chain_meets_exception(order):
    """whether an addition of the chain over |x| finds T = [2k] sigma equal to +-sigma or the identity, for sigma
    of this order: the prefixes k of |x| at its set bits, from the arithmetic alone"""
    k = 1
    for b in range(62, -1, -1):
        k = 2 * k
        if (O.X_ABS >> b) & 1:
            if k % order in (0, 1, order - 1):
                return True
            k += 1
    return False


@pytest.mark.parametrize("order", [13, 23])
def test_sig_chain_on_small_order_points(order):
    """a point of order 13 or 23: exc exactly when a running multiple meets +-sigma or the identity at an addition
    (order 13 does, at the second addition: 2 x 6 = -1 mod 13); without one the chain's result is still [|x|] sigma"""
    pt = _small_order_e2(order)
    exc, got = sig_xabs(pt)
    assert exc == int(_chain_meets_exception(order))
    if not exc:
        assert got == O.g2_mul(pt, O.X_ABS)


def test_order_13_is_an_exceptional_case():
    assert _chain_meets_exception(13)
