"""Host side of the RLC signature MSM's bucket sums: the per-lane folds of csrc/bls_g2_msm.h (what k_msm_fold0 and
k_msm_fold1 run) in a host build with the digit form's column, value and subtraction checks compiled in
(tests/hostcheck_g2msm), against the Python oracle's g2_add.  A violated bound aborts the harness, so a passing
case also says that an accumulator started from a canonical point stays inside the declared contract."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

from oracle import bls_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "hostcheck_g2msm")
LIB = os.path.join(DIR, "libhostcheck_g2msm.so")
INC = os.path.join(os.path.dirname(HERE), "eth-consensus-specs_amd", "csrc")

_lib = None


def lib():
    global _lib
    if _lib is None:
        deps = [os.path.join(DIR, f) for f in ("hostcheck_g2msm.cpp", "Makefile")]
        deps += [os.path.join(INC, f) for f in os.listdir(INC) if f.endswith(".h")]
        if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(d) for d in deps):
            subprocess.check_call(["make", "-C", DIR], timeout=2400)
        _lib = ctypes.CDLL(LIB)
        _lib.hc_g2msm_kmax.restype = ctypes.c_uint32
        _lib.hc_g2msm_bucket.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_uint32,
                                         ctypes.c_uint32, ctypes.c_char_p, ctypes.c_void_p]
        _lib.hc_g2msm_partials.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p]
    return _lib


def _f2(b):
    return (int.from_bytes(b[:48], "big"), int.from_bytes(b[48:96], "big"))


def _f2b(a):
    return a[0].to_bytes(48, "big") + a[1].to_bytes(48, "big")


def _result(rc, out):
    """an affine point, None for the identity (Z = 0: the complete formulas leave (0 : Y != 0 : 0))"""
    r = out.raw
    if rc == 2:
        assert _f2(r[:96]) == (0, 0) and _f2(r[96:192]) != (0, 0)
        return None
    assert rc == 1
    return (_f2(r[:96]), _f2(r[96:192]))


def bucket(points, lst, K):
    """(sum, info): one bucket's entries lst (indices into points) through both fold levels at run length K"""
    raw = b"".join(_f2b(p[0]) + _f2b(p[1]) for p in points)
    a = np.ascontiguousarray(lst, dtype=np.uint32)
    out = ctypes.create_string_buffer(192)
    info = np.zeros(3, dtype=np.uint32)
    rc = lib().hc_g2msm_bucket(raw, len(points), a.ctypes.data, len(lst), K, out, info.ctypes.data)
    return _result(rc, out), info.tolist()


def partials(prj):
    """the partial fold of projective points (X, Y, Z), each an Fp2 pair"""
    raw = b"".join(_f2b(c) for p in prj for c in p)
    out = ctypes.create_string_buffer(192)
    return _result(lib().hc_g2msm_partials(raw, len(prj), out), out)


def osum(pts):
    s = None
    for p in pts:
        s = O.g2_add(s, p)
    return s


@pytest.fixture(scope="module")
def pts():
    rng = random.Random(0x62A7)
    step = O.g2_mul(O.G2_GEN, rng.randrange(1, O.R))
    out, cur = [], O.g2_mul(O.G2_GEN, rng.randrange(1, O.R))
    for _ in range(2 * 16 + 2):
        out.append(cur)
        cur = O.g2_add(cur, step)
    return out


@pytest.mark.parametrize("K", [4, 16])
def test_record_fold_sizes(pts, K):
    """1, 2, K - 1, K (one run: no addition to the identity, the sum written directly), K + 1 (two runs) and
    2 K + 1 points (three runs, cut evenly)"""
    for n in (1, 2, K - 1, K, K + 1, 2 * K + 1):
        got, info = bucket(pts, list(range(n)), K)
        assert got == osum(pts[:n]), n
        runs = -(-n // K)
        assert info[0] == runs and info[1] - info[2] <= 1 and info[1] == -(-n // runs), (n, info)
    assert bucket(pts, [], K) == (None, [0, 0, 0xFFFFFFFF])  # no entries: the identity as k_msm_usum reads it


def test_even_split():
    """39 entries at K = 16 are 13 + 13 + 13, not 16 + 16 + 7"""
    g = O.G2_GEN
    got, info = bucket([g], [0] * 39, 16)
    assert info == [3, 13, 13]
    assert got == O.g2_mul(g, 39)


def test_doublings_and_cancellation(pts):
    K = 4
    p, q, r = pts[0], pts[1], pts[2]
    assert bucket([p], [0, 0], K)[0] == O.g2_add(p, p)  # the same point twice: a doubling inside the formulas
    assert bucket([p], [0, 0, 0], K)[0] == O.g2_mul(p, 3)  # ... and three times
    # sigma and -sigma: (0 : Y : 0); then more points added to it, in the same run and across the partial fold
    assert bucket([p, O.g2_neg(p)], [0, 1], K)[0] is None
    assert bucket([p, O.g2_neg(p), q], [0, 1, 2], K)[0] == q
    assert bucket([p, O.g2_neg(p), q, r], [0, 1, 2, 3, 3, 2], K)[0] == O.g2_mul(O.g2_add(q, r), 2)
    # a whole run that cancels is an identity partial of the second fold: first, in the middle, and every run
    m = [p, O.g2_neg(p), q, O.g2_neg(q), r]
    qr = O.g2_add(q, r)
    assert bucket(m, [0, 1, 1, 0, 2, 4, 4, 2], K) == (O.g2_mul(qr, 2), [2, 4, 4])
    assert bucket(m, [2, 4, 4, 2, 0, 1, 1, 0, 4, 4, 2, 2], K) == (O.g2_mul(qr, 4), [3, 4, 4])
    assert bucket(m, [0, 1, 1, 0, 2, 3, 3, 2], K)[0] is None


def test_partial_fold(pts):
    """1, 2 and K + 1 partials, with the identity (0 : 1 : 0) first, in the middle and alone; projective partials
    with Z != 1"""
    K = lib().hc_g2msm_kmax()
    one, zero = (1, 0), (0, 0)
    ident = (zero, one, zero)

    def prj(p, z):  # (x z, y z, z), z in Fp
        return ((p[0][0] * z % O.P, p[0][1] * z % O.P), (p[1][0] * z % O.P, p[1][1] * z % O.P), (z, 0))

    assert partials([prj(pts[0], 1)]) == pts[0]
    assert partials([prj(pts[0], 5), prj(pts[1], 7)]) == O.g2_add(pts[0], pts[1])
    many = [prj(p, 3 + i) for i, p in enumerate(pts[:K + 1])]
    assert partials(many) == osum(pts[:K + 1])
    assert partials([ident]) is None
    assert partials([ident, prj(pts[0], 2)]) == pts[0]
    assert partials([prj(pts[0], 2), ident, prj(pts[1], 9)]) == O.g2_add(pts[0], pts[1])
    assert partials([prj(pts[0], 2), prj(pts[0], 3)]) == O.g2_add(pts[0], pts[0])
    assert partials([prj(pts[0], 2), prj(O.g2_neg(pts[0]), 3), prj(pts[2], 4)]) == pts[2]
