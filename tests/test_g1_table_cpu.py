"""Host side of the resident G1 table: the per-lane pieces of its MSM (csrc/bls_g1_msm.h: digit split, run folds,
bit sums, window step) in a host build with the digit form's column, value and subtraction checks compiled in
(tests/hostcheck_g1msm), against the Python oracle's G1 arithmetic; and the Python planning -- G1Table's index
map and the routing of curve.G1Point -- with a stub in place of the device."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

from oracle import bls_oracle as O

import g1_table_edge_inputs as E

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DIR = os.path.join(HERE, "hostcheck_g1msm")
LIB = os.path.join(DIR, "libhostcheck_g1msm.so")
INC = os.path.join(ROOT, "eth-consensus-specs_amd", "csrc")

P = O.P
MASK = 2 ** 29 - 1
RM = 2 ** 406  # the digit form's Montgomery radix
RINV = pow(RM, -1, P)
LD = 2 ** 29 + 2 ** 4  # the L-form digit bound of the accumulator contract (bls_fq_g1.h)

_lib = None


def lib():
    global _lib
    if _lib is None:
        deps = [os.path.join(DIR, f) for f in ("hostcheck_g1msm.cpp", "Makefile")]
        deps += [os.path.join(INC, f) for f in os.listdir(INC) if f.endswith(".h")]
        if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(d) for d in deps):
            subprocess.check_call(["make", "-C", DIR], timeout=2400)
        _lib = ctypes.CDLL(LIB)
        _lib.hc_g1m_k.restype = ctypes.c_uint32
        _lib.hc_g1m_digits.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
        _lib.hc_g1m_step.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_char_p]
        _lib.hc_g1m_msm.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p,
                                    ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p,
                                    ctypes.c_void_p]
    return _lib


def test_run_length_matches_the_source():
    with open(os.path.join(INC, "bls_g1_msm.h")) as fh:
        m = re.search(r"constexpr uint32_t G1M_K = (\d+);", fh.read())
    assert m and int(m.group(1)) == E.K == lib().hc_g1m_k()
    with open(os.path.join(INC, "bls_g1_msm.h")) as fh:
        assert re.search(r"constexpr int G1M_WINDOWS = %d;" % E.WINDOWS, fh.read())


def digits(k):
    out = ctypes.create_string_buffer(32)
    lib().hc_g1m_digits(E.k32(k), out)
    return list(out.raw)


def test_digit_split():
    rng = random.Random(0xD161)
    for k in E.EDGE_SCALARS + [E.ONES, 255 * E.ONES] + [rng.randrange(1 << 256) for _ in range(50)]:
        assert digits(k) == [(k >> (8 * w)) & 0xFF for w in range(32)], hex(k)
    assert digits(0) == [0] * 32 and digits(E.ONES) == [1] * 32 and digits((1 << 256) - 1) == [255] * 32


# ---- one step of every per-lane loop, operands at the declared bounds ---------------------------------------------
def dig(v):
    return [(v >> (29 * i)) & MASK for i in range(13)] + [v >> 377]


def val(d):
    return sum(x << (29 * i) for i, x in enumerate(d))


def dec_pt(d):
    return tuple(val(c) * RINV % P for c in d)


def worst(vbound, digit):
    """digits 0..12 all at `digit`, the top digit as large as a value below vbound p allows"""
    low = [digit] * 13
    top = (vbound * P - 1 - val(low + [0])) >> 377
    d = low + [top]
    assert (vbound - 1) * P < val(d) < vbound * P
    return d


def poly_add(p, q):
    X1, Y1, Z1 = p
    X2, Y2, Z2 = q
    xy, yz, xz = X1 * Y2 + X2 * Y1, Y1 * Z2 + Y2 * Z1, X1 * Z2 + X2 * Z1
    m, s = Y1 * Y2 - 12 * Z1 * Z2, Y1 * Y2 + 12 * Z1 * Z2
    return ((xy * m - 12 * yz * xz) % P, (m * s + 36 * X1 * X2 * xz) % P, (s * yz + 3 * X1 * X2 * xy) % P)


def poly_dbl(p):
    X, Y, Z = p
    w = Y * Y - 36 * Z * Z
    return (2 * w * X * Y % P, (w * (Y * Y + 12 * Z * Z) + 96 * Y * Y * Z * Z) % P, 8 * Y * Y * Y * Z % P)


def step(op, acc, mem):
    a = np.array([x for c in acc for x in c], dtype=np.uint32)
    raw = b"".join(int(c).to_bytes(48, "big") for c in mem)
    out_d = np.zeros(42, dtype=np.uint32)
    out_b = ctypes.create_string_buffer(144)
    lib().hc_g1m_step(op, a.ctypes.data, raw, out_d.ctypes.data, out_b)
    d = [[int(x) for x in out_d[14 * k: 14 * k + 14]] for k in range(3)]
    packed = tuple(int.from_bytes(out_b.raw[48 * k: 48 * k + 48], "big") for k in range(3))
    # every output is an accumulator again (X < 66p, Y, Z < 4p, digits <= 2^29 + 2^4: the contract that closes
    # each loop); the packed value is canonical
    for c, lim in zip(d, (66, 4, 4)):
        assert val(c) < lim * P and all(x <= LD for x in c[:13])
    assert packed == dec_pt(d)
    return packed


def test_steps_at_the_declared_bounds():
    """Every loop's step from an accumulator with every digit and value at the accumulator contract's bound
    (X < 66p, Y, Z < 4p, digits 2^29 + 2^4; for the Horner step, whose doubling takes any coordinate up to 66p,
    that too) and the memory operand at the largest canonical value, p - 1: the 128-bit column and subtraction
    checks hold and the result is the formula's polynomial.  (Polynomial identities: no curve points needed.)"""
    acc = [worst(66, LD), worst(4, LD), worst(4, LD)]
    any66 = [worst(66, LD)] * 3
    zero_y = [worst(66, LD), dig(0), worst(4, LD)]
    top = (P - 1, P - 1, P - 1)
    rng = random.Random(7)
    for mem in (top, (P - 1, 1, 0), tuple(rng.randrange(P) for _ in range(3))):
        for a in (acc, zero_y):
            assert step(0, a, mem) == poly_add(dec_pt(a), (mem[0], mem[1], 1))
            assert step(1, a, mem) == poly_add(dec_pt(a), mem)
        for a in (acc, any66):
            assert step(2, a, mem) == poly_add(poly_dbl(dec_pt(a)), mem)
        want = mem
        for _ in range(8):
            want = poly_dbl(want)
        assert step(3, acc, mem) == want


# ---- the whole MSM as the device runs it ---------------------------------------------------------------------------
def msm(points, idx, rows):
    """(rc, sums, info): points are affine (x, y), None for the identity, "bad" for an invalid entry"""
    state = bytes(0 if p == "bad" else 2 if p is None else 1 for p in points)
    raw = b"".join(bytes(96) if p in (None, "bad") else p[0].to_bytes(48, "big") + p[1].to_bytes(48, "big")
                   for p in points)
    a_idx = np.ascontiguousarray(idx, dtype=np.uint32)
    B, n = len(rows), len(idx)
    ks = b"".join(E.k32(k) for row in rows for k in row)
    out = ctypes.create_string_buffer(96 * max(B, 1))
    info = np.zeros(3, dtype=np.uint32)
    rc = lib().hc_g1m_msm(raw, state, len(points), a_idx.ctypes.data, n, ks, B, out, info.ctypes.data)
    sums = []
    for v in range(B):
        r = out.raw[96 * v: 96 * v + 96]
        sums.append(None if r == bytes(96) else (int.from_bytes(r[:48], "big"), int.from_bytes(r[48:], "big")))
    return rc, sums, info.tolist()


@pytest.fixture(scope="module")
def pts():
    rng = random.Random(0x61AB)
    return [O.g1_mul(O.G1_GEN, rng.randrange(1, O.R)) for _ in range(4)]


def test_runs_of_equal_points_around_the_run_length(pts):
    """m copies of one entry with scalar 1 put m equal records into one bucket -- the doubling case of the complete
    addition at every step -- for m = K - 1, K, K + 1 and K^2 + 1 (a third level); scalar ONES does it in all 32
    windows at once."""
    K = E.K
    p = pts[0]
    for m in (K - 1, K, K + 1, K * K + 1):
        rc, sums, info = msm([p], [0] * m, [[1] * m, [E.ONES] * m])
        assert rc == 0
        assert sums == [O.g1_mul(p, m), O.g1_mul(p, m * E.ONES % O.R)]
        assert info[1] == m + 32 * m and info[2] == -(-m // K) + -(-32 * m // K)  # row 1: one bucket of 32 m
    assert msm([p], [0], [[1]])[2][0] == 2 and msm([p], [0] * (K * K + 1), [[1] * (K * K + 1)])[2][0] == 4


def test_edge_scalars_cancellation_and_identity_records(pts):
    """Every edge scalar on one point (digits 0, 1 and 255 in every window among them; 2^256 - 1 is 255 in all 32);
    P then -P with equal scalars cancels to the identity; identity entries add nothing and leave no bucket entry."""
    p, q = pts[1], pts[2]
    n = len(E.EDGE_SCALARS)
    rc, sums, _ = msm([p], [0], [[k] for k in E.EDGE_SCALARS + [E.ONES, 255 * E.ONES]])
    assert rc == 0
    assert sums == [O.g1_mul(p, k % O.R) if k % O.R else None for k in E.EDGE_SCALARS + [E.ONES, 255 * E.ONES]]
    assert sums[0] is None and sums[E.EDGE_SCALARS.index(O.R)] is None and n == 10
    big = (1 << 256) - 1
    table = [None, p, O.g1_neg(p), q]
    rc, sums, info = msm(table, [1, 2, 0, 3, 0], [[big, big, 5, 0, big], [7, 7, 1, 3, 9], [0] * 5])
    assert rc == 0 and sums == [None, O.g1_mul(q, 3), None]
    assert info[1] == 64 + 2 + 1  # 32 + 32 digits of row 0, the digits of 7, 7 and 3 of row 1, none of an identity


def test_random_vectors_and_refusals(pts):
    rng = random.Random(3)
    idx = [3, 0, 1, 3, 2, 0, 1]
    rows = [[rng.randrange(1 << 256) for _ in idx] for _ in range(2)]
    rc, sums, _ = msm(pts, idx, rows)
    assert rc == 0
    for v in range(2):
        want = None
        for i, k in zip(idx, rows[v]):
            want = O.g1_add(want, O.g1_mul(pts[i], k % O.R))
        assert sums[v] == want
    assert msm(pts, [0, 4], [[1, 1]])[0] == -1
    assert msm(pts + ["bad"], [0, 4], [[1, 0]])[0] == -2


# ---- Python planning without a device ------------------------------------------------------------------------------
class FakeLib:
    """the table entry points' bookkeeping: sizes, generations, verdicts (an encoding starting 0xff is invalid)"""

    def __init__(self):
        self.n, self.gen, self.msm, self.decodes, self.mexp = 0, 0, [], 0, []

    def _fill(self, buf, n, ok):
        out = ctypes.cast(ok, ctypes.POINTER(ctypes.c_uint8))
        for i in range(n):
            out[i] = 0 if buf[48 * i] == 0xFF else 1

    def bls_g1_table_load(self, h, buf, n, sg, ok):
        self.n, self.gen = n, self.gen + 1
        self._fill(buf, n, ok)
        return 1

    def bls_g1_table_append(self, h, buf, n, sg, ok):
        self.n += n
        self._fill(buf, n, ok)
        return 1

    def bls_g1_table_size(self, h):
        return self.n

    def bls_g1_table_generation(self, h):
        return self.gen

    def bls_point_decode(self, h, group, b, n, sg, ok):
        self.decodes += 1
        return 1

    def bls_multi_exp(self, h, group, pts, ks, n, sg, out):
        self.mexp.append((group, n, sg))
        return 1


class FakeCtx:
    def __init__(self):
        self.lib, self.h = FakeLib(), None

    def check(self, rc):
        return rc


def _pt(i, bad=False):
    return bytes([0xFF if bad else 0x80 | (i & 0x1F)]) + i.to_bytes(47, "big")


def test_table_indices_and_stale_generation():
    from bls_mi355x import batch

    ctx = FakeCtx()
    t = batch.G1Table(ctx)
    a, b, c, d = (_pt(i) for i in range(4))
    assert t.indices([a]) is None  # nothing loaded
    ok = t.load(a + b + a + _pt(9, bad=True))
    assert ok.tolist() == [1, 1, 1, 0] and len(t) == 4 and t.checked is False
    assert t.indices([b, a, a]).tolist() == [1, 0, 0] and t.indices([b, a]).dtype == np.uint32
    assert t.indices([a, c]) is None and t.indices([]).size == 0
    assert t.usable(1) and not t.usable(3) and not t.usable(4)
    assert t.append([c, d], subgroup_check=True).tolist() == [1, 1]
    assert t.indices([d, c, b]).tolist() == [5, 4, 1] and len(t) == 6 and t.checked is False
    other = batch.G1Table(ctx)
    other.load([d], subgroup_check=True)
    assert other.checked and other.indices([d]).tolist() == [0]
    assert t.indices([a]) is None and not t.usable(0)  # the device table was replaced under t
    t.append([a])  # an append to a table that is not t's: nothing is remembered
    assert t.indices([a]) is None and other.indices([a]) is None
    with pytest.raises(ValueError):
        t.load(b"\x00" * 47)


def test_multiexp_and_decode_routing(monkeypatch):
    from bls_mi355x import batch, curve

    ctx = FakeCtx()
    monkeypatch.setattr(curve, "_ctx", lambda: ctx)
    calls = []

    def lincomb(table, idx, scalars):
        calls.append((np.asarray(idx).tolist(), list(scalars)))
        return curve.G1_IDENTITY

    monkeypatch.setattr(batch, "g1_lincomb_indexed", lincomb)
    G1 = curve.G1Point
    a, b, c, bad = _pt(1), _pt(2), _pt(3), _pt(9, bad=True)
    pa, pb, pc, pbad = (G1._wrap(x) for x in (a, b, c, bad))
    t = batch.G1Table(ctx)
    t.load([a, b, bad])
    try:
        # no table set: today's route
        G1.multiexp_unchecked([pa, pb], [1, 2])
        assert calls == [] and ctx.lib.mexp == [(1, 2, 0)]
        curve.use_g1_table(t)
        G1.multiexp_unchecked([pb, pa, pb], [1, curve.Scalar(2), O.R + 3])
        assert calls == [([1, 0, 1], [1, 2, 3])] and len(ctx.lib.mexp) == 1  # scalars reduced as the old route's
        G1.multiexp_unchecked([pa, pc], [1, 2])       # one point outside the table
        G1.multiexp([pa, pb], [1, 2])                 # the check asked of an unchecked table
        G1.multiexp_unchecked([pa, pbad], [1, 2])     # an unusable entry: the old route reports it
        curve.G2Point.multiexp_unchecked([curve.G2Point()], [5])
        assert len(calls) == 1 and ctx.lib.mexp[1:] == [(1, 2, 0), (1, 2, 1), (1, 2, 0), (2, 1, 0)]
        with pytest.raises(ValueError):
            G1.multiexp_unchecked([], [])
        # decodes: a usable entry is served from the table, anything else goes to the device
        assert batch.g1_table_stats.__doc__ and getattr(ctx, "g1_decode_hits", 0) == 0
        assert G1.from_compressed_bytes_unchecked(a) == pa and ctx.lib.decodes == 0 and ctx.g1_decode_hits == 1
        G1.from_compressed_bytes_unchecked(c)
        G1.from_compressed_bytes_unchecked(bad)
        G1.from_compressed_bytes(a)  # checked decode, unchecked table
        assert ctx.lib.decodes == 3 and ctx.g1_decode_hits == 1
        t.load([a, b], subgroup_check=True)
        G1.from_compressed_bytes(a)
        G1.multiexp([pa, pb], [1, 2])
        assert ctx.lib.decodes == 3 and ctx.g1_decode_hits == 2 and len(calls) == 2
        batch.G1Table(ctx).load([c])  # replaced under t: stale, everything takes the old route
        G1.multiexp_unchecked([pa], [1])
        G1.from_compressed_bytes_unchecked(a)
        assert len(calls) == 2 and ctx.lib.decodes == 4
    finally:
        curve.use_g1_table(None)
    G1.from_compressed_bytes_unchecked(a)
    assert ctx.lib.decodes == 5


def test_header_declares_what_native_binds():
    from bls_mi355x import _native

    with open(os.path.join(ROOT, "include", "blsmi355x.h")) as fh:
        hdr = fh.read()
    for name in ("bls_g1_table_load", "bls_g1_table_append", "bls_g1_table_msm", "bls_g1_table_stats"):
        m = re.search(r"^int %s\(([^;]*)\);" % name, hdr, re.M)
        assert m, name
        assert len(m.group(1).split(",")) == len(_native._SIGS[name][1]), name
    lib_ = _native.load_library()
    for name in _native.EXPORTS:
        if name.startswith("bls_g1_table"):
            assert hasattr(lib_, name), name
