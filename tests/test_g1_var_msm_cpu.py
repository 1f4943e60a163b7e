"""Host side of the bucket MSM over a call's own G1 points (bls_g1_msm): the per-lane pieces that are its own
(csrc/bls_g1_var_msm.h: the (row, window, digit) slots and the window chain) and a whole small MSM, run in a host build
with the digit form's column, value and subtraction checks compiled in (tests/hostcheck_g1vmsm), against the Python
oracle's G1 arithmetic; and batch.g1_msm / g1_msm_stats with a stub in place of the library."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

from oracle import bls_oracle as O

import g1_table_edge_inputs as E

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DIR = os.path.join(HERE, "hostcheck_g1vmsm")
LIB = os.path.join(DIR, "libhostcheck_g1vmsm.so")
INC = os.path.join(ROOT, "eth-consensus-specs_amd", "csrc")

P = O.P
MASK = 2 ** 29 - 1
RM = 2 ** 406  # the digit form's Montgomery radix
RINV = pow(RM, -1, P)
LD = 2 ** 29 + 2 ** 4  # the L-form digit bound of the accumulator contract (bls_fq_g1.h)
W32 = E.WINDOWS

_lib = None


def lib():
    global _lib
    if _lib is None:
        deps = [os.path.join(DIR, f) for f in ("hostcheck_g1vmsm.cpp", "Makefile")]
        deps += [os.path.join(INC, f) for f in os.listdir(INC) if f.endswith(".h")]
        if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(d) for d in deps):
            subprocess.check_call(["make", "-C", DIR], timeout=2400)
        _lib = ctypes.CDLL(LIB)
        _lib.hc_g1vm_k.restype = ctypes.c_uint32
        _lib.hc_g1vm_slots.restype = ctypes.c_uint32
        _lib.hc_g1vm_slots.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_void_p]
        _lib.hc_g1vm_step.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_char_p]
        _lib.hc_g1vm_combine.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
        _lib.hc_g1vm_msm.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p,
                                     ctypes.c_size_t, ctypes.c_char_p, ctypes.c_void_p]
    return _lib


def test_run_length_is_the_tables():
    assert lib().hc_g1vm_k() == E.K


# ---- the sort's slots ----------------------------------------------------------------------------------------------
def slots(k, v):
    out = np.zeros(32, dtype=np.uint32)
    c = lib().hc_g1vm_slots(E.k32(k), v, out.ctypes.data)
    return out[:c].tolist()


def test_slot_of_every_digit():
    """Every non-zero digit d of window w of row v goes to slot (v * 32 + w) * 256 + d, windows ascending, and a zero
    digit to none: the edge scalars (digits 0, 1, 255 in every window), single digits in every window, 2^(8w) - 1
    beside 2^(8w), and random ones, in rows 0, 1 and 255 (the last row a call may have)."""
    rng = random.Random(0x51075)
    ks = E.EDGE_SCALARS + [E.ONES, 255 * E.ONES]
    ks += [d << (8 * w) for w in range(W32) for d in (1, 128, 255)]
    ks += [x for w in range(1, W32) for x in ((1 << (8 * w)) - 1, 1 << (8 * w))]
    ks += [rng.randrange(1 << 256) for _ in range(50)]
    for v in (0, 1, 255):
        for k in ks:
            want = [(v * W32 + w) * 256 + ((k >> (8 * w)) & 0xFF) for w in range(W32) if (k >> (8 * w)) & 0xFF]
            assert slots(k, v) == want, (v, hex(k))
    assert slots(0, 3) == [] and len(slots((1 << 256) - 1, 0)) == 32
    assert max(slots((1 << 256) - 1, 255)) == 256 * W32 * 256 - 1  # the last slot of the largest call


# ---- the window chain, operands at the declared bounds -------------------------------------------------------------
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


def poly_window(p, q):
    for _ in range(8):
        p = poly_dbl(p)
    return poly_add(p, q)


def be144(pt):
    return b"".join(int(c).to_bytes(48, "big") for c in pt)


def step(acc, mem):
    a = np.array([x for c in acc for x in c], dtype=np.uint32)
    out_d = np.zeros(42, dtype=np.uint32)
    out_b = ctypes.create_string_buffer(144)
    lib().hc_g1vm_step(a.ctypes.data, be144(mem), out_d.ctypes.data, out_b)
    d = [[int(x) for x in out_d[14 * k: 14 * k + 14]] for k in range(3)]
    packed = tuple(int.from_bytes(out_b.raw[48 * k: 48 * k + 48], "big") for k in range(3))
    # the output is an accumulator again, so the chain over 31 windows closes; the packed value is canonical
    for c, lim in zip(d, (66, 4, 4)):
        assert val(c) < lim * P and all(x <= LD for x in c[:13])
    assert packed == dec_pt(d)
    return packed


def test_window_step_at_the_declared_bounds():
    """One step of the chain -- eight doublings, then the addition of a canonical window sum -- from an accumulator
    with every digit and value at the contract's bound (X < 66p, Y, Z < 4p, digits 2^29 + 2^4), from one with every
    coordinate at 66p (what g1q_dbl and g1q_add admit), and from one with Y = 0; the window sum at p - 1: the 128-bit
    column and subtraction checks hold and the result is the formulas' polynomial.  (Polynomial identities: no curve
    points needed.)"""
    acc = [worst(66, LD), worst(4, LD), worst(4, LD)]
    any66 = [worst(66, LD)] * 3
    zero_y = [worst(66, LD), dig(0), worst(4, LD)]
    rng = random.Random(8)
    for mem in ((P - 1, P - 1, P - 1), (0, 1, 0), (P - 1, 1, 0), tuple(rng.randrange(P) for _ in range(3))):
        for a in (acc, any66, zero_y):
            assert step(a, mem) == poly_window(dec_pt(a), mem)


IDENT = (0, 1, 0)


def combine(ws):
    out = ctypes.create_string_buffer(144)
    top = lib().hc_g1vm_combine(b"".join(be144(w) for w in ws), out)
    return top, tuple(int.from_bytes(out.raw[48 * k: 48 * k + 48], "big") for k in range(3))


def test_window_chain_from_every_starting_window():
    """The chain starts at the row's highest window whose sum is not the identity (Z != 0): for every s, window sums
    at the largest canonical value p - 1 in window s and random ones below (every third the identity, which passes
    through the complete addition), identities above.  The result is Horner's polynomial from s down, so the windows
    above s cost no doubling."""
    rng = random.Random(0xC4A1)
    top_val = (P - 1, P - 1, P - 1)
    for s in range(W32):
        ws = [IDENT if w > s or (w < s and w % 3 == 2) else tuple(rng.randrange(P) for _ in range(3))
              for w in range(W32)]
        ws[s] = top_val
        want = ws[s]
        for w in range(s - 1, -1, -1):
            want = poly_window(want, ws[w])
        got_top, got = combine(ws)
        assert got_top == s and got == want, s
    top, got = combine([IDENT] * W32)
    assert top == 0 and got == IDENT  # a row of zeros


def test_window_chain_on_curve_points():
    """sum_w 2^(8w) W_w for window sums that are points of G1: the oracle's [sum_w 2^(8w) c_w] G for W_w = [c_w] G
    given in projective form with Z != 1, from top windows 0, 15 and 31."""
    rng = random.Random(0xC0DE)
    g = O.G1_GEN
    for s in (0, 15, 31):
        cs = [rng.randrange(1, 1 << 64) if w <= s and w % 4 != 1 else 0 for w in range(W32)]
        cs[s] = rng.randrange(1, 1 << 64)
        ws = []
        for c in cs:
            if not c:
                ws.append(IDENT)
                continue
            x, y = O.g1_mul(g, c)
            z = rng.randrange(2, P)
            ws.append((x * z % P, y * z % P, z))
        top, (X, Y, Z) = combine(ws)
        zi = pow(Z, -1, P)
        assert top == s and (X * zi % P, Y * zi % P) == O.g1_mul(g, sum(c << (8 * w) for w, c in enumerate(cs)) % O.R)


# ---- the whole MSM as the device runs it ---------------------------------------------------------------------------
def msm(points, rows):
    """(rc, sums, info): points are affine (x, y) or None for the identity"""
    state = bytes(2 if p is None else 1 for p in points)
    raw = b"".join(bytes(96) if p is None else p[0].to_bytes(48, "big") + p[1].to_bytes(48, "big") for p in points)
    B, n = len(rows), len(points)
    ks = b"".join(E.k32(k) for row in rows for k in row)
    out = ctypes.create_string_buffer(96 * max(B, 1))
    info = np.zeros(3, dtype=np.uint32)
    rc = lib().hc_g1vm_msm(raw, state, n, ks, B, out, info.ctypes.data)
    sums = []
    for v in range(B):
        r = out.raw[96 * v: 96 * v + 96]
        sums.append(None if r == bytes(96) else (int.from_bytes(r[:48], "big"), int.from_bytes(r[48:], "big")))
    return rc, sums, info.tolist()


@pytest.fixture(scope="module")
def pts():
    rng = random.Random(0x61AC)
    step_ = O.g1_mul(O.G1_GEN, rng.randrange(1, O.R))
    out, cur = [], O.g1_mul(O.G1_GEN, rng.randrange(1, O.R))
    for _ in range(6):
        out.append(cur)
        cur = O.g1_add(cur, step_)
    return out


def nonzero_digits(k):
    return sum(1 for b in E.k32(k) if b)


def test_small_msm_lane_by_lane(pts):
    """n = 37 drawn from six points with the identity among them, B = 2: a row of edge and random full-width scalars
    and a row of 128-bit ones (the rows' chains start at different windows).  Equal to the oracle's sum over the
    distinct points of (sum of their scalars) P; the bucket entries are the non-zero digits of non-identity points."""
    rng = random.Random(0x37)
    pool = pts[:5] + [None]
    pick = [rng.randrange(6) for _ in range(37)]
    assert len(set(pick)) == 6
    rows = [[rng.choice(E.EDGE_SCALARS) if i % 3 else rng.randrange(1 << 256) for i in range(37)],
            [rng.randrange(1 << 128) for _ in range(37)]]
    rc, sums, info = msm([pool[e] for e in pick], rows)
    assert rc == 0 and info[0] == 2  # 37 entries at most in a bucket: two levels
    for v in range(2):
        want = None
        for e in range(5):
            want = O.g1_add(want, O.g1_mul(pool[e], sum(k for i, k in zip(pick, rows[v]) if i == e) % O.R))
        assert sums[v] == want, v
    assert info[1] == sum(nonzero_digits(k) for row in rows for i, k in zip(pick, row) if pool[i] is not None)


def test_small_msm_run_lengths_and_cancellation(pts):
    """All scalars of a row equal: each window has one bucket holding every point, for n = K - 1, K, K + 1 (one and
    two levels); P and -P with equal scalars and a row of zeros give the identity."""
    K = E.K
    k = 0x80FF00017F << 200 | 0xFF01
    for n in (K - 1, K, K + 1):
        points = [pts[i % 5] for i in range(n)]
        total = None
        for p in points:
            total = O.g1_add(total, p)
        rc, sums, info = msm(points, [[k] * n, [1] * n])
        assert rc == 0 and sums == [O.g1_mul(total, k % O.R), total], n
        assert info[1] == n * nonzero_digits(k) + n and info[0] == (1 if n <= K else 2)
        assert info[2] == (nonzero_digits(k) + 1) * -(-n // K)
    big = (1 << 256) - 1
    rc, sums, info = msm([pts[0], O.g1_neg(pts[0]), None], [[big, big, big], [0, 0, 0], [O.R, 0, 5]])
    assert rc == 0 and sums == [None, None, None] and info[1] == 64 + nonzero_digits(O.R)


# ---- the Python layer with a stub in place of the library ----------------------------------------------------------
class FakeLib:
    """bls_g1_msm's bookkeeping: an encoding starting 0xff is invalid, 0xfe is outside G1; row v's output is 48
    bytes of value v, so that the unpacking is visible"""

    def __init__(self):
        self.calls, self.rc = [], None

    def bls_g1_msm(self, h, pts, n, rows, B, sg, out):
        self.calls.append((bytes(pts), n, bytes(rows), B, sg))
        if self.rc is not None:
            return self.rc
        if any(pts[48 * i] == 0xFF or (sg and pts[48 * i] == 0xFE) for i in range(n)):
            return 0
        ctypes.memmove(out, b"".join(bytes([v]) * 48 for v in range(B)), 48 * B)
        return 1

    def bls_g1_msm_stats(self, h, calls, entries):
        calls._obj.value, entries._obj.value = len(self.calls), 7
        return 0


class FakeCtx:
    def __init__(self):
        self.lib, self.h = FakeLib(), None

    def check(self, rc):
        if rc < 0:
            raise RuntimeError("device error %d" % rc)
        return rc


def _pt(i, first=0x80):
    return bytes([first]) + i.to_bytes(47, "big")


def test_python_argument_checks_packing_and_errors():
    from bls_mi355x import _native, batch

    ctx = FakeCtx()
    a, b = _pt(1), _pt(2)
    big = (1 << 256) - 1
    # rows are packed row-major, 32 big-endian bytes per scalar, as given: O.R + 3 is not reduced
    got = batch.g1_msm([a, b], [[1, big], [O.R + 3, 0]], ctx=ctx)
    assert got == [bytes(48), b"\x01" * 48]
    pts, n, rows, B, sg = ctx.lib.calls[-1]
    assert (pts, n, B, sg) == (a + b, 2, 2, 0)
    assert rows == E.k32(1) + E.k32(big) + E.k32(O.R + 3) + E.k32(0)
    batch.g1_msm((bytearray(a), memoryview(b)), iter([(5, 6)]), subgroup_check=True, ctx=ctx)
    assert ctx.lib.calls[-1][3:] == (1, 1)
    assert batch.g1_msm_stats(ctx) == (2, 7)
    ncalls = len(ctx.lib.calls)
    for bad_pts, bad_rows in (([], [[]]), ([], []), ([a], []), ([a, b], [[1]]), ([a], [[1, 2]]), ([a], [[-1]]),
                              ([a], [[1 << 256]]), ([a[:47]], [[1]]), ([a, b], [[1, 2], [3]])):
        with pytest.raises(ValueError):
            batch.g1_msm(bad_pts, bad_rows, ctx=ctx)
    assert len(ctx.lib.calls) == ncalls  # refused before the library is called
    # error mapping: 0 -> invalid encoding, BLS_E_ARG -> too much for one call, other negatives go through check()
    with pytest.raises(ValueError, match="invalid"):
        batch.g1_msm([a, _pt(3, 0xFF)], [[1, 2]], ctx=ctx)
    assert batch.g1_msm([_pt(3, 0xFE)], [[1]], ctx=ctx) == [bytes(48)]
    with pytest.raises(ValueError, match="invalid"):
        batch.g1_msm([_pt(3, 0xFE)], [[1]], subgroup_check=True, ctx=ctx)
    ctx.lib.rc = _native.BLS_E_ARG
    with pytest.raises(ValueError, match="too many"):
        batch.g1_msm([a], [[1]], ctx=ctx)
    ctx.lib.rc = _native.BLS_E_DEVICE
    with pytest.raises(RuntimeError):
        batch.g1_msm([a], [[1]], ctx=ctx)
    assert "g1_multi_exp" in batch.g1_msm.__doc__ and "no reduction" in batch.g1_msm.__doc__


def test_header_declares_what_native_binds():
    import re

    from bls_mi355x import _native

    with open(os.path.join(ROOT, "include", "blsmi355x.h")) as fh:
        hdr = fh.read()
    for name in ("bls_g1_msm", "bls_g1_msm_stats"):
        m = re.search(r"^int %s\(([^;]*)\);" % name, hdr, re.M)
        assert m, name
        assert len(m.group(1).split(",")) == len(_native._SIGS[name][1]), name
        assert hasattr(_native.load_library(), name), name
