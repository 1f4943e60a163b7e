"""The pair sum of the registry gather (csrc/bls_fq_g1.h: g1q_add_aff2 -- two affine keys summed in homogeneous
coordinates, x2 != x3) and the gather's loop step on it (acc = g1q_add(acc, g1q_add_aff2(a, b)), with the guard
that sends a pair with equal x through two g1q_add_aff) on the CPU: a stand-alone host program with the digit
form's column, value and subtraction checks compiled in (tests/hostcheck_g1pair), against the Python oracle,
against the formula restated as polynomials, and against g1q_add_aff applied twice.

Points travel as raw digit vectors (3 x 14 radix-2^29 digits of the Montgomery representation, R = 2^406), so the
tests choose the redundant form of every operand.  A failed check inside the program aborts it; the test then
fails on the missing reply.
"""
import os
import random
import struct
import subprocess

import pytest

from oracle import bls_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "hostcheck_g1pair")
EXE = os.path.join(DIR, "hostcheck_g1pair")
INC = os.path.join(os.path.dirname(HERE), "eth-consensus-specs_amd", "csrc")

P = O.P
MASK = 2 ** 29 - 1
RM = 2 ** 406
RINV = pow(RM, -1, P)
LD = 2 ** 29 + 2 ** 4  # the L-form digit bound of g1q_add's operands
AFF2, ADD, ADD_AFF, STEP, TWICE = 0, 1, 2, 3, 4
IDENTITY = (0, 1, 0)
ZERO3 = [[0] * 14] * 3


def dig(v):
    """the exact radix-2^29 digits of the integer v (digit 13 takes the rest)"""
    return [(v >> (29 * i)) & MASK for i in range(13)] + [v >> 377]


def val(d):
    return sum(x << (29 * i) for i, x in enumerate(d))


def enc(a, k=0):
    """digits of the field element a: its Montgomery representative plus k p"""
    return dig(a * RM % P + k * P)


def dec(d):
    return val(d) * RINV % P


def enc_pt(pt, k=(0, 0, 0)):
    return [enc(c, kk) for c, kk in zip(pt, k)]


def dec_pt(d):
    return tuple(dec(c) for c in d)


def aff(pt, k=(0, 0)):
    """an affine key as the program takes it: x, y (plus k p: N form allows one p) and an ignored z"""
    return [enc(pt[0], k[0]), enc(pt[1], k[1]), enc(1)]


class Harness:
    def __init__(self):
        deps = [os.path.join(DIR, f) for f in ("hostcheck_g1pair.cpp", "Makefile")]
        deps += [os.path.join(INC, f) for f in os.listdir(INC) if f.endswith(".h")]
        if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(d) for d in deps):
            subprocess.check_call(["make", "-C", DIR], timeout=2400)
        self.proc = subprocess.Popen([EXE], stdin=subprocess.PIPE, stdout=subprocess.PIPE)

    def call(self, op, p, q=ZERO3, s=ZERO3):
        """(digits, packed, fast): three digit vectors, the three canonical packed values as integers, and for
        STEP whether the pair sum ran (1) or the guard's two mixed additions (0)"""
        flat = [x for pt in (p, q, s) for c in pt for x in c]
        self.proc.stdin.write(struct.pack("<130I", op, 0, 0, 0, *flat))
        self.proc.stdin.flush()
        rep = self.proc.stdout.read(4 * 79)
        assert len(rep) == 4 * 79, "the checked host program stopped (a column, value or subtraction check failed)"
        w = struct.unpack("<79I", rep)
        digits = [list(w[14 * k: 14 * k + 14]) for k in range(3)]
        packed = [sum(x << (32 * i) for i, x in enumerate(w[42 + 12 * k: 54 + 12 * k])) for k in range(3)]
        # the output contract of all three formulas: N form (exact 29-bit digits, below 2p); fq_pack is canonical
        for k, d in enumerate(digits):
            assert val(d) < 2 * P and all(x <= MASK for x in d[:13]), (op, k, d)
            assert packed[k] == val(d) % P
        return digits, packed, w[78]

    def close(self):
        self.proc.stdin.close()
        assert self.proc.wait(timeout=60) == 0


@pytest.fixture(scope="module")
def hc():
    h = Harness()
    yield h
    h.close()


@pytest.fixture(scope="module")
def pool():
    """random points of G1 (affine), computed once"""
    rng = random.Random(0x9A12)
    base = [O.g1_mul(O.G1_GEN, rng.randrange(1, O.R)) for _ in range(6)]
    pts = list(base)
    while len(pts) < 48:  # distinct x: any two of them are a pair the pair sum takes
        q = O.g1_add(rng.choice(pts), rng.choice(base))
        if q is not None and all(q[0] != p[0] for p in pts):
            pts.append(q)
    return pts


def proj(a, z=1):
    return IDENTITY if a is None else (a[0] * z % P, a[1] * z % P, z % P)


def same_point(got, a):
    """the projective (X : Y : Z) is the affine point (None: the identity)"""
    X, Y, Z = got
    if a is None:
        return Z == 0 and Y != 0
    return Z != 0 and X == a[0] * Z % P and Y == a[1] * Z % P


def to_affine(packed):
    """canonical Montgomery (X, Y, Z) -> the affine point, None for the identity"""
    X, Y, Z = (c * RINV % P for c in packed)
    if Z == 0:
        assert Y != 0
        return None
    zi = pow(Z, -1, P)
    return (X * zi % P, Y * zi % P)


# the formulas as polynomials, independent of the code's operation order
def poly_aff2(x2, y2, x3, y3):
    H, R = x3 - x2, y3 - y2
    V = x2 * H * H
    W = R * R - H ** 3 - 2 * V
    return (H * W % P, (R * (V - W) - y2 * H ** 3) % P, H ** 3 % P)


def poly_add(p, q):
    X1, Y1, Z1 = p
    X2, Y2, Z2 = q
    xy, yz, xz = X1 * Y2 + X2 * Y1, Y1 * Z2 + Y2 * Z1, X1 * Z2 + X2 * Z1
    m, s = Y1 * Y2 - 12 * Z1 * Z2, Y1 * Y2 + 12 * Z1 * Z2
    return ((xy * m - 12 * yz * xz) % P, (m * s + 36 * X1 * X2 * xz) % P, (s * yz + 3 * X1 * X2 * xy) % P)


def worst(vbound, digit):
    """digits 0..12 all at `digit`, the top digit as large as a value below vbound p allows"""
    low = [digit] * 13
    top = (vbound * P - 1 - val(low + [0])) >> 377
    d = low + [top]
    assert (vbound - 1) * P < val(d) < vbound * P
    return d


def test_pair_sum_against_oracle(hc, pool):
    """g1q_add_aff2 on random pairs, canonical and with one p added to either coordinate (N form: below 2p)"""
    rng = random.Random(1)
    for i in range(80):
        a, b = rng.sample(pool, 2)
        d, packed, _ = hc.call(AFF2, aff(a, (i & 1, (i >> 1) & 1)), aff(b, ((i >> 2) & 1, (i >> 3) & 1)))
        assert same_point(dec_pt(d), O.g1_add(a, b)), i
        assert dec_pt(d) == poly_aff2(a[0], a[1], b[0], b[1])
        assert to_affine(packed) == O.g1_add(a, b)


def test_operands_at_the_n_form_bound(hc):
    """every digit of x2, y2, x3, y3 at 2^29 - 1 and every value just under 2p, and each operand alone at the
    bound against small ones: the 128-bit column checks hold and the result is the polynomial's.  (The formula is
    a polynomial identity, so the operands need not be curve points.)"""
    w = worst(2, MASK)
    lo = dig(1)
    for x2, y2, x3, y3 in ((w, w, w, w), (w, w, lo, lo), (lo, lo, w, w), (w, lo, lo, w), (lo, w, w, lo),
                           (enc(5), enc(7), w, w), (dig(0), dig(0), w, w), (w, w, dig(0), dig(0))):
        d, _, _ = hc.call(AFF2, [x2, y2, enc(1)], [x3, y3, enc(1)])
        assert dec_pt(d) == poly_aff2(dec(x2), dec(y2), dec(x3), dec(y3))


def test_outputs_are_operands_of_g1q_add(hc, pool):
    """the pair sum goes into g1q_add beside an accumulator at the top of its contract (X < 66p, Y, Z < 4p, every
    digit at 2^29 + 2^4), as the first and as the second operand, and beside another pair sum"""
    rng = random.Random(2)
    acc = [worst(66, LD), worst(4, LD), worst(4, LD)]
    w = worst(2, MASK)
    s_worst = hc.call(AFF2, [w, w, enc(1)], [dig(0), dig(0), enc(1)])[0]
    for i in range(12):
        a, b = rng.sample(pool, 2)
        s = s_worst if i == 0 else hc.call(AFF2, aff(a), aff(b))[0]
        for p, q in ((acc, s), (s, acc), (s, s)):
            d, _, _ = hc.call(ADD, p, q)
            assert dec_pt(d) == poly_add(dec_pt(p), dec_pt(q))
        # on a real accumulator: the point is the oracle's
        c = rng.choice(pool)
        z = rng.randrange(1, P)
        d, _, _ = hc.call(ADD, enc_pt(proj(c, z), (65, 3, 3)), hc.call(AFF2, aff(a), aff(b))[0])
        assert same_point(dec_pt(d), O.g1_add(c, O.g1_add(a, b)))


def test_chain_of_600_pair_steps(hc, pool):
    """600 chained steps acc = g1q_add(acc, g1q_add_aff2(a, b)) (longer than any lane's run), every output fed
    back as it came out and checked against the oracle; the chain doubles itself and passes through the identity"""
    rng = random.Random(3)
    acc, want = enc_pt(IDENTITY), None
    for i in range(600):
        a, b = rng.sample(pool, 2)
        if i == 300:  # a + b = want: the accumulator is doubled by the complete addition
            a = rng.choice([p for p in pool if p[0] != want[0]])
            b = O.g1_add(want, O.g1_neg(a))
        elif i == 400:  # a + b = -want: down to the identity
            a = rng.choice([p for p in pool if p[0] != want[0]])
            b = O.g1_add(O.g1_neg(want), O.g1_neg(a))
        assert a[0] != b[0]
        acc, _, fast = hc.call(STEP, acc, aff(a), aff(b))
        assert fast == 1
        want = O.g1_add(want, O.g1_add(a, b))
        assert same_point(dec_pt(acc), want), i
        if i == 400:
            assert want is None
    assert want is not None


def test_the_loops_guard(hc, pool):
    """a repeated key and a key beside its negation have equal x: the step takes two g1q_add_aff and its sum is
    right; the pair sum itself would not be a point / would be the identity there.  An accumulator that is the
    identity before a step, and one that is the identity after it, on both paths."""
    ident = enc_pt(IDENTITY)
    for n, a in enumerate(pool[:8]):
        na = O.g1_neg(a)
        c = pool[8 + n]
        z = (11 * a[0]) % P or 1
        for acc_pt in (None, c, a, na):
            acc = ident if acc_pt is None else enc_pt(proj(acc_pt, z), (65, 3, 3) if n % 2 else (0, 0, 0))
            # a repeated key (also with one copy redundant by p: the guard compares canonical limbs)
            for kb in ((0, 0), (1, 0)):
                d, _, fast = hc.call(STEP, acc, aff(a), aff(a, kb))
                assert fast == 0
                assert same_point(dec_pt(d), O.g1_add(acc_pt, O.g1_add(a, a)))
            # a key beside its negation, either order: the accumulator is unchanged
            for p, q in ((a, na), (na, a)):
                d, _, fast = hc.call(STEP, acc, aff(p), aff(q))
                assert fast == 0
                assert same_point(dec_pt(d), acc_pt)
        # the identity before a step (fast path), and after one: acc = -(a + c)
        d, _, fast = hc.call(STEP, ident, aff(a), aff(c))
        assert fast == 1 and same_point(dec_pt(d), O.g1_add(a, c))
        d2, _, fast = hc.call(STEP, enc_pt(proj(O.g1_neg(O.g1_add(a, c)), z)), aff(a), aff(c))
        assert fast == 1 and same_point(dec_pt(d2), None)
        # and the identity so reached is an accumulator like any other
        d3, _, fast = hc.call(STEP, d2, aff(c), aff(a))
        assert fast == 1 and same_point(dec_pt(d3), O.g1_add(a, c))
        # what the guard keeps out: the bare pair sum of equal x is (0 : 0 : 0) or (0 : Y : 0)
        assert dec_pt(hc.call(AFF2, aff(a), aff(a))[0]) == (0, 0, 0)
        X, Y, Z = dec_pt(hc.call(AFF2, aff(a), aff(na))[0])
        assert X == 0 and Z == 0 and Y != 0


def test_1000_steps_equal_two_mixed_additions(hc, pool):
    """1,000 inputs: the step's packed result, as an affine point, equals g1q_add_aff applied twice -- on
    accumulators in the redundant forms both leave, points with Z != 1, the identity, and pairs that take the
    guard (one in ten)"""
    rng = random.Random(4)
    accs = [enc_pt(IDENTITY)]
    accs += [enc_pt(proj(a, rng.randrange(1, P)), (rng.randrange(66), rng.randrange(4), rng.randrange(4)))
             for a in pool]
    n_fast = 0
    for i in range(1000):
        acc = rng.choice(accs)
        a, b = rng.sample(pool, 2)
        if i % 10 == 3:
            b = a if i % 20 == 3 else O.g1_neg(a)
        new = hc.call(STEP, acc, aff(a), aff(b))
        ref = hc.call(TWICE, acc, aff(a), aff(b))
        assert new[2] == (0 if i % 10 == 3 else 1)
        n_fast += new[2]
        assert to_affine(new[1]) == to_affine(ref[1]), i
        if i % 7 == 0:
            accs[rng.randrange(1, len(accs))] = new[0]
    assert n_fast == 900
