"""The complete G1 formulas with one reduction per output coordinate (csrc/bls_fq_g1.h: g1q_add_aff, g1q_add,
g1q_dbl) and the endomorphism chain on them (csrc/bls_g1_endo.h) on the CPU: a stand-alone host program with the
digit form's column, value and subtraction checks compiled in (tests/hostcheck_g1dot), against the Python oracle,
against the formulas restated as polynomials, and against the formulas as they stood before (kept in the harness).

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
DIR = os.path.join(HERE, "hostcheck_g1dot")
EXE = os.path.join(DIR, "hostcheck_g1dot")
INC = os.path.join(os.path.dirname(HERE), "eth-consensus-specs_amd", "csrc")

P = O.P
MASK = 2 ** 29 - 1
RM = 2 ** 406
RINV = pow(RM, -1, P)
LAMBDA = (-O.X * O.X) % O.R
LD = 2 ** 29 + 2 ** 4  # the L-form digit bound of the input contract
ADD_AFF, ADD, DBL, ENDO = 0, 1, 2, 3
IDENTITY = (0, 1, 0)


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


class Harness:
    def __init__(self):
        deps = [os.path.join(DIR, f) for f in ("hostcheck_g1dot.cpp", "Makefile")]
        deps += [os.path.join(INC, f) for f in os.listdir(INC) if f.endswith(".h")]
        if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(d) for d in deps):
            subprocess.check_call(["make", "-C", DIR], timeout=2400)
        self.proc = subprocess.Popen([EXE], stdin=subprocess.PIPE, stdout=subprocess.PIPE)

    def call(self, op, p, q=None, old=0, a=0, b=0):
        """(digits, packed): three digit vectors, and the three canonical packed values as integers"""
        q = q if q is not None else [[0] * 14] * 3
        flat = [x for c in p for x in c] + [x for c in q for x in c]
        self.proc.stdin.write(struct.pack("<88I", op, old, a, b, *flat))
        self.proc.stdin.flush()
        rep = self.proc.stdout.read(4 * 78)
        assert len(rep) == 4 * 78, "the checked host program stopped (a column, value or subtraction check failed)"
        w = struct.unpack("<78I", rep)
        digits = [list(w[14 * k: 14 * k + 14]) for k in range(3)]
        packed = [sum(x << (32 * i) for i, x in enumerate(w[42 + 12 * k: 54 + 12 * k])) for k in range(3)]
        return digits, packed

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
    rng = random.Random(0x61D07)
    base = [O.g1_mul(O.G1_GEN, rng.randrange(1, O.R)) for _ in range(6)]
    pts = list(base)
    while len(pts) < 48:
        pts.append(O.g1_add(rng.choice(pts), rng.choice(base)))
    return pts


def proj(aff, z=1):
    return IDENTITY if aff is None else (aff[0] * z % P, aff[1] * z % P, z % P)


def same_point(got, aff):
    """the projective (X : Y : Z) is the affine point (None: the identity)"""
    X, Y, Z = got
    if aff is None:
        return Z == 0 and Y != 0
    return Z != 0 and X == aff[0] * Z % P and Y == aff[1] * Z % P


def check_out(op, digits, packed):
    """the output contract: N form (exact 29-bit digits, below 2p), g1q_dbl's X below 4p with digits <= 2^29
    (g1q_mul_endo ends on a doubling when its last digit is zero); fq_pack is the canonical value"""
    for k, d in enumerate(digits):
        lim, top = (4, 2 ** 29) if (op in (DBL, ENDO) and k == 0) else (2, MASK)
        assert val(d) < lim * P and all(x <= top for x in d[:13]), (op, k, d)
        assert packed[k] == val(d) % P


# the formulas as polynomials (Renes-Costello-Batina, a = 0, b3 = 12), independent of the code's operation order
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


def run(hc, op, p, q=None, **kw):
    digits, packed = hc.call(op, p, q, **kw)
    if not kw.get("old"):
        check_out(op, digits, packed)
    return digits, packed


def test_random_points_against_oracle(hc, pool):
    """each of the three functions on random points, the accumulator with Z != 1 and with value-redundant
    coordinates (X + 65p, Y + 3p, Z + 3p: the top of the input contract)"""
    rng = random.Random(1)
    for i in range(60):
        a, b = rng.choice(pool), rng.choice(pool)
        z = rng.randrange(1, P)
        k = (65, 3, 3) if i % 2 else (0, 0, 0)
        acc = enc_pt(proj(a, z), k)
        d, _ = run(hc, ADD_AFF, acc, enc_pt(proj(b)))
        assert same_point(dec_pt(d), O.g1_add(a, b))
        z2 = rng.randrange(1, P)
        d, _ = run(hc, ADD, acc, enc_pt(proj(b, z2), (65, 65, 65) if i % 3 == 0 else (0, 0, 0)))
        assert same_point(dec_pt(d), O.g1_add(a, b))
        assert dec_pt(d) == poly_add(proj(a, z), proj(b, z2))
        d, _ = run(hc, DBL, enc_pt(proj(a, z), (65, 65, 65) if i % 2 else (0, 0, 0)))
        assert same_point(dec_pt(d), O.g1_add(a, a))
        assert dec_pt(d) == poly_dbl(proj(a, z))


def worst(vbound, digit):
    """digits 0..12 all at `digit`, the top digit as large as a value below vbound p allows"""
    low = [digit] * 13
    top = (vbound * P - 1 - val(low + [0])) >> 377
    d = low + [top]
    assert (vbound - 1) * P < val(d) < vbound * P
    return d


def test_operand_digits_at_the_declared_bound(hc):
    """every operand digit at its declared bound (2^29 + 2^4 for L-form inputs, 2^29 - 1 for the affine operand)
    and every value just under its bound: the 128-bit column checks hold and the result is the polynomial's.
    (The formulas are polynomial identities, so the operands need not be curve points.)"""
    acc = [worst(66, LD), worst(4, LD), worst(4, LD)]
    aff = [worst(2, MASK), worst(2, MASK), enc(1)]
    any66 = [worst(66, LD)] * 3
    for p in (acc, [worst(66, LD), dig(0), worst(4, LD)]):
        d, _ = run(hc, ADD_AFF, p, aff)
        assert dec_pt(d) == poly_add(dec_pt(p), (dec(aff[0]), dec(aff[1]), 1))
    for p, q in ((any66, any66), (acc, any66), (any66, [worst(2, MASK)] * 3)):
        d, _ = run(hc, ADD, p, q)
        assert dec_pt(d) == poly_add(dec_pt(p), dec_pt(q))
    for p in (any66, acc):
        d, _ = run(hc, DBL, p)
        assert dec_pt(d) == poly_dbl(dec_pt(p))


def test_degenerate_inputs(hc, pool):
    """the complete formulas have no exceptional case: identity + key, P + P, P + (-P), identity + identity,
    doubling the identity -- by every function that can express the case"""
    ident = enc_pt(IDENTITY)
    for a in pool[:6]:
        z = 7 * a[0] % P or 1
        pa, na = enc_pt(proj(a, z)), enc_pt(proj(O.g1_neg(a)))
        two_a = O.g1_add(a, a)
        # identity + key
        assert same_point(dec_pt(run(hc, ADD_AFF, ident, enc_pt(proj(a)))[0]), a)
        assert same_point(dec_pt(run(hc, ADD, ident, pa)[0]), a)
        assert same_point(dec_pt(run(hc, ADD, pa, ident)[0]), a)
        # P + P
        assert same_point(dec_pt(run(hc, ADD_AFF, pa, enc_pt(proj(a)))[0]), two_a)
        assert same_point(dec_pt(run(hc, ADD, pa, enc_pt(proj(a, 3)))[0]), two_a)
        # P + (-P)
        assert same_point(dec_pt(run(hc, ADD_AFF, pa, na)[0]), None)
        assert same_point(dec_pt(run(hc, ADD, pa, na)[0]), None)
        # the identity reached by cancellation is an operand like any other
        zero = run(hc, ADD, pa, na)[0]
        assert same_point(dec_pt(run(hc, ADD_AFF, zero, enc_pt(proj(a)))[0]), a)
        assert same_point(dec_pt(run(hc, DBL, zero)[0]), None)
    assert same_point(dec_pt(run(hc, ADD, ident, ident)[0]), None)
    assert same_point(dec_pt(run(hc, DBL, ident)[0]), None)


def test_chain_of_600_mixed_additions(hc, pool):
    """600 chained g1q_add_aff (longer than any lane's run), every output fed back as it came out and checked
    against the oracle; the chain passes through P + P and through the identity"""
    rng = random.Random(2)
    acc, want = enc_pt(IDENTITY), None
    for i in range(600):
        if i == 300:
            b = want  # P + P
        elif i == 400:
            b = O.g1_neg(want)  # down to the identity
        else:
            b = rng.choice(pool)
        acc, _ = run(hc, ADD_AFF, acc, enc_pt(proj(b)))
        want = O.g1_add(want, b)
        assert same_point(dec_pt(acc), want), i
    assert want is not None


def test_mul_endo_matches_oracle(hc, pool):
    """g1q_mul_endo(A, a, b) == [(a + b lambda) mod r] A on the formulas' new output forms"""
    rng = random.Random(3)
    m32 = 2 ** 32 - 1
    pairs = [(1, 0), (0, 1), (1, 1), (0, 0), (m32, m32), (2 ** 31, 2 ** 31), (0xAAAAAAAA, 0x55555555)]
    pairs += [(rng.getrandbits(32), rng.getrandbits(32)) for _ in range(8)]
    for j, (a, b) in enumerate(pairs):
        pt = None if j == 5 else pool[j]
        z = rng.randrange(2, P)
        d, _ = run(hc, ENDO, enc_pt(proj(pt, z), (3, 3, 3) if j % 2 else (0, 0, 0)), a=a, b=b)
        assert same_point(dec_pt(d), O.g1_mul(pt, (a + b * LAMBDA) % O.R)), (j, a, b)


def test_packed_outputs_equal_the_former_formulas(hc, pool):
    """1,000 random inputs: the packed X, Y, Z of each function equal those of the formulas before the change
    (namespace before of the harness), so everything downstream of fq_pack is unchanged bit for bit.  The inputs
    are accumulators in the redundant forms both versions produce, points with Z != 1 and the identity."""
    rng = random.Random(4)
    accs = [enc_pt(IDENTITY)]
    for i in range(40):  # accumulators as the former and the present formulas leave them
        accs.append(hc.call(ADD_AFF, rng.choice(accs), enc_pt(proj(rng.choice(pool))), old=i % 2)[0])
        accs.append(hc.call(DBL, rng.choice(accs), old=i % 2)[0])
    accs += [enc_pt(proj(a, rng.randrange(1, P)), (rng.randrange(66), rng.randrange(4), rng.randrange(4)))
             for a in pool]
    n = 0
    for i in range(1000):
        op = (ADD_AFF, ADD, DBL)[i % 3]
        p = rng.choice(accs)
        q = enc_pt(proj(rng.choice(pool))) if op == ADD_AFF else rng.choice(accs)
        new = run(hc, op, p, q)
        old = hc.call(op, p, q, old=1)
        assert new[1] == old[1], (i, op)
        if i % 7 == 0:
            accs[rng.randrange(1, len(accs))] = new[0]
        n += 1
    assert n == 1000
