"""The six-term dot product with one Montgomery reduction (csrc/bls_fq.h fq_mul_dot6) and the f accumulation's steps
built on it (csrc/bls_acc_dot.h: f x line and the Fp12 squaring as three dot6 per lane) on the CPU: a stand-alone
host program with the digit form's column checks (both accumulators, 128-bit), value checks and subtraction
preconditions compiled in (tests/hostcheck_accdot), against Python integers and the Python oracle's f12_mul.

Values travel as raw digit vectors (14 radix-2^29 digits of the Montgomery representation, R = 2^406), so the tests
choose the redundant form of every operand.  The program runs the four lanes (h, q) of one f one after another with
the kernels' exchanges as plain copies.  A failed check inside the program aborts it; the test then fails on the
missing reply.
"""
import os
import random
import struct
import subprocess

import pytest

from oracle import bls_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "hostcheck_accdot")
EXE = os.path.join(DIR, "hostcheck_accdot")
INC = os.path.join(os.path.dirname(HERE), "eth-consensus-specs_amd", "csrc")

P = O.P
MASK = 2 ** 29 - 1
RM = 2 ** 406
RINV = pow(RM, -1, P)
P29 = [(P >> (29 * i)) & MASK for i in range(13)] + [P >> 377]
LD = 2 ** 29 + 64           # L-form digit bound: the line records' l0 (ML_LD) and a prepared y operand (ACC_YD)
QF_V, QF_D = 11, 2 ** 29 + 5  # the loop-carried bound of f's halves (ML_QF_V, ML_QF_D: sqr_fin's output)
L0_V = 4096                 # ML_LV
R_OVER_P = RM // P
DOT6, LINE, SQR = 0, 1, 2
ZERO = [0] * 14


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


def worst(vbound, digit):
    """digits 0..12 all at `digit`, the top digit as large as a value below vbound p allows"""
    low = [digit] * 13
    top = (vbound * P - 1 - val(low + [0])) >> 377
    d = low + [top]
    assert (vbound - 1) * P < val(d) < vbound * P
    return d


def norm(d):
    """fq_norm: the carry-save normalisation"""
    return [d[0] & MASK] + [(d[i] & MASK) + (d[i - 1] >> 29) for i in range(1, 13)] + [d[13] + (d[12] >> 29)]


def k_for(vbound, dbound):
    """bls_fqb.h k_for: the smallest multiple c p in borrowed digits, each >= dbound, the top one covering vbound p"""
    c = 1
    while True:
        w = dig(c * P)
        e_prev, k, ok = 0, [], True
        for i in range(13):
            e = 0
            while w[i] + (e << 29) < dbound + e_prev:
                e += 1
            k.append(w[i] + (e << 29) - e_prev)
            e_prev = e
        if w[13] >= e_prev and w[13] - e_prev >= -(-vbound * 13002090 // 1000000):
            return k + [w[13] - e_prev]
        c += 1


class Harness:
    def __init__(self):
        deps = [os.path.join(DIR, f) for f in ("hostcheck_accdot.cpp", "Makefile")]
        deps += [os.path.join(INC, f) for f in os.listdir(INC) if f.endswith(".h")]
        if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(d) for d in deps):
            subprocess.check_call(["make", "-C", DIR], timeout=2400)
        self.proc = subprocess.Popen([EXE], stdin=subprocess.PIPE, stdout=subprocess.PIPE)

    def call(self, op, vecs):
        flat = [x for v in vecs for x in v]
        flat += [0] * (252 - len(flat))
        self.proc.stdin.write(struct.pack("<253I", op, *flat))
        self.proc.stdin.flush()
        rep = self.proc.stdout.read(4 * 168)
        assert len(rep) == 4 * 168, "the checked host program stopped (a column, value or input-bound check failed)"
        w = struct.unpack("<168I", rep)
        return [list(w[14 * k: 14 * k + 14]) for k in range(12)]

    def close(self):
        self.proc.stdin.close()
        assert self.proc.wait(timeout=60) == 0


@pytest.fixture(scope="module")
def hc():
    h = Harness()
    yield h
    h.close()


# ---- fq_mul_dot6 --------------------------------------------------------------------------------------------------
def dot6(hc, xs, ys):
    """runs the product and checks it: (sum x_t y_t) 2^-406 mod p, in N form (exact digits, below 2p)"""
    assert sum(val(x) * val(y) for x, y in zip(xs, ys)) < P * RM
    r = hc.call(DOT6, [v for x, y in zip(xs, ys) for v in (x, y)])[0]
    assert all(d <= MASK for d in r[:13]) and val(r) < 2 * P, r
    assert val(r) % P == sum(val(x) * val(y) for x, y in zip(xs, ys)) * RINV % P
    return r


def test_dot6_random_operands(hc):
    """random field elements in exact digits with values up to 11 p against up to 4096 p (f against a record)"""
    rng = random.Random(0xD076)
    for i in range(200):
        xs = [enc(rng.randrange(P), rng.randrange(QF_V - 1)) for _ in range(6)]
        ys = [enc(rng.randrange(P), rng.randrange(L0_V - 1) if i % 2 else 0) for _ in range(6)]
        dot6(hc, xs, ys)


def test_dot6_every_digit_at_its_declared_bound(hc):
    """x at the loop-carried bound of f (digits 2^29 + 5, value just under 11 p) and at a normalised sum's (digits
    2^29 + 1, just under 34 p: the squaring's X and Y), y at a prepared operand's bound (digits 2^29 + 64, just under
    8,200 p: a record's l0 and its negation): the fullest columns either accumulator sees"""
    for xv, xd in ((QF_V, QF_D), (34, 2 ** 29 + 2), (QF_V, LD)):
        x, y = worst(xv, xd), worst(2 * L0_V + 8, LD)
        dot6(hc, [x] * 6, [y] * 6)
        dot6(hc, [x] * 6, [y, worst(2, MASK), y, y, worst(2, MASK), y])


def test_dot6_negated_operand(hc):
    """y' = norm(K - y) for an N-form y and for a record's l0 (K = c p in borrowed digits, as bls_fqb.h neg): the
    product sum x y' is -x y, so x y + x y' = 0 and the mixed sums are the differences the Fp2 real part needs"""
    rng = random.Random(0xD077)
    for vb, db in ((2, MASK), (L0_V, LD)):
        K = k_for(vb, db)
        assert val(K) % P == 0 and all(k >= db for k in K[:13])
        for _ in range(40):
            a = [rng.randrange(P) for _ in range(6)]
            b = [rng.randrange(P) for _ in range(6)]
            xs = [enc(v, rng.randrange(QF_V - 1)) for v in a]
            ys = [enc(v, rng.randrange(vb - 1) if vb > 2 else 0) for v in b]
            ny = [norm([k - d for k, d in zip(K, y)]) for y in ys]
            assert all(max(n[:13]) <= LD for n in ny)
            # terms 3..5 negated: the second accumulator's streams, as the q = 0 lanes run them
            r = dot6(hc, xs, ys[:3] + ny[3:])
            want = (sum(a[t] * b[t] for t in range(3)) - sum(a[t] * b[t] for t in range(3, 6))) % P
            assert dec(r) == want
            # x y + x (-y) = 0 in every pair of terms
            r = dot6(hc, [xs[0], xs[1], xs[2], xs[0], xs[1], xs[2]], ys[:3] + ny[:3])
            assert val(r) % P == 0


def test_dot6_zero_pair_and_all_zero(hc):
    rng = random.Random(0xD078)
    xs = [enc(rng.randrange(P)) for _ in range(6)]
    ys = [enc(rng.randrange(P)) for _ in range(6)]
    for t in range(6):
        dot6(hc, xs[:t] + [ZERO] + xs[t + 1:], ys[:t] + [ZERO] + ys[t + 1:])
        dot6(hc, xs[:t] + [ZERO] + xs[t + 1:], ys)
    assert dot6(hc, [ZERO] * 6, [ZERO] * 6) == ZERO


def test_dot6_at_the_extreme_of_the_value_bound(hc):
    """sum V_x V_y at 41,288,643 of the 41,291,124 = floor(R / p) the static_assert allows, every operand just under its
    V p: the result is still below 2p"""
    vx, vy = [2623] * 6, [2623] * 5 + [2626]
    assert R_OVER_P - 3000 < sum(a * b for a, b in zip(vx, vy)) <= R_OVER_P
    for d in (MASK, 0):
        dot6(hc, [worst(v, d) for v in vx], [worst(v, d) for v in vy])
    dot6(hc, [dig(v * P - 1) for v in vx], [dig(v * P - 1) for v in vy])


# ---- the accumulation's steps ----------------------------------------------------------------------------------------
def enc2(c, k=(0, 0)):
    return [enc(c[0], k[0]), enc(c[1], k[1])]


def enc6(h, kmax=1, rng=None):
    return [v for c in h for v in enc2(c, (rng.randrange(kmax), rng.randrange(kmax)) if rng else (0, 0))]


def dec12(vecs):
    f = [dec(v) for v in vecs]
    return tuple(tuple((f[6 * h + 2 * k], f[6 * h + 2 * k + 1]) for k in range(3)) for h in range(2))


def check_f(vecs):
    """a step's output fits the loop-carried bound"""
    for v in vecs:
        assert all(d <= QF_D for d in v[:13]) and val(v) < QF_V * P, v


def line12(l0, l2, l3):
    return ((l0, l2, O.F2_ZERO), (O.F2_ZERO, l3, O.F2_ZERO))


def rand2(rng):
    return (rng.randrange(P), rng.randrange(P))


def rand12(rng):
    return tuple(tuple(rand2(rng) for _ in range(3)) for _ in range(2))


def step_line(hc, fd, l0, l2, l3, rng=None):
    """f (12 digit vectors) times the line; l0 goes in with a value up to 4,096 p, l2 and l3 in N form"""
    k0 = (rng.randrange(L0_V - 1), rng.randrange(L0_V - 1)) if rng else (0, 0)
    k1 = (rng.randrange(2), rng.randrange(2)) if rng else (0, 0)
    out = hc.call(LINE, fd + enc2(l0, k0) + enc2(l2, k1) + enc2(l3, k1[::-1]))
    check_f(out)
    assert all(d <= MASK for v in out for d in v[:13]) and all(val(v) < 2 * P for v in out)  # N form
    return out


def step_sqr(hc, fd):
    out = hc.call(SQR, fd)
    check_f(out)
    return out


def f_cases(rng):
    one = O.F12_ONE
    f = rand12(rng)
    return [("one", one), ("random", f), ("a = 0", (O.F6_ZERO, f[1])), ("b = 0", (f[0], O.F6_ZERO))]


def test_line_product_matches_the_oracle(hc):
    """f x ((l0, l2, 0) + (0, l3, 0) w) == f12_mul for f = 1, f random, f with a zero half; lines with l2 = 0, l3 = 0
    and neither; f's digits exact with values up to 10 p, and as the steps themselves leave them"""
    rng = random.Random(0xACC1)
    for name, f in f_cases(rng):
        for lname, (l0, l2, l3) in (("full", (rand2(rng), rand2(rng), rand2(rng))),
                                    ("l2 = 0", (rand2(rng), O.F2_ZERO, rand2(rng))),
                                    ("l3 = 0", (rand2(rng), rand2(rng), O.F2_ZERO)),
                                    ("l0 = 0", (O.F2_ZERO, rand2(rng), rand2(rng)))):
            want = O.f12_mul(f, line12(l0, l2, l3))
            for fd in (enc6(f[0]) + enc6(f[1]), enc6(f[0], QF_V - 1, rng) + enc6(f[1], QF_V - 1, rng)):
                assert dec12(step_line(hc, fd, l0, l2, l3, rng)) == want, (name, lname)
            fd = step_sqr(hc, step_line(hc, enc6(f[0]) + enc6(f[1]), (1, 0), O.F2_ZERO, O.F2_ZERO))
            f2 = O.f12_mul(f, f)
            assert dec12(step_line(hc, fd, l0, l2, l3, rng)) == O.f12_mul(f2, line12(l0, l2, l3)), (name, lname)


def test_squaring_matches_the_oracle(hc):
    rng = random.Random(0xACC2)
    for name, f in f_cases(rng):
        want = O.f12_mul(f, f)
        for fd in (enc6(f[0]) + enc6(f[1]), enc6(f[0], QF_V - 1, rng) + enc6(f[1], QF_V - 1, rng)):
            assert dec12(step_sqr(hc, fd)) == want, name
        assert dec12(step_sqr(hc, step_sqr(hc, enc6(f[0]) + enc6(f[1])))) == O.f12_mul(want, want), name


def test_steps_with_every_digit_at_the_loop_bound(hc):
    """f's twelve coefficients with every digit at ML_QF_D and the value just under ML_QF_V p, l0 at the record's
    bound (digits 2^29 + 64, just under 4,096 p), l2 and l3 at N form's: the column and value checks of all twelve
    dot6 hold and the results are the oracle's"""
    fd = [worst(QF_V, QF_D)] * 12
    f = dec12(fd)
    l0d, nd = [worst(L0_V, LD)] * 2, [worst(2, MASK)] * 2
    out = hc.call(LINE, fd + l0d + nd + nd)
    check_f(out)
    l0, l2 = (dec(l0d[0]), dec(l0d[1])), (dec(nd[0]), dec(nd[1]))
    assert dec12(out) == O.f12_mul(f, line12(l0, l2, l2))
    assert dec12(step_sqr(hc, fd)) == O.f12_mul(f, f)


def test_chain_of_70_alternating_steps(hc):
    """70 steps, squarings and line products in turn (the Miller loop has 63 + 68), every output fed back as it came
    out: each stays inside the declared loop bound -- the induction the kernels' relax calls encode -- and equals
    the oracle's product"""
    rng = random.Random(0xACC3)
    f = rand12(rng)
    fd = enc6(f[0], QF_V - 1, rng) + enc6(f[1], QF_V - 1, rng)
    for i in range(70):
        if i % 2 == 0:
            fd, f = step_sqr(hc, fd), O.f12_mul(f, f)
        else:
            l0, l2, l3 = rand2(rng), rand2(rng), rand2(rng)
            fd, f = step_line(hc, fd, l0, l2, l3, rng), O.f12_mul(f, line12(l0, l2, l3))
        assert dec12(fd) == f, i
    # and squarings alone, whose outputs are the widest values the loop carries
    for i in range(6):
        fd, f = step_sqr(hc, fd), O.f12_mul(f, f)
        assert dec12(fd) == f, i
