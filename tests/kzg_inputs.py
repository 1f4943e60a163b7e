"""Inputs and expected values of the blob KZG tests (test_fr_cpu.py, test_kzg_cpu.py, test_gpu_kzg.py): the field
and the domain as Python integers, a restatement of the barycentric evaluation and of both quotient cases from the
mathematics, and known-answer blobs from low-degree polynomials whose commitments and proofs come from the monomial
setup with the oracle's G1 arithmetic -- independent of the barycentric formula and of the device.

  domain      w_i = omega^brp(i), omega = 7^((r - 1) / 4096), brp the 12-bit reversal
  evaluation  p(z) = f_m for z = w_m, else (z^4096 - 1) / 4096 * sum_i f_i w_i / (z - w_i)
  quotient    q_i = (f_i - y) / (w_i - z) for w_i != z; for z = w_m, q_m = sum_{i != m} (f_i - y) w_i / (z (z - w_i))
  known answers, p = sum_{k <= d} a_k X^k with d <= 65: the blob is p(w_i), the commitment sum a_k M[k], y is
  Horner at z, and the proof sum q_k M[k] with q the synthetic division of p - y by (X - z)
"""
import functools
import json
import os
import random

from oracle import bls_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
assert R == O.R
N = 4096
OMEGA = pow(7, (R - 1) // N, R)
IDENTITY48 = bytes([0xC0]) + bytes(47)
IN_DOMAIN_K = (0, 15, 16, 255, 256, 4095)  # both ends of a lane's run of 16 and of a workgroup's 256


def brp(i: int) -> int:
    return int(format(i, "012b")[::-1], 2)


DOMAIN = [pow(OMEGA, brp(i), R) for i in range(N)]
assert DOMAIN[1] == R - 1  # omega^2048


def fe(v: int) -> bytes:
    return (v % (1 << 256)).to_bytes(32, "big")


def blob_bytes(f) -> bytes:
    assert len(f) == N
    return b"".join(fe(v) for v in f)


def evaluate(f, z: int) -> int:
    z %= R
    for i, w in enumerate(DOMAIN):
        if w == z:
            return f[i] % R
    s = 0
    for fi, w in zip(f, DOMAIN):
        s += fi * w * pow(z - w, -1, R)
    return s % R * (pow(z, N, R) - 1) * pow(N, -1, R) % R


def quotient(f, z: int, y: int) -> list:
    z %= R
    q = [0] * N
    m = None
    for i, w in enumerate(DOMAIN):
        if w == z:
            m = i
        else:
            q[i] = (f[i] - y) * pow(w - z, -1, R) % R
    if m is not None:
        s = 0
        for i, w in enumerate(DOMAIN):
            if i != m:
                s += (f[i] - y) * w * pow(z * (z - w), -1, R)
        q[m] = s % R
    return q


@functools.lru_cache(maxsize=None)
def trusted_setup():
    """(g1_lagrange, g1_monomial[0..65], g2_monomial) of tests/golden/trusted_setup.json as bytes, in file order"""
    with open(os.path.join(HERE, "golden", "trusted_setup.json")) as fh:
        ts = json.load(fh)
    return tuple([bytes.fromhex(p[2:]) for p in ts[k]] for k in ("g1_lagrange", "g1_monomial", "g2_monomial"))


@functools.lru_cache(maxsize=None)
def monomial_points():
    return [O.g1_decompress(p) for p in trusted_setup()[1]]


def horner(coeffs, x: int) -> int:
    acc = 0
    for a in reversed(coeffs):
        acc = (acc * x + a) % R
    return acc


def poly_blob(coeffs) -> list:
    return [horner(coeffs, w) for w in DOMAIN]


def commit_monomial(coeffs) -> bytes:
    acc = None
    for a, m in zip(coeffs, monomial_points()):
        if a % R:
            acc = O.g1_add(acc, O.g1_mul(m, a % R))
    return O.g1_compress(acc)


def divide_out(coeffs, z: int):
    """(y, q) with p(X) - y = (X - z) q(X): synthetic division"""
    q = [0] * (len(coeffs) - 1)
    acc = 0
    for k in range(len(coeffs) - 1, 0, -1):
        acc = (acc * z + coeffs[k]) % R
        q[k - 1] = acc
    return (acc * z + coeffs[0]) % R, q


class KnownAnswer:
    """A polynomial's blob with its commitment, and (y, proof) at any z, all from the monomial setup"""

    def __init__(self, coeffs):
        self.coeffs = [a % R for a in coeffs]
        self.f = poly_blob(self.coeffs)
        self.blob = blob_bytes(self.f)
        self.commitment = commit_monomial(self.coeffs)

    @functools.lru_cache(maxsize=None)
    def open(self, z: int):
        y, q = divide_out(self.coeffs, z % R)
        return y, (commit_monomial(q) if q else IDENTITY48)


@functools.lru_cache(maxsize=None)
def known_answers():
    """degree 0 (a constant blob), degree 3 and degree 65 (the largest the fixture's monomial points reach)"""
    rng = random.Random(0x4B5A47)
    return (KnownAnswer([rng.randrange(R)]), KnownAnswer([rng.randrange(R) for _ in range(4)]),
            KnownAnswer([rng.randrange(R) for _ in range(66)]))


@functools.lru_cache(maxsize=None)
def linear_answers():
    """four polynomials p = a0 + a1 X as (a0, a1, commitment, proof): p(X) - p(z) = a1 (X - z), so the proof is
    [a1] M[0] whatever z is, and y = a0 + a1 z"""
    rng = random.Random(0x11EA12)
    out = []
    for _ in range(4):
        a0, a1 = rng.randrange(1, R), rng.randrange(1, R)
        out.append((a0, a1, commit_monomial([a0, a1]), commit_monomial([a1])))
    return tuple(out)


CUBIC_Z = (0x5EED, DOMAIN[15], 0, 3, DOMAIN[4095], R - 2, 1 << 200, 0xC0FFEE)


@functools.lru_cache(maxsize=None)
def cubic_openings():
    """eight openings (C, z, y, proof) of the degree-3 known answer, three oracle multiplications each"""
    a = known_answers()[1]
    return tuple((a.commitment, z) + a.open(z) for z in CUBIC_Z)


@functools.lru_cache(maxsize=None)
def batch_items(n: int, seed: int = 0xBA7C4):
    """n valid items (C, z, y, proof) at no oracle cost per item: the four linear polynomials in turn, each item
    with a random z of its own; every 16th item (i = 15 mod 16) one of the eight cubic openings; every 37th
    (i = 36 mod 37) the zero polynomial with the identity as commitment and as proof"""
    rng = random.Random(seed)
    lin, cub = linear_answers(), cubic_openings()
    out = []
    for i in range(n):
        z = rng.randrange(R)
        if i % 37 == 36:
            out.append((IDENTITY48, z, 0, IDENTITY48))
        elif i % 16 == 15:
            out.append(cub[(i // 16) % len(cub)])
        else:
            a0, a1, c, proof = lin[i % 4]
            out.append((c, z, (a0 + a1 * z) % R, proof))
    return tuple(out)


def random_blob(seed: int) -> list:
    rng = random.Random(seed)
    return [rng.randrange(R) for _ in range(N)]
