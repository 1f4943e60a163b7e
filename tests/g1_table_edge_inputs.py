"""Edge inputs of the resident G1 table tests (tests/test_g1_table_cpu.py, tests/test_gpu_g1_table.py): the run
length of the bucket fold, which tests/test_g1_table_cpu.py checks against the text of csrc/, the edge scalars and
the trusted-setup fixture's points with the root of unity that relates its two bases."""
import json
import os

from oracle import bls_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))

K = 16  # G1M_K (csrc/bls_g1_msm.h): entries per run of the bucket fold
WINDOWS = 32  # 8-bit windows of a 256-bit scalar

# digit 0 / 1 / 255 in every window, and the scalars around the window and group-order boundaries
EDGE_SCALARS = [0, 1, 2, 255, 256, 1 << 248, O.R - 1, O.R, 1 << 255, (1 << 256) - 1]
ONES = sum(1 << (8 * w) for w in range(WINDOWS))  # digit 1 in every window

G1_INF = b"\xc0" + bytes(47)


def k32(k: int) -> bytes:
    return int(k).to_bytes(32, "big")


def neg48(p48: bytes) -> bytes:
    """-P of a compressed non-identity point: the sign flag flipped"""
    return bytes([p48[0] ^ 0x20]) + p48[1:]


def trusted_setup():
    """(g1_lagrange, g1_monomial) of tests/golden/trusted_setup.json as 48-byte encodings, in file order"""
    with open(os.path.join(HERE, "golden", "trusted_setup.json")) as fh:
        ts = json.load(fh)
    return ([bytes.fromhex(h[2:]) for h in ts["g1_lagrange"]], [bytes.fromhex(h[2:]) for h in ts["g1_monomial"]])


def root_of_unity(n: int) -> int:
    """omega = 7^((r - 1) / n) mod r: sum_i omega^(i j) L[i] = M[j] for the fixture's Lagrange points L in file
    order and its monomial points M"""
    return pow(7, (O.R - 1) // n, O.R)


def bit_reverse(i: int, bits: int) -> int:
    return int(format(i, "0%db" % bits)[::-1], 2)
