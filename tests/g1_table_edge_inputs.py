"""Edge inputs of the resident G1 table tests (tests/test_g1_table_cpu.py, tests/test_gpu_g1_table.py): the run
length of the bucket fold, which tests/test_g1_table_cpu.py checks against the text of csrc/, the edge scalars and
the trusted-setup fixture's points with the root of unity that relates its two bases, and many-row calls with known
answers over a table of known discrete logarithms (tests/test_gpu_g1_table_rows.py)."""
import json
import os
import random

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


# ---- many rows with known answers ------------------------------------------------------------------------------------
# A table [G, [LOGS[1]] G, [LOGS[2]] G] whose discrete logarithms are known: a row of full-width scalars over the index
# list idx sums to [t] G when its last scalar is chosen as (t - sum of the others' k_i c_i) / c_last mod r.
LOGS = (1, 0x3A5F1C2B9D8E7F60112233445566778899AABBCCDDEEFF0123456789ABCDEF01 % O.R,
        0x5B6C7D8E9FA0B1C2D3E4F5061728394A5B6C7D8E9FA0B1C2D3E4F50617283949 % O.R)


def known_log_table():
    """the 48-byte encodings of [c] G for c in LOGS: two oracle multiplications"""
    return [O.g1_compress(O.g1_mul(O.G1_GEN, c)) for c in LOGS]


def rows_with_known_sums(B: int, idx, seed: int, zero_sum=(), empty=()):
    """(rows, want, nonzero_bytes) for a call of B rows over the index list idx into known_log_table(): row v sums
    to [v + 1] G, rows in zero_sum to the identity with non-zero scalars (t_v = 0), rows in empty are all zeros.
    want[v] is the row's 48 bytes, from running sums of G (one oracle addition per row); nonzero_bytes counts the
    non-zero bytes of all scalars, the bucket entries the call adds (every table point is a point)."""
    rng = random.Random(seed)
    logs = [LOGS[e] for e in idx]
    inv_last = pow(logs[-1], -1, O.R)
    zero_sum, empty = set(zero_sum), set(empty)
    assert not zero_sum & empty and all(0 <= v < B for v in zero_sum | empty)
    rows, want, nonzero = [], [], 0
    acc = None
    for v in range(B):
        acc = O.g1_add(acc, O.G1_GEN)  # [v + 1] G
        if v in empty:
            rows.append([0] * len(idx))
            want.append(G1_INF)
            continue
        t = 0 if v in zero_sum else v + 1
        ks = [rng.randrange(O.R) for _ in logs[:-1]]
        ks.append((t - sum(k * c for k, c in zip(ks, logs))) * inv_last % O.R)
        rows.append(ks)
        want.append(G1_INF if t == 0 else O.g1_compress(acc))
        nonzero += sum(1 for k in ks for b in k.to_bytes(32, "big") if b)
    return rows, want, nonzero
