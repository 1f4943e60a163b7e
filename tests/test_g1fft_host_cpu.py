"""Host side of the G1 transform: csrc/bls_g1_fft.h (index maps, twiddle lookup, butterfly, stage, the inverse's
scaling and the cell proofs' row map) in a host build (tests/hostcheck_g1fft), against the restatement and the
oracle's direct sums of g1fft_inputs.py.  Every case also goes, through a vector file, to the stand-alone build of the
same source under AddressSanitizer and UBSan, which the last test runs as a child process."""
import ctypes
import functools
import os
import random
import struct
import subprocess

from oracle import bls_oracle as O

import cell_inputs as C
import g1fft_inputs as G
import kzg_inputs as K

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DIR = os.path.join(HERE, "hostcheck_g1fft")
LIB = os.path.join(DIR, "libhostcheck_g1fft.so")
SAN = os.path.join(DIR, "san_g1fft")
INC = os.path.join(ROOT, "eth-consensus-specs_amd", "csrc")

R = K.R
LOGS = (1, 3, 7, 12)  # n = 2, 8, 128 and 4,096

_lib = None


def lib():
    global _lib
    if _lib is None:
        deps = [os.path.join(DIR, f) for f in ("hostcheck_g1fft.cpp", "Makefile")]
        deps += [os.path.join(INC, f) for f in os.listdir(INC) if f.endswith(".h")]
        newest = max(os.path.getmtime(d) for d in deps)
        if any(not os.path.exists(p) or os.path.getmtime(p) < newest for p in (LIB, SAN)):
            subprocess.check_call(["make", "-C", DIR], timeout=2400)
        _lib = ctypes.CDLL(LIB)
        _lib.hc_g1fft_maps_len.restype = ctypes.c_uint32
    return _lib


def out_order(logn):
    n = 1 << logn
    return [C.brp_bits(i, logn) for i in range(n)] + list(range(n))


def test_index_and_twiddle_maps_over_their_whole_ranges():
    for logn in LOGS:
        n = 1 << logn
        want = G.stage_maps(logn)
        assert lib().hc_g1fft_maps_len(logn) == len(want) == 5 * logn * n // 2
        out = (ctypes.c_uint32 * len(want))()
        lib().hc_g1fft_maps(logn, out)
        assert list(out) == want, logn
        order = (ctypes.c_uint32 * (2 * n))()
        lib().hc_g1fft_out_index(logn, order)
        assert list(order) == out_order(logn), logn
        # every stage pairs every entry exactly once
        for s in range(logn):
            rows = [want[5 * (s * n // 2 + t): 5 * (s * n // 2 + t) + 5] for t in range(n // 2)]
            assert sorted(i for r in rows for i in r[1:3]) == list(range(n)), (logn, s)


def twiddle_bytes(logn, inverse):
    return b"".join(v.to_bytes(32, "big") for v in G.twiddles(logn, inverse))


def test_twiddles_out_of_montgomery_form():
    for logn in LOGS:
        for inverse in (0, 1):
            out = ctypes.create_string_buffer(32 * ((1 << logn) - 1))
            lib().hc_g1fft_twiddles(logn, inverse, out)
            assert out.raw == twiddle_bytes(logn, bool(inverse)), (logn, inverse)
    # a twiddle is 1 exactly in block 0
    assert [i for i, v in enumerate(G.twiddles(7, False)) if v == 1] == [(1 << s) - 1 for s in range(7)]


def run(logn, inverse, natural, pts):
    out = ctypes.create_string_buffer(48 << logn)
    assert lib().hc_g1fft(logn, 1 if inverse else 0, 1 if natural else 0, b"".join(pts), out) == 1
    return [out.raw[48 * i: 48 * i + 48] for i in range(1 << logn)]


def test_small_transforms_against_the_oracles_direct_sums():
    seen = set()
    for n, inverse, vecs, wants in G.cases():
        logn = n.bit_length() - 1
        for v, (vec, want) in enumerate(zip(vecs, wants)):
            assert run(logn, inverse, True, vec) == want, (n, inverse, v)
            assert run(logn, inverse, False, vec) == [want[C.brp_bits(i, logn)] for i in range(n)], (n, inverse, v)
        seen.add(n)
    assert {2, 8} <= seen


def walk(n, seed):
    """n distinct G1 points at two oracle multiplications: S + i T"""
    rng = random.Random(seed)
    p, step = O.g1_mul(O.G1_GEN, rng.randrange(1, R)), O.g1_mul(O.G1_GEN, rng.randrange(1, R))
    out = []
    for _ in range(n):
        out.append(O.g1_compress(p))
        p = O.g1_add(p, step)
    return out


@functools.lru_cache(maxsize=None)
def half_case():
    """128 points of which the upper 64 are the identity (the cell proofs' shape), and their transform as the host
    arithmetic's direct sum"""
    pts = walk(64, 0x128A) + [K.IDENTITY48] * 64
    out = ctypes.create_string_buffer(48 * 128)
    assert lib().hc_g1fft_direct(7, b"".join(pts), out) == 1
    return pts, [out.raw[48 * i: 48 * i + 48] for i in range(128)]


@functools.lru_cache(maxsize=None)
def mixed_case():
    """128 points with the identity mixed in: at both ends, at a run in the middle and at every 9th place"""
    pts = walk(128, 0x128B)
    for i in [0, 127] + list(range(60, 70)) + list(range(4, 128, 9)):
        pts[i] = K.IDENTITY48
    return pts, run(7, False, True, pts)


def test_128_points_with_an_identity_upper_half_against_the_direct_sum():
    pts, want = half_case()
    assert len(set(want)) == 128 and K.IDENTITY48 not in want
    assert run(7, False, True, pts) == want
    # the transform's own output order is brp7: the cell proofs' order
    assert run(7, False, False, pts) == [want[C.brp_bits(i, 7)] for i in range(128)]
    # two of the outputs against the oracle: X[0] = the sum, X[64] = the alternating sum
    dec = [O.g1_decompress(p) for p in pts[:64]]
    s0 = s64 = None
    for i, p in enumerate(dec):
        s0 = O.g1_add(s0, p)
        s64 = O.g1_add(s64, p if i % 2 == 0 else O.g1_neg(p))
    assert want[0] == O.g1_compress(s0) and want[64] == O.g1_compress(s64)


def test_inverse_of_forward_is_the_identity_map_with_identities_mixed_in():
    pts, fwd = mixed_case()
    assert pts.count(K.IDENTITY48) >= 20
    assert run(7, True, True, fwd) == pts
    zero = [K.IDENTITY48] * 128
    assert run(7, False, True, zero) == zero and run(7, True, False, zero) == zero


GLV_L = 0xD201000000010000 ** 2 - 1  # x^2 - 1: L^2 + L + 1 = r, and [L] is the endomorphism's square


@functools.lru_cache(maxsize=None)
def product_cases():
    """(point, scalar, a, b, [scalar] point) with scalar = a + b L: edge scalars and random ones"""
    assert GLV_L * GLV_L + GLV_L + 1 == R
    rng = random.Random(0x61F)
    ks = [0, 1, 2, GLV_L - 1, GLV_L, GLV_L + 1, GLV_L * GLV_L, R - 1, R - 2, (1 << 128) - 1, 1 << 128,
          G.twiddles(7, False)[5]] + [rng.randrange(R) for _ in range(6)]
    pts = walk(len(ks), 0x61E)
    return [(p, k, k % GLV_L, k // GLV_L, O.g1_compress(O.g1_mul(O.g1_decompress(p), k))) for p, k in zip(pts, ks)]


def test_endomorphism_split_and_both_chains_against_the_oracle():
    for p, k, a, b, want in product_cases():
        assert a < 1 << 128 and b < 1 << 128
        ga, gb = ctypes.create_string_buffer(16), ctypes.create_string_buffer(16)
        lib().hc_g1fft_split(k.to_bytes(32, "big"), ga, gb)
        assert (int.from_bytes(ga.raw, "big"), int.from_bytes(gb.raw, "big")) == (a, b), hex(k)
        for glv in (0, 1):
            out = ctypes.create_string_buffer(48)
            assert lib().hc_g1fft_mul(glv, p, k.to_bytes(32, "big"), out) == 1
            assert out.raw == want, (hex(k), glv)
    out = ctypes.create_string_buffer(48)
    assert lib().hc_g1fft_mul(1, K.IDENTITY48, (R - 1).to_bytes(32, "big"), out) == 1 and out.raw == K.IDENTITY48


def test_invalid_encoding_is_refused():
    out = ctypes.create_string_buffer(96)
    assert lib().hc_g1fft(1, 0, 1, K.IDENTITY48 + bytes(48), out) == -1


def test_cell_proof_rows_shift_and_zero_fill():
    rng = random.Random(0x2035)
    coef = [rng.randrange(R) for _ in range(4096)]
    raw = b"".join(v.to_bytes(32, "big") for v in coef)
    for m in (0, 1, 31, 62):
        out = ctypes.create_string_buffer(32 * 4032)
        assert lib().hc_cellproof_row(raw, m, out) == 1
        got = [int.from_bytes(out.raw[32 * i: 32 * i + 32], "big") for i in range(4032)]
        assert got == (coef[64 * (m + 1):] + [0] * 4096)[:4032], m
    assert lib().hc_cellproof_row(raw, 63, ctypes.create_string_buffer(32 * 4032)) == -2
    assert sum(4096 - 64 * (m + 1) for m in range(63)) == 129024


def test_sanitizer_program_runs_the_same_cases(tmp_path):
    """the stand-alone ASan + UBSan build of hostcheck_g1fft.cpp over the cases above, as a child process"""
    lib()
    recs = []
    for logn in LOGS:
        want, order = G.stage_maps(logn), out_order(logn)
        recs.append(struct.pack("<II", 0, logn) + struct.pack("<%dI" % len(want), *want)
                    + struct.pack("<%dI" % len(order), *order))
        for inverse in (0, 1):
            recs.append(struct.pack("<III", 1, logn, inverse) + twiddle_bytes(logn, bool(inverse)))
    for n, inverse, vecs, wants in G.cases():
        for vec, want in zip(vecs, wants):
            recs.append(struct.pack("<IIII", 2, n.bit_length() - 1, int(inverse), 1) + b"".join(vec) + b"".join(want))
    pts, want = half_case()
    recs.append(struct.pack("<IIII", 2, 7, 0, 0) + b"".join(pts)
                + b"".join(want[C.brp_bits(i, 7)] for i in range(128)))
    pts, fwd = mixed_case()
    recs.append(struct.pack("<IIII", 2, 7, 0, 1) + b"".join(pts) + b"".join(fwd))
    recs.append(struct.pack("<IIII", 2, 7, 1, 1) + b"".join(fwd) + b"".join(pts))
    for p, k, a, b, want in product_cases():
        recs.append(struct.pack("<II", 3, 1) + p + k.to_bytes(32, "big") + a.to_bytes(16, "big")
                    + b.to_bytes(16, "big") + want)
    path = tmp_path / "g1fft_vectors.bin"
    with open(path, "wb") as fh:
        fh.write(struct.pack("<I", len(recs)))
        for r in recs:
            fh.write(r)
    res = subprocess.run([SAN, str(path)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "hostcheck_g1fft: 0 mismatches" in res.stdout
