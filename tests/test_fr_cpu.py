"""Host side of the blob KZG functions: csrc/bls_fr.h (F_r in Montgomery form) and the lane pieces of
csrc/bls_kzg_blob.h in a host build (tests/hostcheck_fr), against Python integers and the restatement of
kzg_inputs.py.  Every case also goes, through a vector file, to the stand-alone build of the same source under
AddressSanitizer and UBSan, which the last test runs."""
import ctypes
import os
import random
import struct
import subprocess
import sys

import pytest

import kzg_inputs as K

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DIR = os.path.join(HERE, "hostcheck_fr")
LIB = os.path.join(DIR, "libhostcheck_fr.so")
SAN = os.path.join(DIR, "san_fr")
INC = os.path.join(ROOT, "eth-consensus-specs_amd", "csrc")

R = K.R
MONT = 1 << 256
OP_ADD, OP_SUB, OP_NEG, OP_MUL, OP_SQR, OP_INV, OP_POW, OP_REDUCE, OP_FROM = range(9)

_lib = None


def lib():
    global _lib
    if _lib is None:
        deps = [os.path.join(DIR, f) for f in ("hostcheck_fr.cpp", "Makefile")]
        deps += [os.path.join(INC, f) for f in ("bls_fr.h", "bls_fr_constants.h", "bls_kzg_blob.h", "bls_field_types.h")]
        newest = max(os.path.getmtime(d) for d in deps)
        if any(not os.path.exists(p) or os.path.getmtime(p) < newest for p in (LIB, SAN)):
            subprocess.check_call(["make", "-C", DIR], timeout=2400)
        _lib = ctypes.CDLL(LIB)
        _lib.hc_fr_op.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p]
        _lib.hc_kzb_blob.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p,
                                     ctypes.POINTER(ctypes.c_int)]
        _lib.hc_kzb_shape.restype = ctypes.c_uint32
    return _lib


def be(v):
    return v.to_bytes(32, "big")


def op(code, a=0, b=0, e=0):
    out = ctypes.create_string_buffer(32)
    rc = lib().hc_fr_op(code, be(a), be(b), e, out)
    return rc, int.from_bytes(out.raw, "big")


def expected(code, a, b, e):
    if code == OP_REDUCE:
        return 1, a % R
    if code == OP_FROM:
        return (1, a) if a < R else (0, 0)
    if a >= R or b >= R:
        return -1, None
    return 1, {
        OP_ADD: (a + b) % R, OP_SUB: (a - b) % R, OP_NEG: -a % R, OP_MUL: a * b % R, OP_SQR: a * a % R,
        OP_INV: pow(a, R - 2, R), OP_POW: pow(a, e, R),
    }[code]


def values():
    rng = random.Random(0xF2)
    return [0, 1, 2, R - 1, MONT % R, K.OMEGA, R - 2, (1 << 255) % R, (1 << 128) - 1] + [rng.randrange(R) for _ in range(12)]


def op_cases():
    vs = values()
    rng = random.Random(0xF3)
    cases = []
    for a in vs:
        for code in (OP_NEG, OP_SQR, OP_INV):
            cases.append((code, a, 0, 0))
        for e in (0, 1, 2, 4095, 4096, 0x80000000, 0xFFFFFFFF, rng.randrange(1 << 32)):
            cases.append((OP_POW, a, 0, e))
        for b in vs:
            for code in (OP_ADD, OP_SUB, OP_MUL):
                cases.append((code, a, b, 0))
    wide = [R - 1, R, R + 1, 1 << 255, (1 << 256) - 1, 2 * R, 2 * R - 1, 2 * R + 1, 0, 1]
    wide += [rng.randrange(1 << 256) for _ in range(20)]
    for a in wide:
        cases.append((OP_REDUCE, a, 0, 0))
        cases.append((OP_FROM, a, 0, 0))
    return cases


def test_every_operation_against_python_integers():
    for code, a, b, e in op_cases():
        rc, got = op(code, a, b, e)
        want_rc, want = expected(code, a, b, e)
        assert rc == want_rc and got == want, (code, hex(a), hex(b), e)


def test_from_be32_bounds():
    """< r is accepted; r, r + 1, 2^255 and 2^256 - 1 are refused and decode to zero"""
    assert op(OP_FROM, R - 1) == (1, R - 1)
    for v in (R, R + 1, 1 << 255, (1 << 256) - 1):
        assert op(OP_FROM, v) == (0, 0), hex(v)
    for v in (R, R + 1, (1 << 256) - 1):
        assert op(OP_REDUCE, v) == (1, v % R)
    assert op(OP_ADD, R, 0)[0] == -1  # the harness itself refuses a non-canonical operand


def test_inverse_of_zero_is_zero():
    """fr_inv is Fermat's a^(r - 2): documented as 0 for 0"""
    assert op(OP_INV, 0) == (1, 0)
    for a in values()[1:]:
        assert op(OP_MUL, a, op(OP_INV, a)[1]) == (1, 1)


def test_generated_constants():
    out = ctypes.create_string_buffer(192)
    lib().hc_fr_constants(out)
    got = [int.from_bytes(out.raw[32 * i: 32 * i + 32], "big") for i in range(6)]
    assert got[0] == R
    assert got[1] == MONT % R
    assert got[2] == MONT * MONT % R
    assert got[3] == pow(7, (R - 1) // 4096, R) == K.OMEGA
    assert got[4] == pow(4096, -1, R)
    assert got[5] == -pow(R, -1, 1 << 32) % (1 << 32)
    assert pow(got[3], 4096, R) == 1 and pow(got[3], 2048, R) == R - 1
    # the committed header is what the generator prints
    gen = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_fr_constants.py")], capture_output=True, text=True,
                         check=True).stdout
    with open(os.path.join(INC, "bls_fr_constants.h")) as fh:
        assert fh.read() == gen


def domain_bytes():
    return b"".join(be(w) for w in K.DOMAIN)


def test_domain_table():
    assert [lib().hc_kzb_shape(k) for k in range(3)] == [4096, 256, 16]
    out = ctypes.create_string_buffer(32 * K.N)
    lib().hc_kzb_domain(out)
    assert out.raw == domain_bytes()


def blob_cases():
    """(blob bytes, z) for a whole blob evaluated and divided: z random, 0, r - 1 (= omega^2048, domain index 1) and
    both ends of a lane's run and of the workgroup's 256; a low-degree blob as well as a random one"""
    f = K.random_blob(0xB10B)
    rng = random.Random(0xB10C)
    zs = [rng.randrange(R), 0, R - 1] + [K.DOMAIN[k] for k in K.IN_DOMAIN_K]
    cases = [(f, z) for z in zs]
    g = K.known_answers()[1].f
    cases += [(g, rng.randrange(R)), (g, K.DOMAIN[17]), ([0] * K.N, K.DOMAIN[4095]), ([0] * K.N, 5)]
    return cases


_expected_blobs = None


def expected_blobs():
    global _expected_blobs
    if _expected_blobs is None:
        out = []
        for f, z in blob_cases():
            y = K.evaluate(f, z)
            hit = K.DOMAIN.index(z) if z in K.DOMAIN else -1
            out.append((K.blob_bytes(f), be(z), 1, hit, be(y), b"".join(be(v) for v in K.quotient(f, z, y))))
        bad = list(K.random_blob(0xBAD))
        bad[77] = R  # refused, decoded as zero: the lane pieces then run on the blob with a zero there
        fz = bad[:77] + [0] + bad[78:]
        z = 12345
        y = K.evaluate(fz, z)
        out.append((K.blob_bytes(bad), be(z), 0, -1, be(y), b"".join(be(v) for v in K.quotient(fz, z, y))))
        _expected_blobs = out
    return _expected_blobs


def test_whole_blobs_lane_by_lane():
    assert R - 1 == K.DOMAIN[1]
    for n, (blob, z, want_rc, want_hit, y, q) in enumerate(expected_blobs()):
        got_y, got_q = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32 * K.N)
        hit = ctypes.c_int(-2)
        rc = lib().hc_kzb_blob(blob, z, got_y, got_q, ctypes.byref(hit))
        assert (rc, hit.value) == (want_rc, want_hit), n
        assert got_y.raw == y, n
        assert got_q.raw == q, n
    got_y, got_q = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32 * K.N)
    assert lib().hc_kzb_blob(expected_blobs()[0][0], be(R), got_y, got_q, ctypes.byref(ctypes.c_int())) == -1


def test_restatement_agrees_with_the_known_answers():
    """the barycentric restatement against Horner and synthetic division on a low-degree polynomial"""
    ka = K.known_answers()[1]
    for z in (987654321, K.DOMAIN[16], 0):
        y, q = K.divide_out(ka.coeffs, z)
        assert K.evaluate(ka.f, z) == y == K.horner(ka.coeffs, z)
        assert K.quotient(ka.f, z, y) == K.poly_blob(q)


def test_sanitizer_program_runs_the_same_cases(tmp_path):
    """the stand-alone ASan + UBSan build of hostcheck_fr.cpp over every case above"""
    lib()
    path = tmp_path / "fr_vectors.bin"
    ops = op_cases()
    with open(path, "wb") as fh:
        fh.write(struct.pack("<I", len(ops)))
        for code, a, b, e in ops:
            rc, want = expected(code, a, b, e)
            fh.write(struct.pack("<II", code, e) + be(a) + be(b) + struct.pack("<i", rc) + be(want or 0))
        fh.write(domain_bytes())
        blobs = expected_blobs()
        fh.write(struct.pack("<I", len(blobs)))
        for blob, z, rc, hit, y, q in blobs:
            fh.write(blob + z + struct.pack("<ii", rc, hit) + y + q)
    res = subprocess.run([SAN, str(path)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "hostcheck_fr: 0 mismatches" in res.stdout
