"""Host side of the cell KZG functions: csrc/bls_fr_ntt.h (index maps, sub-transform, four-step transform, a cell's
interpolation polynomial, the recovery's vanishing polynomial) in a host build (tests/hostcheck_cells), against the
Python FFT and restatement of cell_inputs.py.  Every case also goes, through a vector file, to the stand-alone build
of the same source under AddressSanitizer and UBSan, which the last test runs."""
import ctypes
import functools
import os
import random
import struct
import subprocess

import cell_inputs as C
import kzg_inputs as K

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DIR = os.path.join(HERE, "hostcheck_cells")
LIB = os.path.join(DIR, "libhostcheck_cells.so")
SAN = os.path.join(DIR, "san_cells")
INC = os.path.join(ROOT, "eth-consensus-specs_amd", "csrc")

R = C.R
INV, SRC_BRP, DST_BRP = 1, 2, 4

_lib = None


def lib():
    global _lib
    if _lib is None:
        deps = [os.path.join(DIR, f) for f in ("hostcheck_cells.cpp", "Makefile")]
        deps += [os.path.join(INC, f) for f in ("bls_fr_ntt.h", "bls_fr.h", "bls_fr_constants.h", "bls_field_types.h")]
        newest = max(os.path.getmtime(d) for d in deps)
        if any(not os.path.exists(p) or os.path.getmtime(p) < newest for p in (LIB, SAN)):
            subprocess.check_call(["make", "-C", DIR], timeout=2400)
        _lib = ctypes.CDLL(LIB)
        _lib.hc_cells_maps_len.restype = ctypes.c_uint32
    return _lib


def be(v):
    return v.to_bytes(32, "big")


def pack(vals):
    return b"".join(be(v) for v in vals)


def unpack(raw):
    return [int.from_bytes(raw[i: i + 32], "big") for i in range(0, len(raw), 32)]


def want_maps():
    return [C.brp_bits(i, bits) for bits in (6, 7, 12, 13) for i in range(1 << bits)]


def test_index_maps_over_their_whole_ranges():
    n = lib().hc_cells_maps_len()
    assert n == 64 + 128 + 4096 + 8192
    out = (ctypes.c_uint32 * n)()
    lib().hc_cells_maps(out)
    assert list(out) == want_maps()


def test_generated_constants_and_tables():
    out = ctypes.create_string_buffer(256)
    lib().hc_cells_constants(out)
    got = unpack(out.raw)
    inv7 = pow(7, -1, R)
    assert got == [C.W, pow(64, -1, R), pow(8192, -1, R), 7, inv7, pow(C.W, 8191, R), pow(7, 8191, R),
                   pow(inv7, 8191, R)]
    assert pow(C.W, 8192, R) == 1 and pow(C.W, 4096, R) == R - 1


def inputs(n, seed):
    """random, all-zero, a single one at index 0 and at the last index"""
    rng = random.Random(seed)
    return [[rng.randrange(R) for _ in range(n)], [0] * n, [1] + [0] * (n - 1), [0] * (n - 1) + [1]]


@functools.lru_cache(maxsize=None)
def sub_cases():
    """(logl, inv, input bytes, expected bytes): the 64-point transform both ways (the inverse scaled) and the
    128-point sub-transform (unscaled, as the four-step's pass uses it)"""
    out = []
    for logl in (6, 7):
        n = 1 << logl
        root = C.root_of(n)
        for x in inputs(n, 0x5B + logl):
            out.append((logl, 0, pack(x), pack(C.fft(x, root))))
            inv = C.ifft(x, root) if logl == 6 else C.fft(x, pow(root, -1, R))
            out.append((logl, 1, pack(x), pack(inv)))
    return out


@functools.lru_cache(maxsize=None)
def four_step_cases():
    """(logn, flags, limit, input bytes, expected bytes): forward and inverse in natural order on every input kind;
    the two transforms of compute_cells with their bit reversals and zero padding; inverse of forward"""
    out = []
    for logn in (12, 13):
        n = 1 << logn
        root = C.root_of(n)
        for i, x in enumerate(inputs(n, 0x45 + logn)):
            f = C.fft(x, root)
            out.append((logn, 0, n, pack(x), pack(f)))
            out.append((logn, INV, n, pack(x), pack(C.ifft(x, root))))
            if i == 0:
                out.append((logn, INV, n, pack(f), pack(x)))  # inverse of forward = identity
    f, _, ext, _ = C.blobs()[0]
    coeffs = C.blob_coeffs(f)
    out.append((12, INV | SRC_BRP, 4096, pack(f), pack(coeffs)))
    rng = random.Random(0x9AD)
    padded = coeffs + [rng.randrange(R) for _ in range(4096)]  # what lies past the limit is read as zero
    out.append((13, DST_BRP, 4096, pack(padded), pack(ext)))
    return out


def test_sub_transforms_against_the_python_fft():
    for n, (logl, inv, x, want) in enumerate(sub_cases()):
        out = ctypes.create_string_buffer(len(x))
        assert lib().hc_ntt_sub(logl, inv, x, out) == 1
        assert out.raw == want, (n, logl, inv)


def test_four_step_transforms_against_the_python_fft():
    for n, (logn, flags, limit, x, want) in enumerate(four_step_cases()):
        out = ctypes.create_string_buffer(len(x))
        assert lib().hc_ntt(logn, flags, limit, x, out) == 1
        assert out.raw == want, (n, logn, flags)


def test_extension_restatement():
    """the extension's first half is the blob, and the degree-65 blob's extension is Horner on EXT"""
    for f, _, ext, _ in C.blobs():
        assert ext[:4096] == [v % R for v in f]
    ka = K.known_answers()[2]
    ext = C.blobs()[2][2]
    for i in (0, 1, 4095, 4096, 4097, 8191, 5000):
        assert ext[i] == K.horner(ka.coeffs, C.EXT[i])


@functools.lru_cache(maxsize=None)
def interp_cases():
    """(k, cell bytes, expected bytes): the degree-65 known answer's cells, whose interpolant is a[:64] with
    h^64 a_64 and h^64 a_65 added to its first two coefficients, and a random cell (checked by evaluation)"""
    a = K.known_answers()[2].coeffs
    ext = C.blobs()[2][2]
    out = []
    for k in (0, 1, 64, 127):
        h64 = pow(C.shift(k), 64, R)
        want = list(a[:64])
        want[0] = (want[0] + h64 * a[64]) % R
        want[1] = (want[1] + h64 * a[65]) % R
        out.append((k, pack(ext[64 * k: 64 * k + 64]), pack(want)))
    return out


def test_interpolation_coefficients_of_known_answer_cells():
    for k, cell, want in interp_cases():
        out = ctypes.create_string_buffer(2048)
        assert lib().hc_cells_interp(k, cell, out) == 1
        assert out.raw == want, k
        h = ctypes.create_string_buffer(32)
        lib().hc_cells_shift_pow64(k, h)
        assert int.from_bytes(h.raw, "big") == pow(C.shift(k), 64, R)
    rng = random.Random(0x1E7)
    cell = [rng.randrange(R) for _ in range(64)]
    out = ctypes.create_string_buffer(2048)
    assert lib().hc_cells_interp(77, pack(cell), out) == 1
    coeffs = unpack(out.raw)
    assert [K.horner(coeffs, x) for x in C.EXT[64 * 77: 64 * 78]] == cell


@functools.lru_cache(maxsize=None)
def vanish_cases():
    """(present flags, degree, coefficients, Z on the domain, 1 / Z on the coset) per missing set, the 128 values
    each being what the spec's 8,192-point transforms of the spread polynomial give at n = m (and at every
    n = m mod 128)"""
    out = []
    shift64 = pow(7, 64, R)
    w128 = C.root_of(128)
    for name, missing in C.missing_sets().items():
        short = C.vanishing_short(missing)
        present = bytes(0 if k in missing else 1 for k in range(128))
        zd = [K.horner(short, pow(w128, m, R)) for m in range(128)]
        zc = [K.horner(short, shift64 * pow(w128, m, R) % R) for m in range(128)]
        out.append((present, len(missing), pack(short + [0] * (129 - len(short))), pack(zd),
                    pack([pow(v, -1, R) for v in zc])))
    return out


def test_vanishing_polynomial_of_the_missing_sets():
    for n, (present, deg, coef, zd, zci) in enumerate(vanish_cases()):
        c, d, i = (ctypes.create_string_buffer(129 * 32), ctypes.create_string_buffer(128 * 32),
                   ctypes.create_string_buffer(128 * 32))
        assert lib().hc_cells_vanish(present, c, d, i) == deg
        assert c.raw == coef and d.raw == zd and i.raw == zci, n


def test_vanishing_values_are_the_spread_polynomials_transform():
    """Z(X) = S(X^64): the 8,192-point FFT of the spread coefficients repeats S on the 128th roots"""
    short = C.vanishing_short(C.missing_sets()["random_17"])
    spread = [0] * 8192
    for i, a in enumerate(short):
        spread[64 * i] = a
    full = C.fft(spread, C.W)
    w128 = C.root_of(128)
    assert full == [K.horner(short, pow(w128, n % 128, R)) for n in range(8192)]
    coset = C.fft([a * pow(7, i, R) % R for i, a in enumerate(spread)], C.W)
    s64 = pow(7, 64, R)
    assert coset[:300] == [K.horner(short, s64 * pow(w128, n % 128, R) % R) for n in range(300)]


def test_recovery_restatement_recovers_the_extension():
    """the restatement of the spec's recovery gives back the full extension for every missing set"""
    _, _, ext, _ = C.blobs()[0]
    for name, missing in C.missing_sets().items():
        idx = [k for k in range(128) if k not in missing]
        assert C.recover(idx, [ext[64 * k: 64 * k + 64] for k in idx]) == ext, name


def test_recovery_as_the_library_composes_it():
    """bls_kzg_recover_cells' sequence of pointwise steps and transforms on the host pieces gives the blob's
    coefficients, with the odd cells and with a random 17 missing"""
    f, _, ext, _ = C.blobs()[0]
    coeffs = pack(C.blob_coeffs(f))
    for name in ("odd", "random_17", "none"):
        missing = set(C.missing_sets()[name])
        present = bytes(0 if k in missing else 1 for k in range(128))
        given = [0 if (i // 64) in missing else v for i, v in enumerate(ext)]
        out = ctypes.create_string_buffer(32 * 4096)
        assert lib().hc_cells_recover(present, pack(given), out) == 1
        assert out.raw == coeffs, name


def test_sanitizer_program_runs_the_same_cases(tmp_path):
    """the stand-alone ASan + UBSan build of hostcheck_cells.cpp over every case above"""
    lib()
    path = tmp_path / "cells_vectors.bin"
    recs = [struct.pack("<I", 0) + struct.pack("<%dI" % len(want_maps()), *want_maps())]
    for logl, inv, x, want in sub_cases():
        recs.append(struct.pack("<III", 1, logl, inv) + x + want)
    for logn, flags, limit, x, want in four_step_cases():
        recs.append(struct.pack("<IIII", 2, logn, flags, limit) + x + want)
    for k, cell, want in interp_cases():
        recs.append(struct.pack("<II", 3, k) + cell + want)
    for present, deg, coef, zd, zci in vanish_cases():
        recs.append(struct.pack("<I", 4) + present + struct.pack("<i", deg) + coef + zd + zci)
    with open(path, "wb") as fh:
        fh.write(struct.pack("<I", len(recs)))
        for r in recs:
            fh.write(r)
    res = subprocess.run([SAN, str(path)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "hostcheck_cells: 0 mismatches" in res.stdout
