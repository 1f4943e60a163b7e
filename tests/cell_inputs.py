"""Inputs and expected values of the cell KZG tests (test_cells_host_cpu.py, test_cells_cpu.py, test_gpu_cells.py): the
extended domain, a recursive radix-2 FFT on Python integers, the extension of a blob to its 128 cells, and a
restatement of the recovery of specs/fulu/polynomial-commitments-sampling.md (recover_polynomialcoeff) from its text.

  extended domain  EXT[i] = w^brp13(i), w = 7^((r - 1) / 8192); EXT[:4096] is the blob domain
  cell k           the evaluations at EXT[64 k : 64 k + 64] = h_k g^brp6(j), h_k = w^brp7(k), g = w^128
  extension        coefficients = inverse FFT of the blob in natural order; cells = FFT of the zero-padded
                   coefficients, in bit-reversed order
  recovery         E = the given cells (zero where missing), Z = the vanishing polynomial of the missing cosets;
                   (E Z) -> coefficients -> values on 7 x domain -> divided by Z there -> coefficients of P
"""
import functools
import random

import kzg_inputs as K

R = K.R
N = K.N
EXT_N = 8192
CELL = 64
CELLS = 128
BYTES_PER_CELL = 32 * CELL
W = pow(7, (R - 1) // EXT_N, R)
assert pow(W, 2, R) == K.OMEGA


def brp_bits(i: int, bits: int) -> int:
    return int(format(i, "0%db" % bits)[::-1], 2)


EXT = [pow(W, brp_bits(i, 13), R) for i in range(EXT_N)]
assert EXT[:N] == K.DOMAIN


def shift(k: int) -> int:
    """h_k: cell k's coset is h_k times the 64th roots of unity"""
    return pow(W, brp_bits(k, 7), R)


def fft(vals, root):
    """[sum_n vals[n] root^(n k)] for k < len(vals), a power of two of which root is a primitive root of unity"""
    n = len(vals)
    if n == 1:
        return list(vals)
    r2 = root * root % R
    even, odd = fft(vals[0::2], r2), fft(vals[1::2], r2)
    out = [0] * n
    w = 1
    for k in range(n // 2):
        t = w * odd[k] % R
        out[k] = (even[k] + t) % R
        out[k + n // 2] = (even[k] - t) % R
        w = w * root % R
    return out


def ifft(vals, root):
    n_inv = pow(len(vals), -1, R)
    return [v * n_inv % R for v in fft(vals, pow(root, -1, R))]


def root_of(n: int) -> int:
    return pow(7, (R - 1) // n, R)


def brp_list(seq):
    bits = len(seq).bit_length() - 1
    return [seq[brp_bits(i, bits)] for i in range(len(seq))]


def blob_coeffs(f):
    """the coefficients of the polynomial whose evaluations over K.DOMAIN are f"""
    return ifft(brp_list(list(f)), K.OMEGA)


def extend_coeffs(coeffs):
    """the 8,192 evaluations over EXT (the spec's order) of a polynomial of degree < 4,096"""
    return brp_list(fft(list(coeffs) + [0] * (EXT_N - len(coeffs)), W))


def extend(f):
    return extend_coeffs(blob_coeffs(f))


def cells_of(ext):
    """the 128 cells of an extended blob, as bytes"""
    return [b"".join(K.fe(v) for v in ext[CELL * k: CELL * k + CELL]) for k in range(CELLS)]


def vanishing_short(missing):
    """the coefficients (low first) of prod over missing k of (X - w_128^brp7(k))"""
    w128 = root_of(CELLS)
    poly = [1]
    for k in missing:
        root = pow(w128, brp_bits(k, 7), R)
        nxt = [0] * (len(poly) + 1)
        for i, a in enumerate(poly):
            nxt[i + 1] = (nxt[i + 1] + a) % R
            nxt[i] = (nxt[i] - a * root) % R
        poly = nxt
    return poly


def recover(cell_indices, cells):
    """recover_polynomialcoeff and the extension, on integers: cells is a list of lists of 64 integers; returns the
    8,192 values in the spec's order.  The transforms are the FFT above; every step is the spec's."""
    ext_rbo = [0] * EXT_N
    for k, cell in zip(cell_indices, cells):
        ext_rbo[CELL * k: CELL * k + CELL] = cell
    ext_nat = brp_list(ext_rbo)
    missing = [k for k in range(CELLS) if k not in set(cell_indices)]
    short = vanishing_short(missing)
    zero_poly = [0] * EXT_N
    for i, a in enumerate(short):
        zero_poly[i * CELL] = a
    z_eval = fft(zero_poly, W)
    ez = [a * b % R for a, b in zip(z_eval, ext_nat)]
    ez_coeffs = ifft(ez, W)

    def coset_fft(v):
        return fft([a * pow(7, i, R) % R for i, a in enumerate(v)], W)

    ez_coset = coset_fft(ez_coeffs)
    z_coset = coset_fft(zero_poly)
    p_coset = [a * pow(b, -1, R) % R for a, b in zip(ez_coset, z_coset)]
    inv7 = pow(7, -1, R)
    p_coeffs = [a * pow(inv7, i, R) % R for i, a in enumerate(ifft(p_coset, W))]
    return extend_coeffs(p_coeffs[:N])


def cell_ints(cell: bytes):
    return [int.from_bytes(cell[32 * j: 32 * j + 32], "big") for j in range(CELL)]


def missing_sets():
    """the missing-cell sets of the recovery tests, by name"""
    r64 = sorted(random.Random(0xCE11).sample(range(CELLS), 64))
    r17 = sorted(random.Random(0xCE12).sample(range(CELLS), 17))
    return {
        "none": [], "last": [127], "first_half": list(range(64)), "second_half": list(range(64, 128)),
        "even": list(range(0, 128, 2)), "odd": list(range(1, 128, 2)), "random_64": r64, "random_17": r17,
    }


@functools.lru_cache(maxsize=None)
def blobs():
    """(f, blob bytes, extension, cells) of a random blob, the zero blob and the degree-65 known answer"""
    out = []
    for f in (K.random_blob(0xCE77), [0] * N, K.known_answers()[2].f):
        ext = extend(f)
        out.append((f, K.blob_bytes(f), ext, cells_of(ext)))
    return tuple(out)


class CellAnswer:
    """A polynomial p = sum a_k X^k of degree <= 65 with its commitment, any of its cells and their proof, all from
    the monomial setup and independent of the device: p = I_k + (X^64 - h_k^64) q with q = a_64 + a_65 X for every
    cell k, so one proof [q(tau)]_1 serves all of p's cells (the identity for a degree below 64)"""

    def __init__(self, coeffs):
        self.coeffs = [a % R for a in coeffs]
        self.commitment = K.commit_monomial(self.coeffs)
        q = self.coeffs[CELL:]
        self.proof = K.commit_monomial(q) if any(q) else K.IDENTITY48

    @functools.lru_cache(maxsize=None)
    def cell(self, k: int) -> bytes:
        return b"".join(K.fe(K.horner(self.coeffs, x)) for x in EXT[CELL * k: CELL * k + CELL])

    def item(self, k: int):
        """(commitment, cell index, cell, proof)"""
        return self.commitment, k, self.cell(k), self.proof

    def interpolant(self, k: int):
        h64 = pow(shift(k), CELL, R)
        out = (self.coeffs + [0] * CELL)[:CELL]
        for i, a in enumerate(self.coeffs[CELL:]):
            out[i] = (out[i] + h64 * a) % R
        return out


@functools.lru_cache(maxsize=None)
def cell_answers():
    """degree 0, 63, 64 and 65 (the last is kzg_inputs' degree-65 known answer)"""
    rng = random.Random(0xCE115)
    return (CellAnswer([rng.randrange(R)]), CellAnswer([rng.randrange(R) for _ in range(64)]),
            CellAnswer([rng.randrange(R) for _ in range(65)]), CellAnswer(K.known_answers()[2].coeffs))


EDGE_CELLS = (0, 1, 63, 64, 127)


def batch_items(n: int):
    """n items mixing the four polynomials: the edge cell indices first, repeats of one index past 128 items"""
    ans = cell_answers()
    ks = list(EDGE_CELLS) + [k for k in range(CELLS) if k not in EDGE_CELLS]
    return [ans[i % 4].item(ks[(i // 4) % CELLS] if i < 4 * CELLS else 77) for i in range(n)]
