"""Inputs and independent expectations of the G1 transform tests (test_g1fft_host_cpu.py, test_gpu_cell_proofs.py):
small vectors of G1 points with their transforms as direct sums of the Python oracle's g1_mul / g1_add, and the
restatement of the transform's index and twiddle maps.  Everything is computed once per process."""
import functools
import random

from oracle import bls_oracle as O

import cell_inputs as C
import kzg_inputs as K

R = K.R


def w_n(n: int) -> int:
    """the n-th root of unity of the cell functions' domain: w^(8192 / n)"""
    return pow(C.W, C.EXT_N // n, R)


@functools.lru_cache(maxsize=None)
def vectors():
    """{n: [vector, ...]} of oracle points (None the identity): one vector for n = 2 and n = 8, three for n = 4, the
    second of which has the identity at both ends and the third only identities"""
    rng = random.Random(0x61FF7)
    g = O.G1_GEN

    def pts(n):
        return [O.g1_mul(g, rng.randrange(1, R)) for _ in range(n)]

    four = pts(4)
    return {2: [pts(2)], 4: [four, [None, four[1], four[0], None], [None] * 4], 8: [pts(7)[:3] + [None] + pts(4)]}


def direct(vec, inverse: bool):
    """[sum_i [w_n^(+-i k)] vec[i]] (times 1 / n for the inverse), k < n: oracle multiplications and additions"""
    n = len(vec)
    root = pow(w_n(n), -1, R) if inverse else w_n(n)
    scale = pow(n, -1, R) if inverse else 1
    out = []
    for k in range(n):
        acc = None
        for i, p in enumerate(vec):
            if p is not None:
                acc = O.g1_add(acc, O.g1_mul(p, pow(root, i * k, R) * scale % R))
        out.append(acc)
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """((n, inverse, [input vectors as lists of 48-byte encodings], [expected vectors]), ...)"""
    out = []
    for n, vecs in vectors().items():
        for inverse in (False, True):
            out.append((n, inverse, [[O.g1_compress(p) for p in v] for v in vecs],
                        [[O.g1_compress(p) for p in direct(v, inverse)] for v in vecs]))
    return tuple(out)


def stage_maps(logn: int):
    """per stage s and butterfly t < n / 2, block-major: (block m, i0, i1, forward and inverse index into the 8,192
    powers of w of the twiddle w_n^(+-brp_s(m) n / 2^(s + 1)))"""
    n = 1 << logn
    out = []
    for s in range(logn):
        half = n >> (s + 1)
        for m in range(1 << s):
            e = (C.brp_bits(m, s) if s else 0) * half * (C.EXT_N // n)
            for j in range(half):
                i0 = 2 * half * m + j
                out += [m, i0, i0 + half, e, (C.EXT_N - e) % C.EXT_N]
    return out


def twiddles(logn: int, inverse: bool):
    """the twiddle of every (stage, block), as integers"""
    n = 1 << logn
    root = pow(w_n(n), -1, R) if inverse else w_n(n)
    return [pow(root, (C.brp_bits(m, s) if s else 0) * (n >> (s + 1)), R) for s in range(logn) for m in range(1 << s)]
