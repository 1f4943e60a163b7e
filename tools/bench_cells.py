#!/usr/bin/env python3
"""A/B of the device cell KZG functions (bls_mi355x.kzg_cells; bls_kzg_verify_cells, bls_kzg_compute_cells,
bls_kzg_recover_cells) against the same algorithms in Python integers around the project's existing device group
calls, on one MI355X in one process.  The baseline is FFT-based, not the spec's O(n^2) loops:

  verification  per cell the inverse 64-point FFT and the h_k^-m / 64 scaling; the column sums s_m = sum r_k c_{k,m},
                the commitments' weights; sum r_k pi_k and sum w_i C_i + sum r_k h_k^64 pi_k as one
                multi-exponentiation each, sum s_m [tau^m] G1 on the resident G1 table, one pairing check
  cells         inverse FFT of the blob (4,096), FFT of the zero-padded coefficients (8,192)
  recovery      recover_polynomialcoeff with 8,192-point FFTs, then the extension

The items are valid: polynomials of degree 65, whose commitments and proofs the 66 monomial points of the fixture
reach ([q(tau)]_1 with q = a_64 + a_65 X is the proof of every cell of such a polynomial).

Every shape runs both forms on the same inputs, alternating per repetition: one warm-up call per form, then `--reps`
timed windows, the device synchronised around every window (wall clock: ctypes and copies included).  One JSON line
per shape and form: median, min and max ms per call over the windows, and baseline / form.  The results of every
timed call are compared with the baseline's.  No ratio is asserted: the lines are the result.

Shapes: verification of 128, 768 (6 blobs x 128) and 8,192 cells; compute_cells of 1, 6 and 64 blobs; recovery of 1
and 6 blobs with the odd cells missing.  `--only-verify N --calls K` runs K verifications of N cells and nothing
else: the workload for a kernel-trace profiler, which gives the per-kernel split."""
from __future__ import annotations

import argparse
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "eth-consensus-specs_amd"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from bench_kzg import G2_GEN, R, _line, _timed, run_shape  # noqa: E402

N, EXT_N, CELL, CELLS = 4096, 8192, 64, 128
W = pow(7, (R - 1) // EXT_N, R)


def brp_bits(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2)


BRP6 = [brp_bits(i, 6) for i in range(64)]
BRP7 = [brp_bits(i, 7) for i in range(128)]
BRP12 = [brp_bits(i, 12) for i in range(N)]
BRP13 = [brp_bits(i, 13) for i in range(EXT_N)]


def fft(vals, root):
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


def ints(raw):
    return [int.from_bytes(raw[i: i + 32], "big") for i in range(0, len(raw), 32)]


def cells_bytes(ext):
    return [b"".join(v.to_bytes(32, "big") for v in ext[CELL * k: CELL * k + CELL]) for k in range(CELLS)]


def extend_int(coeffs):
    nat = fft(list(coeffs) + [0] * (EXT_N - len(coeffs)), W)
    return [nat[BRP13[i]] for i in range(EXT_N)]


def compute_cells_int(blob):
    f = ints(blob)
    coeffs = ifft([f[BRP12[i]] for i in range(N)], W * W % R)
    return cells_bytes(extend_int(coeffs))


def recover_int(idx, cells):
    """recover_polynomialcoeff with FFTs, then the extension; the vanishing polynomial is built as the spec builds it"""
    ext_rbo = [0] * EXT_N
    for k, c in zip(idx, cells):
        ext_rbo[CELL * k: CELL * k + CELL] = ints(c)
    ext = [ext_rbo[BRP13[i]] for i in range(EXT_N)]
    w128 = pow(W, 64, R)
    short = [1]
    for k in range(CELLS):
        if k in idx:
            continue
        root = pow(w128, BRP7[k], R)
        nxt = [0] * (len(short) + 1)
        for i, a in enumerate(short):
            nxt[i + 1] = (nxt[i + 1] + a) % R
            nxt[i] = (nxt[i] - a * root) % R
        short = nxt
    zero = [0] * EXT_N
    for i, a in enumerate(short):
        zero[CELL * i] = a
    z_eval = fft(zero, W)
    ez = ifft([a * b % R for a, b in zip(z_eval, ext)], W)
    p7 = [1] * EXT_N
    for i in range(1, EXT_N):
        p7[i] = p7[i - 1] * 7 % R
    ez_coset = fft([a * s % R for a, s in zip(ez, p7)], W)
    z_coset = fft([a * s % R for a, s in zip(zero, p7)], W)
    p_coset = [a * pow(b, -1, R) % R for a, b in zip(ez_coset, z_coset)]
    inv7 = pow(7, -1, R)
    coeffs, s = [], 1
    for a in ifft(p_coset, W)[:N]:
        coeffs.append(a * s % R)
        s = s * inv7 % R
    return cells_bytes(extend_int(coeffs))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5, help="timed windows per form (at least 5)")
    ap.add_argument("--max-blobs", type=int, default=64, help="largest shapes' blobs (64; smaller to rehearse)")
    ap.add_argument("--only-verify", type=int, default=0, help="run only verifications of this many cells")
    ap.add_argument("--calls", type=int, default=5, help="... this many times")
    args = ap.parse_args()
    reps = max(5, args.reps)
    from bls_mi355x import _native, batch, kzg_cells

    with open(os.path.join(ROOT, "tests", "golden", "trusted_setup.json")) as fh:
        ts = json.load(fh)
    M = [bytes.fromhex(h[2:]) for h in ts["g1_monomial"]]
    tau64_g2 = bytes.fromhex(ts["g2_monomial"][64][2:])
    ctx = _native.context()
    table = batch.G1Table(ctx)
    assert table.load(M, subgroup_check=True).all()
    from bls_mi355x import curve
    curve.use_g1_table(table)
    ms, S = _timed(ctx, lambda: kzg_cells.CellSetup(ctx, M[:64], tau64_g2))
    _line(shape="setup: 64 monomial points found in the table, [tau^64] G2, the transform's tables", ms=round(ms, 3))
    import ctypes
    neg = ctypes.create_string_buffer(96)
    assert ctx.lib.bls_point_neg(ctx.h, 2, tau64_g2, neg) == 1
    neg_tau64 = neg.raw
    idx66 = np.arange(66, dtype=np.uint32)
    idx64 = np.arange(64, dtype=np.uint32)

    rng = random.Random(0xCE11B)
    n_blobs = max(6, args.max_blobs)
    polys = [[rng.randrange(R) for _ in range(66)] for _ in range(n_blobs)]
    blobs = []
    for a in polys:
        nat = fft(a + [0] * (N - 66), W * W % R)
        blobs.append(b"".join(nat[BRP12[i]].to_bytes(32, "big") for i in range(N)))
    commitments = [batch.g1_lincomb_indexed(table, idx66, a) for a in polys]
    proofs = [batch.g1_lincomb_indexed(table, idx66[:2], a[64:]) for a in polys]
    all_cells = []
    for s in range(0, n_blobs, 64):
        all_cells += S.compute_cells_batch(blobs[s: s + 64])

    def items(n):
        """n items, column-major as the sidecars come: every blob's cell 0, then every blob's cell 1, ..."""
        nb = max(1, n // CELLS)
        out = [(commitments[b], k, all_cells[b][k], proofs[b]) for k in range(CELLS) for b in range(nb)]
        return [list(x) for x in zip(*out[:n])]

    if args.only_verify:
        cm, ci, ce, pf = items(args.only_verify)
        for _ in range(args.calls):
            assert S.verify_cell_kzg_proof_batch(cm, ci, ce, pf) is True
        ctx.check(ctx.lib.bls_sync(ctx.h))
        _line(shape="only-verify", cells=len(cm), calls=args.calls)
        return

    # -- verification
    inv64 = pow(64, -1, R)
    g_inv = pow(W, -128, R)

    def verify_int(cm, ci, ce, pf):
        distinct, cidx = kzg_cells.dedupe_commitments(cm)
        n = len(cm)
        r = [rng.randrange(1, 1 << 128) for _ in range(n)]
        s = [0] * CELL
        for k in range(n):
            e = ints(ce[k])
            c = fft([e[BRP6[i]] for i in range(CELL)], g_inv)
            hinv = pow(W, -BRP7[ci[k]], R)
            sc = r[k] * inv64 % R
            for m in range(CELL):
                s[m] = (s[m] + sc * c[m]) % R
                sc = sc * hinv % R
        wts = [0] * len(distinct)
        for k in range(n):
            wts[cidx[k]] = (wts[cidx[k]] + r[k]) % R
        ll = batch.g1_multi_exp(pf, r)
        rli = batch.g1_lincomb_indexed(table, idx64, [-v % R for v in s])
        h64 = [pow(W, 64 * BRP7[k], R) for k in ci]
        rl = batch.g1_multi_exp(list(distinct) + list(pf) + [rli],
                                wts + [ri * h % R for ri, h in zip(r, h64)] + [1])
        return bool(batch.pairing_check([(ll, neg_tau64), (rl, G2_GEN)]))

    shapes = [128, 768] + ([8192] if n_blobs >= 64 else [])
    for n in shapes:
        cm, ci, ce, pf = items(n)
        run_shape(ctx, "verify_cell_kzg_proof_batch, %d cells" % n, {
            "python ints + multi_exp + table MSM + pairing_check": lambda: verify_int(cm, ci, ce, pf),
            "bls_kzg_verify_cells": lambda: S.verify_cell_kzg_proof_batch(cm, ci, ce, pf)}, reps, 1)

    # -- cells
    for B in (1, 6, n_blobs if n_blobs >= 64 else 0):
        if not B:
            continue
        run_shape(ctx, "compute_cells, %d blob%s" % (B, "s" * (B > 1)), {
            "python ints": lambda B=B: [compute_cells_int(b) for b in blobs[:B]],
            "bls_kzg_compute_cells": lambda B=B: S.compute_cells_batch(blobs[:B])}, reps, 1)

    # -- recovery, the odd cells missing
    even = list(range(0, CELLS, 2))
    for B in (1, 6):
        given = [[all_cells[b][k] for k in even] for b in range(B)]
        run_shape(ctx, "recover_cells, %d blob%s, odd cells missing" % (B, "s" * (B > 1)), {
            "python ints": lambda given=given: [recover_int(even, g) for g in given],
            "bls_kzg_recover_cells": lambda given=given: S.recover_cells_batch(even, given)}, reps, 1)
    _line(shape="counters", g1_table_stats=batch.g1_table_stats(ctx))


if __name__ == "__main__":
    main()
