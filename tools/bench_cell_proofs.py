#!/usr/bin/env python3
"""Timing of the device cell proofs (bls_mi355x.kzg_cells.CellProofSetup; bls_kzg_compute_cells_and_proofs,
bls_kzg_recover_cells_and_proofs, bls_g1_fft) on one MI355X in one process, against the direct form as the library
could already do it without them:

  direct form   per blob and cell k the quotient of p by X^64 - a_k (synthetic division in Python integers, 4,032
                coefficients), the 128 quotients of a blob as 128 rows x 4,032 entries of `g1_lincomb_batch`'s call
                (bls_g1_table_msm) on the same table.  Its Python time (quotients and the rows' bytes) is measured
                once and reported apart; its device MSM time -- the fair comparison -- is timed over prepared rows.
  new call      63 rows x 4,032 entries per blob (a quarter of the bucket additions: the rows are zero-filled, and
                zero digits cost nothing), then one 128-point transform over G1 and one compression.

Per shape: one warm-up call per form, then `--reps` timed windows alternating between the forms, the device
synchronised around every window (wall clock: ctypes and copies included).  One JSON line per shape and form: median,
min and max ms per call.  The proofs of every timed call are compared with the direct form's.  No ratio is asserted:
the lines are the result.

Shapes: compute_cells_and_kzg_proofs_batch of 1, 6 and 64 blobs (the direct form at 1 and 6: its rows for 64 blobs
are a gigabyte of Python bytes), recovery of 6 blobs with the odd cells missing.  The split of the new call is
reported from calls of its parts on the same sizes: `bls_kzg_compute_cells` (the transforms over F_r, shared),
`bls_g1_fft` of B x 128 points (decode, the seven stages, the compression) and the remainder (the rows and their
MSM).  The setup's 4,096-point derivation (twelve stages) is timed once.  `--only-proofs B --calls K` runs K proof
calls of B blobs and nothing else: the workload for a kernel-trace profiler, which gives the per-kernel split."""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "eth-consensus-specs_amd"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from bench_cells import BRP7, BRP12, CELLS, N, W, ifft, ints  # noqa: E402
from bench_kzg import R, _line, _timed, run_shape  # noqa: E402

ROW_N = N - 64
MSM_ROWS = 511


def quotient_rows(blob: bytes) -> bytes:
    """the 128 quotients of one blob as bls_g1_table_msm's rows: 128 x 4,032 scalars of 32 bytes"""
    f = ints(blob)
    coeffs = ifft([f[BRP12[i]] for i in range(N)], W * W % R)
    rows = []
    for k in range(CELLS):
        a = pow(W, 64 * BRP7[k], R)
        q = [0] * N
        for i in range(ROW_N - 1, -1, -1):
            q[i] = (coeffs[i + 64] + a * q[i + 64]) % R
        rows.append(b"".join(v.to_bytes(32, "big") for v in q[:ROW_N]))
    return b"".join(rows)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5, help="timed windows per form (at least 5)")
    ap.add_argument("--max-blobs", type=int, default=64, help="the largest shape's blobs (64; smaller to rehearse)")
    ap.add_argument("--only-proofs", type=int, default=0, help="run only proof calls of this many blobs")
    ap.add_argument("--calls", type=int, default=5, help="... this many times")
    args = ap.parse_args()
    reps = max(5, args.reps)
    from bls_mi355x import _native, batch, kzg_cells

    with open(os.path.join(ROOT, "tests", "golden", "trusted_setup.json")) as fh:
        ts = json.load(fh)
    L = [bytes.fromhex(h[2:]) for h in ts["g1_lagrange"]]
    ctx = _native.context()
    ms, mono = _timed(ctx, lambda: kzg_cells.g1_monomial_from_lagrange(L, ctx))  # also the library's first calls
    ms, mono = _timed(ctx, lambda: kzg_cells.g1_monomial_from_lagrange(L, ctx))
    _line(shape="setup: 4,096 monomial points from the Lagrange points (decode, 12 stages, compression)",
          ms=round(ms, 3))
    ms, S = _timed(ctx, lambda: kzg_cells.CellProofSetup(ctx, g1_monomial=mono))
    _line(shape="setup: 4,096 points into a G1 table of their own (32 windows)", ms=round(ms, 3))
    idx = np.arange(S.first, S.first + ROW_N, dtype=np.uint32)

    rng = random.Random(0xCE11F)
    n_blobs = max(6, args.max_blobs)
    blobs = [b"".join(rng.randrange(R).to_bytes(32, "big") for _ in range(N)) for _ in range(n_blobs)]

    if args.only_proofs:
        for _ in range(args.calls):
            S.compute_cells_and_kzg_proofs_batch(blobs[:args.only_proofs])
        ctx.check(ctx.lib.bls_sync(ctx.h))
        _line(shape="only-proofs", blobs=args.only_proofs, calls=args.calls)
        return

    def direct_msm(rows: bytes, n_rows: int) -> list:
        """the prepared rows through bls_g1_table_msm, at most 511 per call"""
        out = []
        for s in range(0, n_rows, MSM_ROWS):
            c = min(MSM_ROWS, n_rows - s)
            o = ctypes.create_string_buffer(48 * c)
            rc = ctx.lib.bls_g1_table_msm(ctx.h, idx.ctypes.data_as(ctypes.c_void_p), ROW_N,
                                          rows[32 * ROW_N * s: 32 * ROW_N * (s + c)], c, o)
            assert ctx.check(rc) == 1
            out += [o.raw[48 * v: 48 * v + 48] for v in range(c)]
        return out

    def proofs_only(B):
        return [p for _, pf in S.compute_cells_and_kzg_proofs_batch(blobs[:B]) for p in pf]

    for B in (1, 6, n_blobs if n_blobs >= 64 else 0):
        if not B:
            continue
        name = "compute_cells_and_kzg_proofs, %d blob%s" % (B, "s" * (B > 1))
        forms = {}
        if B <= 6:
            t = time.perf_counter()
            rows = b"".join(quotient_rows(b) for b in blobs[:B])
            _line(shape=name, form="direct form, Python part (quotients, row bytes), once",
                  ms=round((time.perf_counter() - t) * 1e3, 1))
            forms["direct form, device part: bls_g1_table_msm of %d rows x 4,032" % (128 * B)] = (
                lambda rows=rows, B=B: direct_msm(rows, 128 * B))
        forms["bls_kzg_compute_cells_and_proofs"] = lambda B=B: proofs_only(B)
        run_shape(ctx, name, forms, reps, 1)
        # the split: the parts on the same sizes
        pts = proofs_only(B)
        parts = {
            "part: bls_kzg_compute_cells (F_r transforms, cells out)":
                lambda B=B: kzg_cells.compute_cells_batch(blobs[:B], ctx) and None,
            "part: bls_g1_fft of %d x 128 points (decode, 7 stages, compression)" % B:
                lambda B=B, pts=pts: batch.g1_fft([pts[128 * b: 128 * b + 128] for b in range(B)], ctx=ctx) and None,
        }
        med = {}
        for pname, fn in parts.items():
            fn()
            ts_ = [_timed(ctx, fn)[0] for _ in range(reps)]
            med[pname] = statistics.median(ts_)
            _line(shape=name, form=pname, ms_per_call_median=round(med[pname], 3), ms_min=round(min(ts_), 3),
                  ms_max=round(max(ts_), 3), reps=reps)
        whole = statistics.median([_timed(ctx, lambda B=B: proofs_only(B))[0] for _ in range(reps)])
        _line(shape=name, form="remainder: the 63 rows per blob and their table MSM (whole - parts)",
              ms=round(whole - sum(med.values()), 3), whole_ms=round(whole, 3))

    even = list(range(0, CELLS, 2))
    cells6 = [c for c, _ in S.compute_cells_and_kzg_proofs_batch(blobs[:6])]
    given = [[cells6[b][k] for k in even] for b in range(6)]
    run_shape(ctx, "recover_cells_and_kzg_proofs, 6 blobs, odd cells missing", {
        "bls_kzg_compute_cells_and_proofs on the blobs themselves": lambda: proofs_only(6),
        "bls_kzg_recover_cells_and_proofs":
            lambda: [p for _, pf in S.recover_cells_and_kzg_proofs_batch(even, given) for p in pf]}, reps, 1)
    _line(shape="counters", g1_table_stats=batch.g1_table_stats(ctx))


if __name__ == "__main__":
    main()
