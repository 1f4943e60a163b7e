#!/usr/bin/env python3
"""A/B of the bucket MSM over a call's own G1 points (bls_g1_msm, batch.g1_msm) against the per-point chains of
bls_multi_exp on the same point and scalar bytes, on one MI355X in one process.

Every shape runs the forms on the same inputs, alternating per repetition: one warm-up call per form, then `--reps`
timed windows, the device synchronised around every window (wall clock: ctypes, copies and the decode of the points
included on both sides).  One JSON line per shape and form: median, min and max ms per call over the windows, and
baseline / form.  Every timed result is compared byte for byte with the baseline's.  No ratio is asserted: the lines
are the result (DESIGN.md sections 4.15 and 7).

Forms: `bls_multi_exp x B` is B calls of the C ABI, one per row, on prepacked bytes (the baseline); `bls_g1_msm` is
one call of the C ABI on the same prepacked bytes; `batch.g1_msm` is the Python entry on lists of ints, which packs
32 B n bytes per call.

Shapes: n in {64, 768, 4,096, 65,536} with B in {1, 2} rows of full-width scalars, and a row of 128-bit scalars at
n = 768.  The points are the 8,192 of the trusted-setup fixture, repeated in order where n is larger (a repeated
point lands in its first copy's buckets when their digits agree: the complete addition's doubling case, same cost)."""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "eth-consensus-specs_amd"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from bench_kzg import _line, run_shape  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5, help="timed windows per form (at least 5)")
    ap.add_argument("--max-n", type=int, default=65536, help="largest n (65,536; smaller to rehearse)")
    args = ap.parse_args()
    reps = max(5, args.reps)
    from bls_mi355x import _native, batch

    with open(os.path.join(ROOT, "tests", "golden", "trusted_setup.json")) as fh:
        ts = json.load(fh)
    fixture = [bytes.fromhex(h[2:]) for h in ts["g1_lagrange"] + ts["g1_monomial"]]
    ctx = _native.context()
    rng = random.Random(0x6A5B)

    def multi_exp_rows(pts, rows, n):
        out = ctypes.create_string_buffer(48)
        res = []
        for row in rows:
            assert ctx.check(ctx.lib.bls_multi_exp(ctx.h, 1, pts, row, n, 0, out)) == 1
            res.append(out.raw)
        return res

    def g1_msm_abi(pts, packed, n, B):
        out = ctypes.create_string_buffer(48 * B)
        assert ctx.check(ctx.lib.bls_g1_msm(ctx.h, pts, n, packed, B, 0, out)) == 1
        return [out.raw[48 * v: 48 * v + 48] for v in range(B)]

    shapes = [(n, B, 256) for n in (64, 768, 4096, 65536) for B in (1, 2)] + [(768, 1, 128)]
    for n, B, bits in shapes:
        if n > args.max_n:
            continue
        plist = [fixture[i % len(fixture)] for i in range(n)]
        pts = b"".join(plist)
        ints = [[rng.randrange(1 << bits) for _ in range(n)] for _ in range(B)]
        rows = [b"".join(k.to_bytes(32, "big") for k in row) for row in ints]
        packed = b"".join(rows)
        s0 = batch.g1_msm_stats(ctx)
        run_shape(ctx, "n = %d, B = %d, %d-bit scalars" % (n, B, bits), {
            "bls_multi_exp x B": lambda: multi_exp_rows(pts, rows, n),
            "bls_g1_msm": lambda: g1_msm_abi(pts, packed, n, B),
            "batch.g1_msm": lambda: batch.g1_msm(plist, ints, ctx=ctx)}, reps, 1)
        s1 = batch.g1_msm_stats(ctx)
        _line(shape="n = %d, B = %d, %d-bit scalars" % (n, B, bits), g1_msm_calls=s1[0] - s0[0],
              bucket_entries_per_call=(s1[1] - s0[1]) // (s1[0] - s0[0]))


if __name__ == "__main__":
    main()
