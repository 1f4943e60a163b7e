#!/usr/bin/env python3
"""Grouped signature aggregation (bls_aggregate_grouped) against the loop it replaces, on one MI355X, in one
process.  Two shapes -- 125,000 signatures in 2,048 groups and 16,384 signatures in 64 groups, members shuffled --
and three routes over the same groups:

  (a) host   the host-buffer call: signatures uploaded, 97 G bytes back
  (b) dev    bls_aggregate_grouped_dev on signatures resident in HBM
  (c) loop   one bls_aggregate per group (each group's signatures already contiguous on the host)

Inputs are seeded; one warm-up call per route, then `--reps` timed calls each (the loop: `--loop-reps`), the
device synchronised around every timed window.  The three routes' outputs are compared, and what must hold is
asserted: every repetition of (a) and of (b) is faster than the fastest repetition of (c).  Prints one JSON line.
`--only dev` runs route (b) alone (for a kernel trace)."""
from __future__ import annotations

import argparse
import ctypes
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "eth-consensus-specs_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

SHAPES = ((125000, 2048), (16384, 64))


def _timed(ctx, fn):
    ctx.check(ctx.lib.bls_sync(ctx.h))
    t = time.perf_counter()
    out = fn()
    ctx.check(ctx.lib.bls_sync(ctx.h))
    return (time.perf_counter() - t) * 1e3, out


def _stats(ts):
    return {"ms_median": round(statistics.median(ts), 3), "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3),
            "reps": len(ts)}


def run_shape(batch, ctx, B, G, reps, loop_reps, only):
    rng = np.random.default_rng(0xA66 + B)
    ids = (np.arange(B, dtype=np.uint32) % G).astype(np.uint32)
    rng.shuffle(ids)
    sks = b"".join((int(k) + 1).to_bytes(32, "big") for k in rng.integers(1, 1 << 62, size=B))
    roots = [hashlib.sha256(b"agg" + g.to_bytes(8, "little")).digest() for g in range(G)]
    sigs = batch.sign_batch(sks, b"".join(roots[g] for g in ids), ctx=ctx)
    s_np = np.frombuffer(sigs, dtype=np.uint8).reshape(B, 96)
    d_sigs = batch.DeviceBuffer(ctx, sigs)
    d_out = batch.DeviceBuffer(ctx, nbytes=97 * G)
    p_ids = ids.ctypes.data_as(ctypes.c_void_p)

    def host():
        return batch.aggregate_grouped(sigs, ids, n_groups=G, ctx=ctx)

    def dev():
        ctx.check(ctx.lib.bls_aggregate_grouped_dev(ctx.h, d_sigs.ptr, B, p_ids, G, None, 1, d_out.ptr,
                                                    d_out.ptr + 96 * G))

    grouped = [s_np[ids == g].tobytes() for g in range(G)]
    one = ctypes.create_string_buffer(96)

    def loop():
        res = []
        for g in range(G):
            rc = ctx.check(ctx.lib.bls_aggregate(ctx.h, grouped[g], len(grouped[g]) // 96, one))
            res.append(one.raw if rc == 1 else None)
        return res

    times = {}
    try:
        dev()
        raw = d_out.to_host()
        ref = [raw[96 * g: 96 * g + 96].tobytes() if raw[96 * G + g] else None for g in range(G)]
        assert all(r is not None for r in ref)
        times["dev"] = [_timed(ctx, dev)[0] for _ in range(reps)]
        if not only:
            assert host() == ref
            assert loop() == ref
            times["host"], times["loop"] = [], []
            for k in range(reps):
                times["host"].append(_timed(ctx, host)[0])
                if k < loop_reps:
                    times["loop"].append(_timed(ctx, loop)[0])
    finally:
        d_sigs.free()
        d_out.free()
    res = {"B": B, "G": G, **{k: _stats(v) for k, v in times.items()}}
    if not only:
        fastest_loop = min(times["loop"])
        for k in ("host", "dev"):
            res[f"loop_over_{k}"] = round(statistics.median(times["loop"]) / statistics.median(times[k]), 2)
            assert max(times[k]) < fastest_loop, (k, times)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=7, help="timed calls of (a) and (b) per shape")
    ap.add_argument("--loop-reps", type=int, default=3, help="timed passes of the per-group loop per shape")
    ap.add_argument("--only", choices=("dev",), default=None, help="run route (b) alone")
    ap.add_argument("--shape", type=int, choices=(0, 1), default=None, help="one of the two shapes only")
    args = ap.parse_args()
    from bls_mi355x import _native, batch

    ctx = _native.context()
    shapes = SHAPES if args.shape is None else (SHAPES[args.shape],)
    out = [run_shape(batch, ctx, B, G, max(3, args.reps), max(2, min(args.loop_reps, args.reps)), args.only)
           for B, G in shapes]
    print(json.dumps({"bench": "aggregate_grouped", "unit": "ms per call (all G aggregates)", "shapes": out}),
          flush=True)


if __name__ == "__main__":
    main()
