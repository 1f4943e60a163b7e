#!/usr/bin/env python3
"""A/B of the resident G1 table's batched bucket MSM (bls_g1_table_msm) against bls_multi_exp -- the route every
multi-exponentiation took before the table existed -- on one MI355X in one process.  Every shape runs its forms on
the same inputs, alternating per repetition: one warm-up call per form, then `--reps` timed windows each of
consecutive host-buffer calls, the device synchronised around every window (wall clock, ctypes and copies included:
these are the calls a spec run makes).  One JSON line per shape and form: median, min and max ms per call over the
windows, and baseline / form.  The result bytes of every timed call are checked against the baseline's.

  (a) n = 4,096, B = 1, full-width scalars.
  (b) n = 4,096, B = 128 (one blob's cell-proof MSMs) against 128 bls_multi_exp calls.
  (c) the spec's g1_lincomb body (bytes48_to_G1 per point, then multi_exp) at n = 4,096 with and without
      curve.use_g1_table.
  (d) n = 16, 64, 256, B = 1: whether the table route loses below some n.
The points are the 4,096 Lagrange points of tests/golden/trusted_setup.json.  The load of 8,192 entries (the points
twice: decode and 31 window multiples each) is timed and reported, not compared.  No ratio is asserted: the lines are
the result."""
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
for _p in (ROOT, os.path.join(ROOT, "eth-consensus-specs_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def _line(**kw):
    print(json.dumps(kw), flush=True)


def _timed(ctx, fn):
    ctx.check(ctx.lib.bls_sync(ctx.h))
    t = time.perf_counter()
    out = fn()
    ctx.check(ctx.lib.bls_sync(ctx.h))
    return (time.perf_counter() - t) * 1e3, out


def run_shape(ctx, shape, forms, reps, calls):
    """forms: name -> callable returning the result bytes; the first is the baseline of the ratio"""
    base = next(iter(forms))
    expect = forms[base]()
    for name, fn in forms.items():
        assert fn() == expect, (shape, name)
    times = {k: [] for k in forms}

    def window(fn):
        out = None
        for _ in range(calls):
            out = fn()
        return out

    for _ in range(reps):
        for name, fn in forms.items():
            ms, out = _timed(ctx, lambda fn=fn: window(fn))
            assert out == expect, (shape, name)
            times[name].append(ms / calls)
    med = {k: statistics.median(v) for k, v in times.items()}
    for name, ts in times.items():
        _line(shape=shape, form=name, ms_per_call_median=round(med[name], 3), ms_min=round(min(ts), 3),
              ms_max=round(max(ts), 3), reps=len(ts), calls_per_window=calls,
              baseline_over_form=round(med[base] / med[name], 2),
              separated=bool(name == base or max(ts) < min(times[base])))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5, help="timed windows per form (at least 5)")
    ap.add_argument("--shapes", default="a,b,c,d", help="comma-separated subset of a, b, c, d")
    args = ap.parse_args()
    reps = max(5, args.reps)
    shapes = set(args.shapes.split(","))
    from bls_mi355x import _native, batch, bls, curve

    with open(os.path.join(ROOT, "tests", "golden", "trusted_setup.json")) as fh:
        L = [bytes.fromhex(h[2:]) for h in json.load(fh)["g1_lagrange"]]
    ctx = _native.context()
    lib, h = ctx.lib, ctx.h
    rng = random.Random(0x61)
    table = batch.G1Table(ctx)
    ms, _ = _timed(ctx, lambda: (table.load(L), table.append(L)))
    _line(shape="load: 8,192 entries (decode + 31 window multiples each, host map included)", ms=round(ms, 3))
    lib.bls_g1_table_load(h, b"".join(L), len(L), 0, None)  # warm
    ms, _ = _timed(ctx, lambda: (lib.bls_g1_table_load(h, b"".join(L), len(L), 0, None),
                                 lib.bls_g1_table_append(h, b"".join(L), len(L), 0, None)))
    _line(shape="load: 8,192 entries, C ABI calls alone", ms=round(ms, 3))
    table.load(L)

    def multi_exp(pts, ks):
        out = ctypes.create_string_buffer(48)
        assert lib.bls_multi_exp(h, 1, pts, ks, len(ks) // 32, 0, out) == 1
        return out.raw

    def table_msm(idx, ks, B):
        out = ctypes.create_string_buffer(48 * B)
        assert lib.bls_g1_table_msm(h, idx.ctypes.data, idx.size, ks, B, out) == 1
        return out.raw

    def scalars(n, B=1):
        return b"".join(rng.randrange(1 << 256).to_bytes(32, "big") for _ in range(n * B))

    if "a" in shapes or "d" in shapes:
        for n, calls in ((4096, 5),) * ("a" in shapes) + ((16, 20), (64, 20), (256, 20)) * ("d" in shapes):
            idx = np.arange(n, dtype=np.uint32)
            pts, ks = b"".join(L[:n]), scalars(n)
            run_shape(ctx, "n = %d, B = 1" % n, {
                "bls_multi_exp": lambda: multi_exp(pts, ks),
                "bls_g1_table_msm": lambda: table_msm(idx, ks, 1)}, reps, calls)

    if "b" in shapes:
        n, B = 4096, 128
        idx = np.arange(n, dtype=np.uint32)
        pts, ks = b"".join(L), scalars(n, B)
        run_shape(ctx, "n = 4096, B = 128", {
            "128 x bls_multi_exp": lambda: b"".join(multi_exp(pts, ks[32 * n * v: 32 * n * (v + 1)]) for v in range(B)),
            "bls_g1_table_msm": lambda: table_msm(idx, ks, B)}, reps, 1)

    if "c" in shapes:
        bls.use_mi355x()
        bls.bls_active = True
        kz = [rng.randrange(R) for _ in range(len(L))]

        def g1_lincomb(points, scalars_):  # specs/deneb/polynomial-commitments.md:266-286
            points_g1 = []
            for point in points:
                points_g1.append(bls.bytes48_to_G1(point))
            return bytes(bls.G1_to_bytes48(bls.multi_exp(points_g1, scalars_)))

        def with_table():
            curve.use_g1_table(table)
            try:
                return g1_lincomb(L, kz)
            finally:
                curve.use_g1_table(None)

        run_shape(ctx, "spec g1_lincomb, n = 4096", {
            "no table": lambda: g1_lincomb(L, kz), "curve.use_g1_table": with_table}, reps, 1)
    _line(shape="counters", g1_table_stats=batch.g1_table_stats(ctx))


if __name__ == "__main__":
    main()
