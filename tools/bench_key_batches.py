#!/usr/bin/env python3
"""A/B of the key-table batches (bls_fav_batch_keys, bls_verify_batch_keys, bls_deposits_verify) against the routes
sigsets takes for the same sets today and against the indexed batch on a preloaded registry (the ceiling: no
KeyValidate in the timed call), on one MI355X in one process.  Every shape runs its forms on the same inputs,
alternating per repetition: one warm-up call per form, then `--reps` timed windows each of `--calls` consecutive
host-buffer calls, the device synchronised around every window (wall clock, copies included: these are the calls a
spec run makes).  One JSON line per shape and form: median, min and max ms per call over the windows, the ratio
today / form, and for the keys forms the key-table stage's own time from bls_profile_read (untimed extra calls).

  (a) 64 FastAggregateVerify sets x 128 keys drawn from a pool of 256.   today: one per-call FastAggregateVerify each
  (b) 1,024 Verify items on distinct raw keys, all valid and with one bad signature.   today: aggregate_verify_batch
  (c) 16 and 4,096 deposits.   today: hashlib signing roots on the host + aggregate_verify_batch
No ratio is asserted: the lines are the result.  Verdicts of every timed call are checked."""
from __future__ import annotations

import argparse
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

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def _line(**kw):
    print(json.dumps(kw), flush=True)


def _timed(ctx, fn):
    ctx.check(ctx.lib.bls_sync(ctx.h))
    t = time.perf_counter()
    out = fn()
    ctx.check(ctx.lib.bls_sync(ctx.h))
    return (time.perf_counter() - t) * 1e3, out


def _msg(tag, j):
    return hashlib.sha256(tag + j.to_bytes(8, "little")).digest()


def run_shape(batch, ctx, shape, forms, expect, reps, calls, profiled=()):
    """forms: name -> callable returning the verdicts; "today" is the baseline of the ratio.  A timed window is
    `calls` consecutive calls of one form (ms per call = window / calls).  profiled: the forms whose key-table
    stage is then read from bls_profile_read in untimed calls (hipEvent pair around the one launch)."""
    times = {k: [] for k in forms}
    for name, fn in forms.items():
        assert list(fn()) == list(expect), (shape, name)

    def window(fn):
        out = None
        for _ in range(calls):
            out = fn()
        return out

    for _ in range(reps):
        for name, fn in forms.items():
            ms, out = _timed(ctx, lambda fn=fn: window(fn))
            assert list(out) == list(expect), (shape, name)
            times[name].append(ms / calls)
    kv = {}
    pr = batch.Profiler(ctx)
    for name in profiled:
        pr.start()
        for _ in range(4):
            forms[name]()
        got = pr.read()
        pr.stop()
        kv[name] = round(got["key_validate"][0] / max(got["key_validate"][1], 1), 4)
    med = {k: statistics.median(v) for k, v in times.items()}
    for name, ts in times.items():
        _line(shape=shape, form=name, ms_per_call_median=round(med[name], 3), ms_min=round(min(ts), 3),
              ms_max=round(max(ts), 3), reps=len(ts), calls_per_window=calls,
              today_over_form=round(med["today"] / med[name], 3), key_table_stage_ms=kv.get(name))


def deposit_root(pk, wc, amount, domain):
    h = lambda x: hashlib.sha256(x).digest()
    return h(h(h(h(pk[:32] + pk[32:] + bytes(16)) + wc) + h(amount.to_bytes(8, "little") + bytes(56))) + domain)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=7, help="timed windows per form (at least 5)")
    ap.add_argument("--calls", type=int, default=20, help="consecutive calls per timed window")
    ap.add_argument("--shapes", default="a,b,c", help="comma-separated subset of a, b, c")
    args = ap.parse_args()
    reps, calls = max(5, args.reps), max(1, args.calls)
    shapes = set(args.shapes.split(","))
    from bls_mi355x import _native, batch
    from bls_mi355x.backend import mi355x_bls

    ctx = _native.context()
    NK = 4096
    raw = batch.sk_to_pk_batch(b"".join((i + 1).to_bytes(32, "big") for i in range(NK)), ctx=ctx)
    pool = [raw[48 * i: 48 * i + 48] for i in range(NK)]
    reg = batch.Registry(ctx)

    def sign(sks, msgs):
        return batch.sign_batch(b"".join((s % R).to_bytes(32, "big") for s in sks), b"".join(msgs), ctx=ctx)

    if "a" in shapes:
        rng = np.random.default_rng(0xA)
        sets = [rng.choice(256, size=128, replace=False) for _ in range(64)]
        msgs = [_msg(b"a", j) for j in range(64)]
        sigs = sign([int((s + 1).sum()) for s in sets], msgs)
        table, idx, offs = batch.key_table([[pool[t] for t in s] for s in sets])
        reg.load(table)
        forms = {
            "today": lambda: [mi355x_bls.FastAggregateVerify([pool[t] for t in s], msgs[j], sigs[96 * j: 96 * j + 96])
                              for j, s in enumerate(sets)],
            "keys": lambda: batch.fast_aggregate_verify_batch_keys(table, idx, offs, b"".join(msgs), sigs, ctx=ctx),
            "keys + key_table": lambda: batch.fast_aggregate_verify_batch_keys(
                *batch.key_table([[pool[t] for t in s] for s in sets]), b"".join(msgs), sigs, ctx=ctx),
            "indexed (registry preloaded)": lambda: batch.fast_aggregate_verify_batch(idx, offs, b"".join(msgs), sigs,
                                                                                      ctx=ctx),
        }
        run_shape(batch, ctx, "a: 64 FAV x 128 keys of 256", forms, [True] * 64, reps, calls, ("keys",))

    if "b" in shapes:
        B = 1024
        msgs = [_msg(b"b", j) for j in range(B)]
        good = sign([i + 1 for i in range(B)], msgs)
        bad = bytearray(good)
        bad[96 * 500: 96 * 501] = bad[96 * 499: 96 * 500]
        keys = b"".join(pool[:B])
        reg.load(keys)
        ident = np.arange(B, dtype=np.uint32)
        for tag, sigs, expect in (("all valid", good, [True] * B),
                                  ("one bad", bytes(bad), [j != 500 for j in range(B)])):
            sl = [sigs[96 * j: 96 * j + 96] for j in range(B)]
            forms = {
                "today": lambda sl=sl: batch.aggregate_verify_batch([[k] for k in pool[:B]], [[m] for m in msgs], sl,
                                                                    ctx=ctx),
                "keys": lambda sigs=sigs: batch.verify_batch_keys(keys, b"".join(msgs), sigs, ctx=ctx),
                "indexed (registry preloaded)": lambda sigs=sigs: batch.verify_batch(ident, b"".join(msgs), sigs,
                                                                                     ctx=ctx),
            }
            run_shape(batch, ctx, "b: 1,024 raw-key Verify, " + tag, forms, expect, reps, calls, ("keys",))

    if "c" in shapes:
        domain = bytes([3, 0, 0, 0]) + hashlib.sha256(b"genesis").digest()[:28]
        for N in (16, 4096):
            pks = pool[:N]
            wcs = [_msg(b"wc", i) for i in range(N)]
            amts = [32 * 10 ** 9 + i for i in range(N)]
            roots = [deposit_root(pks[i], wcs[i], amts[i], domain) for i in range(N)]
            sigs = sign([i + 1 for i in range(N)], roots)
            sl = [sigs[96 * j: 96 * j + 96] for j in range(N)]
            reg.load(b"".join(pks))
            ident = np.arange(N, dtype=np.uint32)

            def today():
                rr = [deposit_root(pks[i], wcs[i], amts[i], domain) for i in range(N)]
                return batch.aggregate_verify_batch([[k] for k in pks], [[r] for r in rr], sl, ctx=ctx)

            forms = {
                "today": today,
                "deposits": lambda: batch.verify_deposits(pks, wcs, amts, sl, domain, ctx=ctx),
                "indexed (registry preloaded, roots given)": lambda: batch.verify_batch(ident, b"".join(roots), sigs,
                                                                                        ctx=ctx),
            }
            run_shape(batch, ctx, "c: %d deposits" % N, forms, [True] * N, reps, calls, ("deposits",))


if __name__ == "__main__":
    main()
