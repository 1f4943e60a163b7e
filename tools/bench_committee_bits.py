#!/usr/bin/env python3
"""A/B of the committee-bitfield FAV batches against the index-list job API on one MI355X, in one process and
alternating per repetition (one warm-up call per form, then `--reps` timed calls each of `--passes` pipelined
passes, the device synchronised around every timed window).  Prints one JSON line per form and participation, a
conditions line per participation, and the bls_profile_read split of the gather and the expansion.

Workload: the C3 shape -- 2,048 FastAggregateVerify x 512 keys from a registry of 2^20, the committees a table of
64 per slot x 32 slots -- with exactly round(512 q) participants per item, q in {50 %, 90 %, 99 %, 100 %}:
  indexed      bls_fav_job_submit_dev on the expanded index lists: the code every earlier batch runs, the baseline
  indexed A/A  the same batch object timed as a second series: the run-to-run spread
  bits auto    bls_fav_job_submit_bits_dev, mode auto (complement iff it adds fewer points)
  bits direct  the same, mode direct
aa_spread = |median(indexed) - median(indexed A/A)| / median(indexed).  What must hold is checked after everything
is printed (exit status 1 otherwise): every form's verdicts are all true; at 99 % auto beats the indexed baseline
by more than aa_spread; at 50 % direct is no slower than the baseline beyond aa_spread.
"""
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

# the hardware-queue policy of bench.py, before HIP starts: the pipelined passes keep ten jobs x two streams busy
if not os.environ.get("BLSMI355X_KEEP_HW_QUEUES") and int(os.environ.get("GPU_MAX_HW_QUEUES", "0") or 0) < 24:
    os.environ["GPU_MAX_HW_QUEUES"] = "24"

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
B, N = 2048, 512


def _line(**kw):
    print(json.dumps(kw), flush=True)


def _timed(ctx, fn):
    ctx.check(ctx.lib.bls_sync(ctx.h))
    t = time.perf_counter()
    out = fn()
    ctx.check(ctx.lib.bls_sync(ctx.h))
    return (time.perf_counter() - t) * 1e3, out


def _passes(rb, passes):
    return rb.run_pipelined([os.urandom(32) for _ in range(passes)])


def one_participation(batch, ctx, com, members, q, reps, passes):
    rng = np.random.default_rng(int(q * 1000))
    p = int(round(N * q))
    bits = np.zeros((B, N), dtype=bool)
    for b in range(B):
        bits[b, rng.choice(N, size=p, replace=False)] = True
    agg = ((members.astype(np.int64) + 1) * bits).sum(axis=1)
    sks = b"".join((int(a) % R).to_bytes(32, "big") for a in agg)
    msgs = b"".join(hashlib.sha256(b"bits%d" % p + j.to_bytes(8, "little")).digest() for j in range(B))
    sigs = batch.sign_batch(sks, msgs, ctx=ctx)
    idx = members[bits].astype(np.uint32)
    offs = np.arange(B + 1, dtype=np.uint64) * p
    cids, rows = list(range(B)), list(bits)
    rbs = {
        "indexed": batch.ResidentFavBatch(idx, offs, msgs, sigs, ctx=ctx),
        "bits auto": batch.ResidentFavBatch(None, None, msgs, sigs, ctx=ctx, committees=com, committee_ids=cids,
                                            bits=rows, mode="auto"),
        "bits direct": batch.ResidentFavBatch(None, None, msgs, sigs, ctx=ctx, committees=com, committee_ids=cids,
                                              bits=rows, mode="direct"),
    }
    series = {"indexed": "indexed", "indexed A/A": "indexed", "bits auto": "bits auto", "bits direct": "bits direct"}
    times = {k: [] for k in series}
    work, prof = {}, {}
    try:
        for name, rb in rbs.items():  # warm-up: scratch allocation, and the verdicts
            assert all(_passes(rb, 1)) and rb.verdicts().all(), name
            if name != "indexed":
                work[name] = batch.gather_work(ctx=ctx)
        for _ in range(reps):
            for name, rbn in series.items():
                ms, oks = _timed(ctx, lambda rb=rbs[rbn]: _passes(rb, passes))
                assert all(oks) and rbs[rbn].verdicts().all(), name
                times[name].append(ms / passes)
        pr = batch.Profiler(ctx)
        for name, rb in rbs.items():  # untimed: the per-kernel split (hipEvent pairs serialise the streams' kernels)
            pr.start()
            _passes(rb, 4)
            got = pr.read()
            pr.stop()
            prof[name] = {k: round(got[k][0] / max(got[k][1], 1), 4) for k in ("fav_gather", "bits_expand")
                          if k in got and got[k][1]}
    finally:
        for rb in rbs.values():
            rb.free()
    med = {k: statistics.median(v) for k, v in times.items()}
    aa = abs(med["indexed"] - med["indexed A/A"]) / med["indexed"]
    for name, ts in times.items():
        _line(participation=q, form=name, ms_per_pass_median=round(med[name], 4), ms_min=round(min(ts), 4),
              ms_max=round(max(ts), 4), reps=len(ts), passes=passes, fav_per_s=round(B / med[name] * 1e3, 1),
              speedup_vs_indexed=round(med["indexed"] / med[name], 4), gather_work=work.get(name),
              kernel_ms=prof.get(series[name]))
    return med, aa


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5, help="timed calls per form (at least 5)")
    ap.add_argument("--passes", type=int, default=300, help="pipelined passes per timed call (a third of a second)")
    args = ap.parse_args()
    reps, passes = max(5, args.reps), max(1, args.passes)
    from bls_mi355x import _native, batch

    ctx = _native.context()
    reg_n = 1 << 20
    batch.Registry(ctx).generate(reg_n, first_sk=1)
    members = np.random.default_rng(0xC3).permutation(reg_n).astype(np.uint32).reshape(B, N)
    com = batch.Committees(ctx).load((members.reshape(-1), np.arange(B + 1, dtype=np.uint64) * N))
    ok = True
    for q in (0.5, 0.9, 0.99, 1.0):
        med, aa = one_participation(batch, ctx, com, members, q, reps, passes)
        cond = {}
        if q == 0.99:
            cond["auto beats indexed by more than aa_spread"] = med["bits auto"] < med["indexed"] * (1 - aa)
        if q == 0.5:
            cond["direct no slower than indexed beyond aa_spread"] = med["bits direct"] <= med["indexed"] * (1 + aa)
        _line(participation=q, summary=True, aa_spread=round(aa, 4), conditions=cond)
        ok = ok and all(cond.values())
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
