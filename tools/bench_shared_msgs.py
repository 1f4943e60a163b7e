#!/usr/bin/env python3
"""A/B of the shared-message RLC batches against the unshared entry points on one MI355X, in one process and
alternating per repetition (one warm-up call per shape, then `--reps` timed calls each, the device synchronised
around every timed window).  Prints one JSON line per shape and a summary line per part.

  (a) C4 shard shape: 125,000 Verify with pk_i = registry[i] through the host-buffer calls (PCIe included):
      verify_batch on distinct messages (the unshared path) against verify_batch_shared with
      M in {125,000, 2,048, 64, 1} table entries (item i signs entry i mod M).
  (b) C3 shape: 2,048 FastAggregateVerify x 512 keys through ResidentFavBatch (device-resident inputs, pipelined
      passes): one distinct message per committee against msg_ids with M = 32 (one message per slot).

What must hold is asserted: the verdicts of every timed call equal the unshared call's, and every repetition of
every shape with M <= 2,048 is faster than every unshared repetition.  The M = B line shows what the fold costs
when nothing is shared.
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

# the hardware-queue policy of bench.py, before HIP starts: the pipelined part keeps ten jobs x two streams busy
if not os.environ.get("BLSMI355X_KEEP_HW_QUEUES") and int(os.environ.get("GPU_MAX_HW_QUEUES", "0") or 0) < 24:
    os.environ["GPU_MAX_HW_QUEUES"] = "24"

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def _line(**kw):
    print(json.dumps(kw), flush=True)


def _msgs(tag: bytes, n: int) -> list[bytes]:
    return [hashlib.sha256(tag + j.to_bytes(8, "little")).digest() for j in range(n)]


def _timed(ctx, fn):
    ctx.check(ctx.lib.bls_sync(ctx.h))
    t = time.perf_counter()
    out = fn()
    ctx.check(ctx.lib.bls_sync(ctx.h))
    return (time.perf_counter() - t) * 1e3, out


def _report(part, base_name, times, units, unit):
    """JSON lines of one part: every shape against the unshared call of the same run"""
    base = times[base_name]
    spread = (max(base) - min(base)) / statistics.median(base)
    for name, ts in times.items():
        med = statistics.median(ts)
        _line(part=part, shape=name, ms_median=round(med, 3), ms_min=round(min(ts), 3), ms_max=round(max(ts), 3),
              reps=len(ts), value=round(units / med * 1e3, 1), unit=unit,
              speedup_vs_unshared=round(statistics.median(base) / med, 3))
    _line(part=part, summary=True, unshared_spread=round(spread, 4),
          note="speedup_vs_unshared = unshared median / shape median; unshared_spread = (max - min) / median")


def part_a(batch, ctx, reg_n, B, reps):
    idx = (np.arange(B, dtype=np.uint32) % reg_n).astype(np.uint32)
    sks = b"".join(int(k + 1).to_bytes(32, "big") for k in idx)
    shapes = {}
    msgs = _msgs(b"gossip", B)
    m_un = b"".join(msgs)
    s_un = batch.sign_batch(sks, m_un, ctx=ctx)
    shapes["unshared"] = (lambda: batch.verify_batch(idx, m_un, s_un, ctx=ctx), (B, B + 64))
    for M in (B, 2048, 64, 1):
        table = _msgs(b"shared%d" % M, M)
        ids = (np.arange(B, dtype=np.uint32) % M).astype(np.uint32)
        sg = batch.sign_batch(sks, b"".join(table[m] for m in ids), ctx=ctx)
        tb = b"".join(table)
        shapes[f"shared M={M}"] = (
            lambda tb=tb, ids=ids, sg=sg: batch.verify_batch_shared(idx, tb, ids, sg, ctx=ctx), (M, M + 64))
    times = {k: [] for k in shapes}
    for name, (fn, work) in shapes.items():  # warm-up: scratch allocation, and the verdicts
        assert fn().all(), name
        assert batch.batch_work(ctx=ctx) == work, name
    for _ in range(reps):
        for name, (fn, _) in shapes.items():
            ms, v = _timed(ctx, fn)
            assert v.all(), name  # = the unshared call's verdicts: every item is valid
            times[name].append(ms)
    _report("a: %d Verify, host buffers" % B, "unshared", times, B, "Verify/s")
    fastest_un = min(times["unshared"])
    for M in (2048, 64, 1):
        assert max(times[f"shared M={M}"]) < fastest_un, (M, times)


def part_b(batch, ctx, reg_n, reps, passes):
    rng = np.random.default_rng(0x5EED)
    perm = rng.permutation(reg_n).astype(np.uint32)
    B, n = 2048, reg_n // 2048
    offs = np.arange(B + 1, dtype=np.uint64) * n
    agg = (perm.reshape(B, n).astype(np.int64) + 1).sum(axis=1)
    sks = b"".join((int(a) % R).to_bytes(32, "big") for a in agg)
    msgs = _msgs(b"epoch", B)
    table = _msgs(b"slot", 32)
    ids = (np.arange(B, dtype=np.uint32) // 64).astype(np.uint32)  # 64 committees per slot
    s_un = batch.sign_batch(sks, b"".join(msgs), ctx=ctx)
    s_sh = batch.sign_batch(sks, b"".join(table[m] for m in ids), ctx=ctx)
    rbs = {
        "unshared": batch.ResidentFavBatch(perm, offs, b"".join(msgs), s_un, ctx=ctx),
        "shared M=32": batch.ResidentFavBatch(perm, offs, b"".join(table), s_sh, ctx=ctx, msg_ids=ids),
    }
    times = {k: [] for k in rbs}
    try:
        for name, rb in rbs.items():
            assert all(rb.run_pipelined([os.urandom(32)])) and rb.verdicts().all(), name
        for _ in range(reps):
            for name, rb in rbs.items():
                ms, oks = _timed(ctx, lambda rb=rb: rb.run_pipelined([os.urandom(32) for _ in range(passes)]))
                assert all(oks) and rb.verdicts().all(), name
                times[name].append(ms / passes)
    finally:
        for rb in rbs.values():
            rb.free()
    _report("b: 2048 FAV x %d keys, resident, %d pipelined passes per call" % (n, passes), "unshared", times, B,
            "FAV/s")
    assert max(times["shared M=32"]) < min(times["unshared"]), times


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5, help="timed calls per shape (at least 5)")
    ap.add_argument("--passes", type=int, default=40, help="pipelined passes per timed call of part (b)")
    ap.add_argument("--part", choices=("a", "b", "ab"), default="ab")
    args = ap.parse_args()
    reps = max(5, args.reps)
    from bls_mi355x import _native, batch

    ctx = _native.context()
    reg_n = 1 << 20
    batch.Registry(ctx).generate(reg_n, first_sk=1)
    if "a" in args.part:
        part_a(batch, ctx, reg_n, 125000, reps)
    if "b" in args.part:
        part_b(batch, ctx, reg_n, reps, max(1, args.passes))


if __name__ == "__main__":
    main()
