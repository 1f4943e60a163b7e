"""Scenarios of the launch-plan test (tests/test_gpu_launch_plan.py) and of its recorder
(tools/record_launch_plan.py): one small batch per form of a FastAggregateVerify batch, each run once all-valid and
once with corrupted items, and what the library reports of it afterwards -- the profiler's per-name launch counts
(never its times), bls_last_batch_work, after a failing batch bls_last_fallback_stats, and for bits batches
bls_last_gather_work.  Everything here is a function of the scenario alone (the RLC seed moves no count), so the
records of two builds of the library can be compared for equality.

Registry: 2^10 generated keys, key i the public key of secret i + 1, so an item's aggregate secret is the sum of
(i + 1) over its signers and every signature is valid by construction unless the scenario replaces it."""
import hashlib

import numpy as np

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
REG = 1 << 10
SMALL_B = 80          # bisection tree 80 -> 5 -> 1: one gated level below the first checked one
SMALL_BAD = (5, 70)   # two failures in different 16-blocks
COMMITTEES = (9, 17)  # members per committee, neither a multiple of 8
SEEDS = (bytes(range(32)), bytes(range(32, 64)))


def _msgs(tag: str, n: int) -> list:
    return [hashlib.sha256(b"launch-plan" + tag.encode() + j.to_bytes(4, "little")).digest() for j in range(n)]


def _sign(batch, ctx, sks, msgs, bad):
    """One signature per item; every item of `bad` then carries its right-hand neighbour's (another key set, and
    for unshared batches another message: only the pairing check catches it).  Returns (sigs, expected verdicts)."""
    sigs = bytearray(batch.sign_batch(b"".join(int(sk).to_bytes(32, "big") for sk in sks), b"".join(msgs), ctx=ctx))
    expect = np.ones(len(sks), dtype=bool)
    for b in bad:
        assert sks[b] != sks[b + 1]
        sigs[96 * b: 96 * b + 96] = sigs[96 * (b + 1): 96 * (b + 2)]
        expect[b] = False
    return bytes(sigs), expect


def _indexed_items(B: int, seed: int):
    """B items of 1 to 3 distinct registry keys."""
    rng = np.random.default_rng(seed)
    idx = [rng.choice(REG, size=1 + b % 3, replace=False).astype(np.uint32) for b in range(B)]
    sks = [sum(int(k) + 1 for k in c) % R for c in idx]
    return idx, sks


def _bits_items(B: int):
    """Items over one or both committees (members 0 .. 8 and 9 .. 25): every third item lacks one member (the
    complement form adds fewer points), the others have two signers (the direct form does)."""
    lists = [np.arange(0, COMMITTEES[0], dtype=np.uint32), np.arange(COMMITTEES[0], sum(COMMITTEES), dtype=np.uint32)]
    comm_ids, bits, sks = [], [], []
    for b in range(B):
        ids = [[0], [1], [0, 1]][b % 3]
        members = np.concatenate([lists[c] for c in ids])
        on = np.zeros(members.size, dtype=bool)
        if b % 3 == 0:
            on[:] = True
            on[(3 * b + 1) % members.size] = False
        else:
            on[[b % members.size, (b + 4) % members.size]] = True
        comm_ids.append(ids)
        bits.append(on)
        sks.append(sum(int(k) + 1 for k in members[on]) % R)
    return lists, comm_ids, bits, sks


class Run:
    """Profiler on around one scenario; record() is what the fixture keeps of it."""

    def __init__(self, batch, ctx):
        self.batch, self.ctx = batch, ctx
        self.prof = batch.Profiler(ctx)
        self.prof.start()

    def record(self, failing: bool, bits: bool = False) -> dict:
        b = self.batch
        rec = {"launches": {name: cnt for name, (_, cnt) in self.prof.read().items()},
               "batch_work": list(b.batch_work(self.ctx))}
        if failing:
            rec["fallback_stats"] = list(b.fallback_stats(self.ctx))
        if bits:
            rec["gather_work"] = list(b.gather_work(self.ctx))
        self.prof.stop()
        return rec


def _small(form: str, bad):
    def run(batch, ctx):
        B = SMALL_B
        shared = form.endswith("shared")
        msg_ids = np.arange(B, dtype=np.uint32) % 3 if shared else None
        table = _msgs(form, 3 if shared else B)
        item_msgs = [table[i] for i in msg_ids] if shared else table
        if form.startswith("bits"):
            lists, comm_ids, bits, sks = _bits_items(B)
            comm = batch.Committees(ctx).load(lists)
        elif form == "verify":
            idx = [np.array([(7 * b + 3) % REG], dtype=np.uint32) for b in range(B)]
            sks = [int(c[0]) + 1 for c in idx]
        else:
            idx, sks = _indexed_items(B, seed=B)
        sigs, expect = _sign(batch, ctx, sks, item_msgs, bad)
        r = Run(batch, ctx)
        if form.startswith("bits"):
            out = batch.fast_aggregate_verify_batch_bits(comm, comm_ids, bits, b"".join(table), sigs,
                                                         msg_ids=msg_ids, mode="auto", ctx=ctx)
        elif form == "verify":
            out = batch.verify_batch(np.concatenate(idx), b"".join(table), sigs, ctx=ctx)
        elif shared:
            out = batch.fast_aggregate_verify_batch_shared(np.concatenate(idx),
                                                           batch.offsets_from_lengths([len(c) for c in idx]),
                                                           b"".join(table), msg_ids, sigs, ctx=ctx)
        else:
            out = batch.fast_aggregate_verify_batch(np.concatenate(idx),
                                                    batch.offsets_from_lengths([len(c) for c in idx]),
                                                    b"".join(table), sigs, ctx=ctx)
        return r.record(bool(bad), bits=form.startswith("bits")), out, expect
    return run


def _threshold(B: int, bad):
    def run(batch, ctx):
        idx = (np.arange(B, dtype=np.uint32) * 5 + 1) % REG
        sks = [int(k) + 1 for k in idx]
        msgs = _msgs("threshold", B)
        sigs, expect = _sign(batch, ctx, sks, msgs, bad)
        r = Run(batch, ctx)
        out = batch.verify_batch(idx, b"".join(msgs), sigs, ctx=ctx)
        return r.record(bool(bad)), out, expect
    return run


def _jobs(batch, ctx):
    """The job API: two passes (two seeds) over the small indexed batch with its bad items."""
    idx, sks = _indexed_items(SMALL_B, seed=SMALL_B)
    msgs = _msgs("jobs", SMALL_B)
    sigs, expect = _sign(batch, ctx, sks, msgs, SMALL_BAD)
    rb = batch.ResidentFavBatch(np.concatenate(idx), batch.offsets_from_lengths([len(c) for c in idx]),
                                b"".join(msgs), sigs, ctx=ctx)
    r = Run(batch, ctx)
    try:
        oks = rb.run_pipelined(SEEDS)  # ends with bls_sync
        out = rb.verdicts()
        rec = r.record(True)
    finally:
        rb.free()
    rec["passes_ok"] = [bool(o) for o in oks]
    return rec, out, expect


def scenarios() -> dict:
    """name -> run(batch, ctx) -> (record, verdicts, expected verdicts); the registry is loaded by the caller."""
    s = {}
    for form in ("indexed", "shared", "bits", "bits_shared", "verify"):
        s[form + "_valid"] = _small(form, ())
        s[form + "_bad"] = _small(form, SMALL_BAD)
    for B in (2047, 2048, 4096):  # either side of ACC8_MAX, and ACC_SHARED_MIN (the bisection recomputes f there)
        s["threshold_%d_valid" % B] = _threshold(B, ())
        s["threshold_%d_bad" % B] = _threshold(B, (B // 2,))
    s["jobs_bad"] = _jobs
    return s


def load_registry(batch, ctx) -> None:
    batch.Registry(ctx).generate(REG, first_sk=1)
