#!/usr/bin/env python3
"""A/B of the device blob KZG functions (bls_mi355x.kzg, bls_kzg_*) against the route the same functions had before
them, on one MI355X in one process: Python-int F_r arithmetic as the spec writes it (one modular inversion per
denominator), with every g1_lincomb over the Lagrange setup on the resident G1 table (bls_g1_table_msm) and the
pairing check on the device.  The baseline is restated here from the mathematics:

  evaluation   p(z) = f_m for z = w_m, else (z^4096 - 1) / 4096 * sum_i f_i w_i / (z - w_i)
  commitment   sum_i f_i L_i
  proof        sum_i q_i L_i, q_i = (f_i - y) / (w_i - z)                     (z is a hash: outside the domain)
  batch check  e(sum r_i pi_i, -[tau] G2) e(sum r_i C_i + sum r_i z_i pi_i - (sum r_i y_i) G1, G2) == 1, the two
               sums as one multi-exponentiation each

Every shape runs both forms on the same inputs, alternating per repetition: one warm-up call per form, then `--reps`
timed windows of consecutive calls, the device synchronised around every window (wall clock: ctypes, copies and the
challenge hashes included -- these are the calls a spec run makes).  One JSON line per shape and form: median, min
and max ms per call over the windows, and baseline / form.  The results of every timed call are compared with the
baseline's.  No ratio is asserted: the lines are the result.

Shapes: evaluation of 1 and 6 blobs; blob_to_kzg_commitment; compute_blob_kzg_proof; verify_blob_kzg_proof_batch of
1, 6 (a Deneb block) and 64 blobs."""
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
N = 4096
OMEGA = pow(7, (R - 1) // N, R)
DOMAIN = [pow(OMEGA, int(format(i, "012b")[::-1], 2), R) for i in range(N)]
G1_GEN = bytes.fromhex("97f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb")
G2_GEN = bytes.fromhex(
    "93e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049334cf11213945d57e5ac7d055d042b7e"
    "024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d1770bac0326a805bbefd48056c8c121bdb8")


def _line(**kw):
    print(json.dumps(kw), flush=True)


def _timed(ctx, fn):
    ctx.check(ctx.lib.bls_sync(ctx.h))
    t = time.perf_counter()
    out = fn()
    ctx.check(ctx.lib.bls_sync(ctx.h))
    return (time.perf_counter() - t) * 1e3, out


def run_shape(ctx, shape, forms, reps, calls):
    """forms: name -> callable returning the result; the first is the baseline of the ratio"""
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


# ---- the baseline: Python integers, the table MSM and the device pairing check ------------------------------------
def blob_ints(blob):
    f = [int.from_bytes(blob[32 * i: 32 * i + 32], "big") for i in range(N)]
    assert all(v < R for v in f)
    return f


def evaluate_int(f, z):
    if z in DOMAIN:
        return f[DOMAIN.index(z)]
    s = 0
    for fi, w in zip(f, DOMAIN):
        s += fi * w * pow(z - w, -1, R)
    return s % R * (pow(z, N, R) - 1) * pow(N, -1, R) % R


def quotient_int(f, z, y):
    return [(fi - y) * pow(w - z, -1, R) % R for fi, w in zip(f, DOMAIN)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5, help="timed windows per form (at least 5)")
    ap.add_argument("--max-blobs", type=int, default=64, help="largest verification batch (64; smaller to rehearse)")
    args = ap.parse_args()
    reps = max(5, args.reps)
    from bls_mi355x import _native, batch, kzg

    with open(os.path.join(ROOT, "tests", "golden", "trusted_setup.json")) as fh:
        ts = json.load(fh)
    L = [bytes.fromhex(h[2:]) for h in ts["g1_lagrange"]]
    tau_g2 = bytes.fromhex(ts["g2_monomial"][1][2:])
    assert bytes.fromhex(ts["g2_monomial"][0][2:]) == G2_GEN
    ctx = _native.context()
    lib, h = ctx.lib, ctx.h
    ms, S = _timed(ctx, lambda: kzg.KzgSetup(L, tau_g2, ctx=ctx))
    _line(shape="setup: 4,096 Lagrange points into the table, [tau] G2", ms=round(ms, 3))
    idx = S.first + np.arange(N, dtype=np.uint32)
    neg = ctypes.create_string_buffer(96)
    assert lib.bls_point_neg(h, 2, tau_g2, neg) == 1
    neg_tau = neg.raw

    def lincomb(ks):
        return batch.g1_lincomb_indexed(S.table, idx, ks)

    rng = random.Random(0x4B5A)
    B_max = max(6, args.max_blobs)
    blobs = [b"".join(rng.randrange(R).to_bytes(32, "big") for _ in range(N)) for _ in range(6)]
    ints = [blob_ints(b) for b in blobs]
    commitments = S.blob_to_kzg_commitments(blobs)
    proofs = S.compute_blob_kzg_proofs(blobs, commitments)
    zs6 = [rng.randrange(R) for _ in range(6)]

    # -- evaluation
    for B, calls in ((1, 3), (6, 1)):
        run_shape(ctx, "evaluate_polynomial_in_evaluation_form, %d blob%s" % (B, "s" * (B > 1)), {
            "python ints": lambda B=B: [evaluate_int(ints[b], zs6[b]).to_bytes(32, "big") for b in range(B)],
            "bls_kzg_eval_blobs": lambda B=B: S.evaluate_blobs(blobs[:B], zs6[:B])}, reps, calls)

    # -- commitment and proof of one blob
    run_shape(ctx, "blob_to_kzg_commitment", {
        "python ints + table MSM": lambda: lincomb(blob_ints(blobs[0])),
        "bls_kzg_blob_commitments": lambda: S.blob_to_kzg_commitment(blobs[0])}, reps, 5)

    def proof_int(blob, commitment):
        f = blob_ints(blob)
        z = kzg.compute_challenge(blob, commitment)
        return lincomb(quotient_int(f, z, evaluate_int(f, z)))

    run_shape(ctx, "compute_blob_kzg_proof", {
        "python ints + table MSM": lambda: proof_int(blobs[0], commitments[0]),
        "bls_kzg_compute_proofs": lambda: S.compute_blob_kzg_proof(blobs[0], commitments[0])}, reps, 3)

    # -- verification batches
    def verify_int(bl, cm, pf):
        n = len(bl)
        z = [kzg.compute_challenge(b, c) for b, c in zip(bl, cm)]
        y = [evaluate_int(blob_ints(b), zz) for b, zz in zip(bl, z)]
        r = [rng.randrange(1, 1 << 128) for _ in range(n)]
        a = batch.g1_multi_exp(pf, r)
        ks = r + [ri * zi % R for ri, zi in zip(r, z)] + [-sum(ri * yi for ri, yi in zip(r, y)) % R]
        b = batch.g1_multi_exp(list(cm) + list(pf) + [G1_GEN], ks)
        return bool(batch.pairing_check([(a, neg_tau), (b, G2_GEN)]))

    for B in (1, 6, B_max):
        k = [i % 6 for i in range(B)]
        bl, cm, pf = [blobs[i] for i in k], [commitments[i] for i in k], [proofs[i] for i in k]
        run_shape(ctx, "verify_blob_kzg_proof_batch, %d blob%s" % (B, "s" * (B > 1)), {
            "python ints + multi_exp + pairing_check": lambda: verify_int(bl, cm, pf),
            "bls_kzg_verify_blob_batch": lambda: S.verify_blob_kzg_proof_batch(bl, cm, pf)}, reps, 3 if B == 1 else 1)
    _line(shape="counters", g1_table_stats=batch.g1_table_stats(ctx))


if __name__ == "__main__":
    main()
