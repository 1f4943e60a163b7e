"""GPU check of the RLC batch check's signature MSM (csrc/bls_msm.hip) through bls_test_rlc_msm, which runs the FAV
batch's own stage -- sort, bucket folds (k_msm_fold0 / k_msm_fold1), bit sums, affine pairs -- and returns the 64 bit
sums U_b, against the oracle's sum_i r_i sigma_i.

The weights.  The batch pairs U_b with -w_b G1, w_b = 2^b for b < 32 and 2^(b - 32) lambda for b >= 32, lambda =
-x^2 mod r the eigenvalue of the G1 endomorphism (bls_g1_endo.h: r_i = a + b lambda is a statement about the G1
side).  The product of the e(-w_b G1, U_b) is e(-G1, S) for S = sum_b w_b U_b with the w_b taken as integers mod r,
so on G2 the scalar the device's pairs imply for a 64-bit s is the integer r(s) = (s mod 2^32) + (s >> 32) lambda
mod r, and the test compares S with sum_i r(s_i) sigma_i.

Every scalar 0x0101010101010101 puts all n entries in bucket 1 of every window; with the run length K given, n = 1,
2, K, K + 1, 2 K + 1 and K^2 + 1 reach the run boundary, the even cut and the second fold with one and with K + 1
partials."""
import ctypes
import hashlib
import random

import numpy as np
import pytest

from oracle import bls_oracle as O

pytestmark = pytest.mark.gpu

X_ABS = 0xD201000000010000
LAMBDA = (-X_ABS * X_ABS) % O.R
ONES = 0x0101010101010101
IDENT = bytes([0xC0]) + bytes(95)


def r_of(s):
    return ((s & 0xFFFFFFFF) + (s >> 32) * LAMBDA) % O.R


def usums(points, scalars, K=0):
    """the 64 bit sums (affine points, None for the identity) of the device's MSM at run length K (0: its own)"""
    from bls_mi355x import _native

    ctx = _native.context()
    sigs = b"".join(O.g2_compress(p) for p in points)
    sc = np.ascontiguousarray(scalars, dtype=np.uint64)
    out = ctypes.create_string_buffer(64 * 96)
    assert ctx.check(ctx.lib.bls_test_rlc_msm(ctx.h, sigs, sc.ctypes.data, len(points), K, out)) == 1
    raw = [out.raw[96 * b: 96 * b + 96] for b in range(64)]
    return [None if u == IDENT else O.g2_decompress(u) for u in raw]


def weighted(U):
    """S = sum_b w_b U_b: one Horner chain per half, the high half times lambda"""
    def horner(us):
        s = None
        for u in reversed(us):
            s = O.g2_add(O.g2_add(s, s), u)
        return s

    return O.g2_add(horner(U[:32]), O.g2_mul(horner(U[32:]), LAMBDA))


@pytest.fixture(scope="module")
def chain():
    """sigma_i = (k0 + i step) G2 for i < 300: distinct points with known discrete logs"""
    rng = random.Random(0x51C)
    k0, step = rng.randrange(1, O.R), rng.randrange(1, O.R)
    d = O.g2_mul(O.G2_GEN, step)
    pts, cur = [], O.g2_mul(O.G2_GEN, k0)
    for _ in range(300):
        pts.append(cur)
        cur = O.g2_add(cur, d)
    return pts, [(k0 + i * step) % O.R for i in range(300)]


def _one_bucket(points, K):
    """all entries in bucket 1 of every window: U_b is the plain sum for b = 0 mod 8 and the identity elsewhere"""
    n = len(points)
    U = usums(points, [ONES] * n, K)
    total = None
    for p in points:
        total = O.g2_add(total, p)
    for b in range(64):
        assert U[b] == (total if b % 8 == 0 else None), (n, K, b)
    assert weighted(U) == O.g2_mul(total, r_of(ONES)), (n, K)


@pytest.mark.parametrize("K", [4, 8, 16])
def test_one_bucket_run_boundaries(chain, K):
    pts, _ = chain
    for n in (1, 2, K, K + 1, 2 * K + 1, K * K + 1):
        _one_bucket(pts[:n], K)


@pytest.mark.parametrize("K", [4, 16])
def test_one_bucket_duplicates_and_cancellation(chain, K):
    pts, _ = chain
    for n in (2, K + 1, 2 * K + 1):
        _one_bucket([pts[0]] * n, K)  # doublings inside the complete formulas, in the runs and between partials
    # sigma_j = -sigma_i pairs cancel the whole bucket: its sum reads as the identity downstream (every U_b, and S)
    for n in (2, 2 * K + 2, K * K + K):
        half = pts[: n // 2]
        both = [q for p in half for q in (p, O.g2_neg(p))]
        U = usums(both, [ONES] * n, K)
        assert U == [None] * 64, (n, K)
        # (the scatter's atomics order a bucket's entries, so which runs cancel alone is not the test's to choose)
        U = usums(half + [O.g2_neg(p) for p in half], [ONES] * n, K)
        assert U == [None] * 64, (n, K)
    # the cancelled pairs and one more point
    extra = [pts[1], O.g2_neg(pts[1])] * K + [pts[2]]
    _one_bucket(extra, K)


def _check_against_oracle(pts, logs, sc, K):
    U = usums(pts, sc, K)
    k = sum(r_of(s) * e for s, e in zip(sc, logs)) % O.R
    assert weighted(U) == O.g2_mul(O.G2_GEN, k), K
    for b in (0, 31, 32, 63):
        e = None
        for s, p in zip(sc, pts):
            if (s >> b) & 1:
                e = O.g2_add(e, p)
        assert U[b] == e, (K, b)


@pytest.mark.parametrize("K", [16, 4, 1, 0])
def test_random_scalars(chain, K):
    """300 random 64-bit scalars on 300 distinct signatures: ~0.15 entries per bucket, so most buckets are empty or
    hold one entry and a few hold two.  With the run folds on (K = 16, 4) every run is its bucket's only one: each
    lane bisects the run offsets to its own bucket and k_msm_fold0 writes the sum straight to the bucket sums, and
    k_msm_fold1 writes the identity for the many empty buckets.  K = 1 makes every entry a run, so the buckets of two
    are folded by k_msm_fold1 from partials that lie between other buckets'.  K = 0 is the batch's own form for 300
    items, the lane-pair kernel (300 < MSM_FOLD_MIN)."""
    pts, logs = chain
    rng = random.Random(0x51D)
    sc = [rng.getrandbits(64) for _ in range(300)]
    sc[7] = 0  # no entry at all
    sc[8] = 1 << 63
    _check_against_oracle(pts, logs, sc, K)


@pytest.mark.parametrize("K", [16, 4])
def test_few_full_buckets(chain, K):
    """300 scalars whose bytes are all 1, 2 or 3: three buckets of ~100 entries in every window and 2,037 empty
    ones -- 7 (K = 16) or 25 (K = 4) runs per bucket, cut evenly, the partials of neighbouring buckets side by side."""
    pts, logs = chain
    rng = random.Random(0x51E)
    sc = [sum(rng.randrange(1, 4) << (8 * w) for w in range(8)) for _ in range(300)]
    _check_against_oracle(pts, logs, sc, K)


@pytest.mark.parametrize("K", [0, 16])
def test_no_items(K):
    """no entry anywhere: every bucket sum is the identity k_msm_fold1 (K = 16) or the lane-pair kernel writes"""
    assert usums([], [], K) == [None] * 64


N_REG = 1 << 12
FOLD_MIN = 32 * 255  # MSM_FOLD_MIN of csrc/bls_msm.hip: the run folds from here, the lane-pair kernel below


def test_fold_min_matches_the_source():
    import os
    import re

    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "eth-consensus-specs_amd", "csrc",
                            "bls_msm.hip")).read()
    assert re.search(r"constexpr size_t MSM_FOLD_MIN = 32 \* 255;", src)


@pytest.fixture(scope="module")
def registry():
    from bls_mi355x import batch

    reg = batch.Registry()
    reg.generate(N_REG, first_sk=1, want_bytes=False)
    return batch


@pytest.mark.parametrize("B", [FOLD_MIN - 1, FOLD_MIN])
def test_fav_batch_on_each_side_of_the_size_switch(registry, B):
    """One FAV batch just below MSM_FOLD_MIN (k_msm_bucketc<4>) and one at it (k_msm_fold0 / k_msm_fold1), by the
    construction of tests/test_gpu_batches.py: item j signs SHA256(seed || j) with the sum of its committee's secret
    keys sk_i = i + 1.  All valid: the batch check passes with no fallback work, which it cannot with a wrong S.
    Then item 5 carries item 6's signature, a valid point for another message: exactly that verdict is false."""
    batch = registry
    n = 4
    rng = np.random.default_rng(B)
    idx = rng.integers(0, N_REG, size=(B, n), dtype=np.int64)
    offs = np.arange(B + 1, dtype=np.uint64) * n
    msgs = b"".join(hashlib.sha256(B.to_bytes(8, "little") + j.to_bytes(8, "little")).digest() for j in range(B))
    agg = [int(a) % O.R for a in (idx + 1).sum(axis=1)]
    sigs = bytearray(batch.sign_batch(b"".join(a.to_bytes(32, "big") for a in agg), msgs))
    flat = idx.reshape(-1).astype(np.uint32)
    out = batch.fast_aggregate_verify_batch(flat, offs, msgs, bytes(sigs))
    assert out.all()
    assert batch.fallback_stats() == (0, 0)
    sigs[96 * 5: 96 * 6] = sigs[96 * 6: 96 * 7]
    out = batch.fast_aggregate_verify_batch(flat, offs, msgs, bytes(sigs))
    expect = np.ones(B, dtype=bool)
    expect[5] = False
    assert (out == expect).all(), np.nonzero(out != expect)
    assert batch.fallback_stats()[1] >= 1
