"""GPU tests of the complete G1 formulas with one reduction per output coordinate (csrc/bls_fq_g1.h) through the
kernels that run them: the registry gather (k_fav_gather_q: g1q_add_aff per lane, g1q_add in the LDS tree), the
r_i apk_i chain of k_sig_lane2 (g1q_mul_endo: g1q_dbl / g1q_add) and the segmented sum of shared-message batches
(k_g1_seg_fold).  The gather runs k_fav_gather_q<64> (one workgroup and 64 lanes per aggregate) below 1,024
aggregates and k_fav_gather_q<16> (16 lanes per aggregate, four aggregates per workgroup) from there up, so the
cases come twice: in batches of five aggregates, and inside one batch of 1,029.  A 4,096-key registry (sk_i = i + 1) with the negations of keys 0 .. 63 and one invalid key
appended.  An aggregate's signature is made with the sum of its secret keys, so its verdict is True exactly when
the device's aggregate key is the oracle's sum; the C oracle gives that sum (AggregatePKs) and every item's
verdict (FastAggregateVerify).  Requires an MI355X."""
import hashlib

import numpy as np
import pytest

from oracle import bls_oracle as O
from oracle import bls_oracle_c as OC

pytestmark = pytest.mark.gpu

REG = 1 << 12
NEG = REG            # REG + i: -pk_i, i < 64
INVALID = REG + 64   # the G1 identity: fails KeyValidate
OUT_OF_RANGE = REG + 65
G1_INF = b"\xc0" + bytes(47)


def _neg(pk48: bytes) -> bytes:
    return bytes([pk48[0] ^ 0x20]) + pk48[1:]  # the sign flag: -P has the other y


@pytest.fixture(scope="module")
def batch():
    from bls_mi355x import batch as b
    return b


@pytest.fixture(scope="module")
def keys(batch):
    """the registry's compressed keys by index"""
    reg = batch.Registry()
    pks = reg.generate(REG, first_sk=1, want_bytes=True)
    extra = b"".join(_neg(pks[48 * i: 48 * i + 48]) for i in range(64)) + G1_INF
    valid = reg.append(extra)
    assert valid[:64].all() and not valid[64] and len(reg) == OUT_OF_RANGE
    return pks + extra


def _sk(k: int) -> int:
    return k + 1 if k < REG else -(k - REG + 1)


def _msgs(tag: bytes, B: int):
    return [hashlib.sha256(b"g1dot" + tag + j.to_bytes(4, "little")).digest() for j in range(B)]


def _sign(batch, sks, msgs):
    return batch.sign_batch(b"".join((sk or 1).to_bytes(32, "big") for sk in sks), b"".join(msgs))


def _oracle(keys, committee, sk, msg, sig):
    """the oracle's verdict on one item, after checking that its sum of the keys is [sk] G1 (so that the
    signature by sk tests the device's sum against the oracle's)"""
    if any(k >= OUT_OF_RANGE for k in committee):
        return False  # no such key: the item is invalid by construction
    pkl = [keys[48 * k: 48 * k + 48] for k in committee]
    if sk and all(k != INVALID for k in committee):
        assert OC.AggregatePKs(pkl) == OC.SkToPk(sk)
    return OC.FastAggregateVerify(pkl, msg, sig)


def _check(batch, keys, committees, tag):
    B = len(committees)
    sks = [sum(_sk(k) for k in c if k < INVALID) % O.R for c in committees]
    msgs = _msgs(tag, B)
    sigs = _sign(batch, sks, msgs)
    offs = batch.offsets_from_lengths([len(c) for c in committees])
    out = batch.fast_aggregate_verify_batch(np.concatenate([np.asarray(c, dtype=np.uint32) for c in committees]),
                                            offs, b"".join(msgs), sigs)
    expect = [_oracle(keys, c, sk, m, sigs[96 * j: 96 * j + 96])
              for j, (c, sk, m) in enumerate(zip(committees, sks, msgs))]
    assert out.tolist() == expect, (out.tolist(), expect)
    return expect


@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 33, 64])
def test_aggregates_of_n_keys(batch, keys, n):
    """five aggregates of n keys: k_fav_gather_q<64>, one key per lane at most (identity + key in every lane that
    has one), the sums formed by g1q_add in the LDS tree over 63, 62, 49, 48, 47, 31 and no identity leaves"""
    rng = np.random.default_rng(n)
    committees = [rng.choice(REG, size=n, replace=False).tolist() for _ in range(5)]
    assert all(_check(batch, keys, committees, b"n%d" % n))


def test_degenerate_aggregates(batch, keys):
    """inside one aggregate each, in k_fav_gather_q<64> (one key per lane, so the pairs meet in the tree's g1q_add):
    a repeated key, a key beside its negation in neighbouring lanes and another 16 lanes apart, a sum that is the
    identity, an invalid key, an out-of-range index"""
    rng = np.random.default_rng(99)
    base = [rng.choice(np.arange(64, REG), size=33, replace=False).tolist() for _ in range(5)]
    base[0][19] = base[0][3]
    base[1][0], base[1][1] = 5, NEG + 5
    base[1][2], base[1][18] = 9, NEG + 9
    base[2] = [k for i in range(16) for k in (i, NEG + i)]  # the pairs meet in the tree and in lanes
    base[3][20] = INVALID
    base[4][32] = OUT_OF_RANGE
    assert _check(batch, keys, base, b"deg") == [True, True, False, False, False]


def test_batch_with_one_forgery(batch, keys):
    """70 aggregates of 33 keys, item 41 signed on another item's message: only the pairing check catches it,
    through r_41 apk_41 of the chain"""
    B, n = 70, 33
    rng = np.random.default_rng(7)
    committees = [rng.choice(REG, size=n, replace=False) for _ in range(B)]
    sks = [int(sum(int(k) + 1 for k in c)) % O.R for c in committees]
    msgs = _msgs(b"forge", B)
    signed = list(msgs)
    signed[41] = msgs[40]
    sigs = _sign(batch, sks, signed)
    out = batch.fast_aggregate_verify_batch(np.concatenate(committees).astype(np.uint32),
                                            batch.offsets_from_lengths([n] * B), b"".join(msgs), sigs)
    assert np.nonzero(~out)[0].tolist() == [41]


def test_shared_message_batch(batch, keys):
    """70 items over 3 messages (groups of 40, 29 and 1: two fold levels, one run and a singleton), so the segmented
    G1 sum folds the r_i apk_i; all valid, then one forgery inside the largest group"""
    n = 3
    ids = np.repeat(np.arange(3, dtype=np.uint32), [40, 29, 1])
    np.random.default_rng(5).shuffle(ids)
    table = _msgs(b"shared", 3)
    rng = np.random.default_rng(6)
    committees = [rng.choice(REG, size=n, replace=False) for _ in range(len(ids))]
    sks = [int(sum(int(k) + 1 for k in c)) % O.R for c in committees]
    idx = np.concatenate(committees).astype(np.uint32)
    offs = batch.offsets_from_lengths([n] * len(ids))
    sigs = bytearray(_sign(batch, sks, [table[m] for m in ids]))
    out = batch.fast_aggregate_verify_batch_shared(idx, offs, b"".join(table), ids, bytes(sigs))
    assert out.all(), np.nonzero(~out)
    j = int(np.nonzero(ids == 0)[0][17])
    sigs[96 * j: 96 * j + 96] = _sign(batch, [sks[j]], [table[1]])
    out = batch.fast_aggregate_verify_batch_shared(idx, offs, b"".join(table), ids, bytes(sigs))
    assert np.nonzero(~out)[0].tolist() == [j]


# ---- the same cases inside a batch large enough for k_fav_gather_q<16> (key position p of an aggregate goes to
# lane p % 16, four aggregates per workgroup) ----
BIG_B = 1029  # >= 1,024, and 1,029 % 4 == 1: the last workgroup holds one aggregate and three empty slots
SIZES = [1, 2, 15, 16, 17, 33, 64]
FORGED = 600


def _big_committees():
    rng = np.random.default_rng(1029)
    c = [rng.choice(np.arange(64, REG), size=SIZES[b % 7] if b >= 8 else 33, replace=False).tolist()
         for b in range(BIG_B)]
    c[0][19] = c[0][3]                                      # P + P in lane 3's accumulator
    c[1][0], c[1][16] = 9, NEG + 9                          # lane 0 passes through the identity, then adds c[1][32]
    c[1][1], c[1][2] = 5, NEG + 5                           # neighbouring lanes: they meet in the tree
    c[2] = [k for i in range(16) for k in (i, NEG + i)]     # the identity, pairs in neighbouring lanes
    c[3] = list(range(16)) + [NEG + i for i in range(16)]   # the identity in every lane: the tree adds identities
    c[4][20] = INVALID
    c[5][32] = OUT_OF_RANGE
    c[6] = [77]                                             # 15 lanes of the aggregate stay at the identity
    c[7][4], c[7][20] = 11, NEG + 11                        # one lane back at the identity, nothing after it
    c[BIG_B - 1] = rng.choice(np.arange(64, REG), size=33, replace=False).tolist()
    c[BIG_B - 1][21] = c[BIG_B - 1][5]                      # the lone aggregate of the last workgroup: P + P in lane 5
    return c


@pytest.fixture(scope="module")
def big(batch, keys):
    """one batch of 1,029 aggregates through the device, computed once: (committees, sks, msgs, sigs, verdicts)"""
    committees = _big_committees()
    sks = [sum(_sk(k) for k in c if k < INVALID) % O.R for c in committees]
    msgs = _msgs(b"big", BIG_B)
    signed = list(msgs)
    signed[FORGED] = msgs[FORGED + 1]
    sigs = _sign(batch, sks, signed)
    offs = batch.offsets_from_lengths([len(c) for c in committees])
    out = batch.fast_aggregate_verify_batch(np.concatenate([np.asarray(c, dtype=np.uint32) for c in committees]),
                                            offs, b"".join(msgs), sigs)
    return committees, sks, msgs, sigs, out


def _oracle_item(keys, big, j):
    committees, sks, msgs, sigs, _ = big
    return _oracle(keys, committees[j], sks[j], msgs[j], sigs[96 * j: 96 * j + 96])


def test_lanes16_degenerate_aggregates(keys, big):
    """k_fav_gather_q<16>: a key repeated at positions j and j + 16 (P + P in one lane's g1q_add_aff), a key and its
    negation 16 positions apart (the lane's accumulator passes through the identity and goes on) and in neighbouring
    lanes, the identity sum with pairs across lanes and inside every lane, an invalid key, an out-of-range index, a
    single key, and the repeated key again in the lone aggregate of the partly empty last workgroup -- each against
    the oracle's sum and verdict"""
    out = big[4]
    items = list(range(8)) + [BIG_B - 1]
    expect = [_oracle_item(keys, big, j) for j in items]
    assert expect == [True, True, False, False, False, False, True, True, True]
    assert [bool(out[j]) for j in items] == expect


def test_lanes16_aggregates_of_n_keys(keys, big):
    """k_fav_gather_q<16>: aggregates of 1, 2, 15, 16, 17, 33 and 64 keys (fewer keys than lanes, one per lane, one
    lane with two, two full rounds and a third, four rounds), two of each size against the oracle's sum and verdict;
    the other aggregates of the batch are valid by construction (signed with the sum of their secret keys) but for
    the forged item, which only the pairing check catches"""
    committees, _, _, _, out = big
    for n in SIZES:
        for j in [b for b in range(8, BIG_B - 1) if len(committees[b]) == n and b != FORGED][:2]:
            assert _oracle_item(keys, big, j) is True and out[j], (n, j)
    assert not _oracle_item(keys, big, FORGED)
    bad = set(np.nonzero(~out)[0].tolist())
    assert bad == {2, 3, 4, 5, FORGED}
