"""The registry gather's pair-first loop (k_fav_gather_q: two keys of a lane summed first by g1q_add_aff2, a pair
with equal x sent through the complete mixed additions) through the batch API, against the construction: every
signature is made from the sum of its committee's secret keys, so a wrong aggregate key is a wrong verdict.

One batch of 4,099 aggregates runs the full-batch kernel (4,099 % 16 = 3: the last workgroup is part empty), one of
1,029 the 16-lane kernel and three of 5 the 64-lane kernel.  Planted in each: for every stride s in {2, 4, 8, 16, 64}
(whichever lane count a kernel has, positions 0 and s are one lane's pair for one of them) a repeated key at 0 and
s, a key at 0 with its negation at s, a repeated key at 0 and 2s (one lane, different pairs), a lane whose partial
sum passes through the identity, and the invalid key as the first and as the second key of a pair; {P, -P} alone
(the identity: invalid), an out-of-range index, an empty aggregate and one signature of another message (batch_ok
is False and the bisection runs)."""
import hashlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
REG = 1 << 14
NNEG = 64
INVALID = REG + NNEG  # the registry index of the key that fails KeyValidate
OUT_OF_RANGE = REG + NNEG + 1 + 1000
STRIDES = (2, 4, 8, 16, 64)
SIZES = (1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 33, 130)


def _neg(pk48: bytes) -> bytes:
    return bytes([pk48[0] ^ 0x20]) + pk48[1:]  # the sign flag: -P has the other y


def _sk(k: int) -> int:
    """the secret key of registry entry k: key i is (i + 1) G, entry REG + i its negation"""
    return k + 1 if k < REG else -(k - REG + 1)


def _planted(rng, strides):
    """(committee, good) for every planted case; good: the construction's verdict for a signature by the summed
    secret keys"""
    def fresh(n):  # n distinct keys outside 0..63 (so none meets its own negation by accident)
        return (NNEG + rng.choice(REG - NNEG, size=n, replace=False)).astype(np.int64)

    cases = []
    for s in strides:
        c = fresh(2 * s + 3)
        c[s] = c[0]
        cases.append((c, True))  # the same key at 0 and s
        c = fresh(2 * s + 3)
        c[0], c[s] = s % NNEG, REG + s % NNEG
        cases.append((c, True))  # a key at 0, its negation at s
        c = fresh(2 * s + 3)
        c[2 * s] = c[0]
        cases.append((c, True))  # the same key at 0 and 2s
        c = fresh(3 * s + 5)
        c[0], c[s], c[2 * s], c[3 * s] = 3, 9, REG + 3, REG + 9
        cases.append((c, True))  # a lane's partial sum is the identity after its second pair, then goes on
        c = fresh(2 * s + 3)
        c[0] = INVALID
        cases.append((c, False))  # the invalid key first in its pair
        c = fresh(2 * s + 3)
        c[s] = INVALID
        cases.append((c, False))  # ... and second
    return cases


def _planted_other(rng):
    c = (NNEG + rng.choice(REG - NNEG, size=9, replace=False)).astype(np.int64)
    c[4] = OUT_OF_RANGE
    return [(np.array([7, REG + 7], dtype=np.int64), False),  # {P, -P}: the identity
            (c, False),  # an out-of-range index
            (np.array([], dtype=np.int64), False)]  # an empty aggregate


def _batch(seed, B, planted):
    """B committees: the planted ones first (then a wrong-message signature's aggregate), the rest random with
    sizes cycling through SIZES"""
    rng = np.random.default_rng(seed)
    comms, good = [], []
    for c, g in planted(rng):
        comms.append(c)
        good.append(g)
    wrong = len(comms)
    assert wrong + 2 <= B
    for b in range(wrong, B):
        comms.append(rng.choice(REG, size=SIZES[b % len(SIZES)], replace=False).astype(np.int64))
        good.append(True)
    sks = [sum(_sk(int(k)) for k in c if k < REG + NNEG) % R for c in comms]
    assert all(sk != 0 for c, sk, g in zip(comms, sks, good) if g)
    msgs = [hashlib.sha256(b"pairs" + seed.to_bytes(4, "little") + j.to_bytes(4, "little")).digest() for j in range(B)]
    return comms, sks, good, msgs, wrong


@pytest.fixture(scope="module")
def registry():
    """a 2^14-key registry + the negations of keys 0..63 + one key that fails KeyValidate, loaded once"""
    from bls_mi355x import _native, batch

    ctx = _native.context()
    reg = batch.Registry(ctx)
    pks = reg.generate(REG, first_sk=1, want_bytes=True)
    assert reg.append(b"".join(_neg(pks[48 * i: 48 * i + 48]) for i in range(NNEG))).all()
    assert not reg.append(bytes(48)).any()  # no compression flag: not a key
    assert len(reg) == REG + NNEG + 1
    return ctx


def _run(ctx, seed, B, planted):
    from bls_mi355x import batch

    comms, sks, good, msgs, wrong = _batch(seed, B, planted)
    sigs = bytearray(batch.sign_batch(b"".join((sk or 1).to_bytes(32, "big") for sk in sks), b"".join(msgs), ctx=ctx))
    expect = np.array(good, dtype=bool)
    # the first random aggregate carries its neighbour's signature: only the pairing check catches it
    sigs[96 * wrong: 96 * (wrong + 1)] = sigs[96 * (wrong + 1): 96 * (wrong + 2)]
    expect[wrong] = False
    offs = batch.offsets_from_lengths([len(c) for c in comms])
    flat = np.concatenate(comms).astype(np.uint32)
    out = batch.fast_aggregate_verify_batch(flat, offs, b"".join(msgs), bytes(sigs), ctx=ctx)
    rb = batch.ResidentFavBatch(flat, offs, b"".join(msgs), bytes(sigs), ctx=ctx)
    oks = rb.run_pipelined([os.urandom(32) for _ in range(2)])
    v = rb.verdicts()
    rb.free()
    assert (out == expect).all(), np.nonzero(out != expect)
    assert (v == expect).all(), np.nonzero(v != expect)
    assert oks == [False, False]


def _all_planted(rng):
    return _planted(rng, STRIDES) + _planted_other(rng)


def test_full_batch_kernel(registry, monkeypatch):
    """4,099 aggregates: the full-batch lane count, the last workgroup part empty"""
    monkeypatch.setenv("BLS_GATHER", "complete")
    _run(registry, 4099, 4099, _all_planted)


def test_sixteen_lane_kernel(registry, monkeypatch):
    """1,029 aggregates: k_fav_gather_q<16>, whose loop is the same"""
    monkeypatch.setenv("BLS_GATHER", "complete")
    _run(registry, 1029, 1029, _all_planted)


@pytest.mark.parametrize("part", [0, 1])
def test_sixty_four_lane_kernel(registry, monkeypatch, part):
    """5 aggregates: k_fav_gather_q<64>, one lane's pair is positions 0 and 64.  Five aggregates hold three planted
    cases beside the wrong-message pair, so the cases come in batches of 5: these two and the bad inputs below."""
    monkeypatch.setenv("BLS_GATHER", "complete")

    def planted(rng):
        p = _planted(rng, (64,))
        # part 0: repeated key, key and negation, repeated key two pairs apart
        # part 1: the lane through the identity, the invalid key second in its pair, {P, -P}
        return p[:3] if part == 0 else [p[3], p[5], _planted_other(rng)[0]]

    _run(registry, 5 + part, 5, planted)


def test_sixty_four_lane_kernel_bad_inputs(registry, monkeypatch):
    """5 aggregates: the invalid key first in its pair, an out-of-range index, an empty aggregate"""
    monkeypatch.setenv("BLS_GATHER", "complete")

    def planted(rng):
        return [_planted(rng, (64,))[4]] + _planted_other(rng)[1:]

    _run(registry, 7, 5, planted)
