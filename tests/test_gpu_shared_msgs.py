"""GPU tests of the shared-message RLC batches (bls_fav_batch_indexed_shared, bls_verify_batch_indexed_shared,
bls_fav_job_submit_shared_dev): items that sign the same message share one hash_to_G2 and one Miller
pair, through the segmented G1 sum of csrc/bls_g1_segsum.h.  Verdicts are known by construction, compared with the
unshared entry points on the expanded messages, and spot-checked with the C oracle.  Requires an MI355X."""
import hashlib
import linecache

import numpy as np
import pytest

from oracle import bls_oracle as O
from oracle import bls_oracle_c as OC

pytestmark = pytest.mark.gpu

N_REG = 1 << 14
G1_INF = b"\xc0" + bytes(47)
BAD_PK_0x40 = b"\x40" + bytes(47)
KINDS = ["wrong_msg", "inf_sig", "zero_sig", "ff_tail", "g1_inf_pk", "pk_0x40"]


@pytest.fixture(scope="module")
def batch():
    from bls_mi355x import batch as b
    return b


@pytest.fixture(scope="module")
def registry(batch):
    """Registry sk_i = i + 1 (N_REG keys) with two invalid entries: G1 infinity at index 1 and a 0x40-flag
    encoding at index 2."""
    reg = batch.Registry()
    pks = bytearray(reg.generate(N_REG, first_sk=1, want_bytes=True))
    pks[48:96] = G1_INF
    pks[96:144] = BAD_PK_0x40
    valid = reg.load(bytes(pks))
    assert not valid[1] and not valid[2] and valid.sum() == N_REG - 2
    return bytes(pks)


def _table(seed, M):
    return [hashlib.sha256(b"shared" + seed.to_bytes(8, "little") + m.to_bytes(8, "little")).digest()
            for m in range(M)]


def _ids_from_sizes(sizes, seed):
    """message ids with sizes[m] items of message m, shuffled so that no group is contiguous"""
    ids = np.repeat(np.arange(len(sizes), dtype=np.uint32), sizes)
    np.random.default_rng(seed).shuffle(ids)
    return ids


def _sign(batch, agg_sks, msgs):
    return batch.sign_batch(b"".join(int(a).to_bytes(32, "big") for a in agg_sks), b"".join(msgs))


def _make_batch(batch, ids, table, n, seed, bad_pk_items=()):
    """len(ids) committees of n distinct valid registry keys (>= 3); item j signs table[ids[j]] with the sum of
    its secret keys.  Returns flat indices, offsets, the aggregate secret keys and the signatures."""
    B = len(ids)
    rng = np.random.default_rng(seed)
    if n == 1:
        idx = rng.integers(3, N_REG, size=(B, 1)).astype(np.uint32)
    else:
        idx = np.stack([rng.choice(np.arange(3, N_REG), size=n, replace=False) for _ in range(B)]).astype(np.uint32)
    agg = [int(a) % O.R for a in (idx.astype(np.int64) + 1).sum(axis=1)]  # before the bad keys go in
    for j, k in bad_pk_items:
        idx[j, 0] = k
    offs = np.arange(B + 1, dtype=np.uint64) * n
    sigs = bytearray(_sign(batch, agg, [table[m] for m in ids]))
    return idx.reshape(-1), offs, agg, sigs


def _corrupt(batch, sigs, agg, ids, table, j, kind):
    if kind == "wrong_msg":  # the item's own keys on another table entry: a valid G2 point, only the pairing catches it
        other = table[(int(ids[j]) + 1) % len(table)]
        sigs[96 * j: 96 * j + 96] = _sign(batch, [agg[j]], [other])
    elif kind == "inf_sig":
        sigs[96 * j: 96 * j + 96] = b"\xc0" + bytes(95)
    elif kind == "zero_sig":
        sigs[96 * j: 96 * j + 96] = bytes(96)
    elif kind == "ff_tail":
        sigs[96 * j + 92: 96 * j + 96] = b"\xff" * 4
    else:
        raise AssertionError(kind)


def _expand(table, ids):
    return b"".join(table[m] for m in ids)


def test_parity_with_unshared_path(batch, registry):
    """600 FAV items (n = 4) on 5 messages with skewed group sizes: the shared call's verdicts equal the unshared
    call's on the expanded messages, no fallback work, and the shared batch hashed 5 messages into 5 + 64 pairs."""
    sizes = [1, 3, 40, 156, 400]
    ids = _ids_from_sizes(sizes, 1)
    table = _table(1, 5)
    idx, offs, agg, sigs = _make_batch(batch, ids, table, 4, seed=11)
    out = batch.fast_aggregate_verify_batch_shared(idx, offs, b"".join(table), ids, bytes(sigs))
    assert out.all(), np.nonzero(~out)
    assert batch.fallback_stats() == (0, 0)
    assert batch.batch_work() == (5, 69)
    ref = batch.fast_aggregate_verify_batch(idx, offs, _expand(table, ids), bytes(sigs))
    assert batch.batch_work() == (600, 664)
    assert (out == ref).all()
    # and with bad items in it: still the unshared call's verdicts
    for j, kind in ((7, "wrong_msg"), (300, "inf_sig"), (599, "wrong_msg")):
        _corrupt(batch, sigs, agg, ids, table, j, kind)
    out = batch.fast_aggregate_verify_batch_shared(idx, offs, b"".join(table), ids, bytes(sigs))
    ref = batch.fast_aggregate_verify_batch(idx, offs, _expand(table, ids), bytes(sigs))
    assert (out == ref).all() and sorted(np.nonzero(~out)[0].tolist()) == [7, 300, 599]


FOLD_SIZES = [1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4099]


def test_fold_boundaries(batch, registry):
    """Verify items in groups of every size around K, K^2 and K^3 for K in {8, 16, 32} (three fold levels): all
    valid, then one wrong-message forgery inside the 4,099 group and one inside the singleton -- exactly those
    two fail."""
    ids = _ids_from_sizes(FOLD_SIZES, 2)
    table = _table(2, len(FOLD_SIZES))
    idx, _, agg, sigs = _make_batch(batch, ids, table, 1, seed=12)
    tb = b"".join(table)
    out = batch.verify_batch_shared(idx, tb, ids, bytes(sigs))
    assert out.all(), np.nonzero(~out)
    assert batch.batch_work() == (len(FOLD_SIZES), len(FOLD_SIZES) + 64)
    big = int(np.nonzero(ids == FOLD_SIZES.index(4099))[0][1234])
    single = int(np.nonzero(ids == 0)[0][0])
    for j in (big, single):
        _corrupt(batch, sigs, agg, ids, table, j, "wrong_msg")
    out = batch.verify_batch_shared(idx, tb, ids, bytes(sigs))
    assert sorted(np.nonzero(~out)[0].tolist()) == sorted([big, single])


def test_same_group_swap(batch, registry):
    """Two items of one group exchange signatures: each is a valid signature on the group's message by the other
    item's keys, so the group's UNWEIGHTED sum would still verify; the per-item r_i catch both."""
    ids = _ids_from_sizes([30, 50, 20], 3)
    table = _table(3, 3)
    n = 4
    idx, offs, agg, sigs = _make_batch(batch, ids, table, n, seed=13)
    a, b = (int(x) for x in np.nonzero(ids == 1)[0][[5, 31]])
    sa, sb = bytes(sigs[96 * a: 96 * a + 96]), bytes(sigs[96 * b: 96 * b + 96])
    sigs[96 * a: 96 * a + 96], sigs[96 * b: 96 * b + 96] = sb, sa
    out = batch.fast_aggregate_verify_batch_shared(idx, offs, b"".join(table), ids, bytes(sigs))
    expect = np.ones(len(ids), dtype=bool)
    expect[[a, b]] = False
    assert (out == expect).all(), np.nonzero(out != expect)
    good = next(j for j in range(len(ids)) if j not in (a, b))
    for j in (a, good):
        pkl = [registry[48 * int(x): 48 * int(x) + 48] for x in idx[n * j: n * j + n]]
        assert OC.FastAggregateVerify(pkl, table[ids[j]], bytes(sigs[96 * j: 96 * j + 96])) == bool(expect[j])


def test_adversarial_kinds_in_shared_groups(batch, registry):
    """1,024 FAV items on 16 messages with 8 bad items of every kind of KINDS inside shared groups, plus a group
    whose three items all carry an invalid key: verdicts exact, the bisection isolates the forgeries in fewer
    checks than items, and the dead group does not disturb the others."""
    B, M, n = 1024, 16, 4
    sizes = [3] + [(B - 3) // (M - 1)] * (M - 2)
    sizes.append(B - sum(sizes))
    ids = _ids_from_sizes(sizes, 4)
    table = _table(4, M)
    dead = [int(j) for j in np.nonzero(ids == 0)[0]]
    rng = np.random.default_rng(104)
    bad = sorted(int(j) for j in rng.choice(np.nonzero(ids != 0)[0], size=8, replace=False))
    kinds = {j: KINDS[t % len(KINDS)] for t, j in enumerate(bad)}
    pk_bad = [(j, 1 if kinds[j] == "g1_inf_pk" else 2) for j in bad if kinds[j] in ("g1_inf_pk", "pk_0x40")]
    pk_bad += [(j, 1 + t % 2) for t, j in enumerate(dead)]
    idx, offs, agg, sigs = _make_batch(batch, ids, table, n, seed=14, bad_pk_items=pk_bad)
    for j in bad:
        if kinds[j] not in ("g1_inf_pk", "pk_0x40"):
            _corrupt(batch, sigs, agg, ids, table, j, kinds[j])
    out = batch.fast_aggregate_verify_batch_shared(idx, offs, b"".join(table), ids, bytes(sigs))
    expect = np.ones(B, dtype=bool)
    expect[bad + dead] = False
    assert (out == expect).all(), np.nonzero(out != expect)
    checks, rounds = batch.fallback_stats()
    assert sum(1 for j in bad if kinds[j] == "wrong_msg") > 0 and rounds >= 2
    assert checks < B
    assert batch.batch_work() == (M, M + 64)


@pytest.mark.parametrize("B,M,forge", [(4200, 2100, False), (8400, 4200, True)])
def test_form_thresholds_by_M(batch, registry, B, M, forge):
    """The Miller kernel forms key on M: M = 2,100 is past the eight-lane form (ACC8_MAX = 2,048), M = 4,200 past
    ACC_SHARED_MIN = 4,096 (several pairs per f), where a forgery sends the bisection through its per-item H."""
    ids = _ids_from_sizes([B // M] * M, 5)
    table = _table(5 + M, M)
    idx, _, agg, sigs = _make_batch(batch, ids, table, 1, seed=15 + M)
    expect = np.ones(B, dtype=bool)
    if forge:
        _corrupt(batch, sigs, agg, ids, table, 4321, "wrong_msg")
        expect[4321] = False
    out = batch.verify_batch_shared(idx, b"".join(table), ids, bytes(sigs))
    assert (out == expect).all(), np.nonzero(out != expect)
    assert batch.batch_work() == (M, M + 64)


def test_pipelined_shared_jobs(batch, registry):
    """ResidentFavBatch(msg_ids=...) through run_pipelined: three passes with fixed seeds, the middle one on a
    copy with one forgery; then a shared job followed on the same slot by an unshared one, and the reverse, each
    after a bisection (the per-item H is gathered before the slot's next batch may overwrite H and the ids)."""
    B, M, n = 512, 4, 4
    ids = _ids_from_sizes([B // M] * M, 6)
    table = _table(6, M)
    tb = b"".join(table)
    idx, offs, agg, sigs = _make_batch(batch, ids, table, n, seed=16)
    forged = bytearray(sigs)
    _corrupt(batch, forged, agg, ids, table, 77, "wrong_msg")
    expect_bad = np.ones(B, dtype=bool)
    expect_bad[77] = False
    seeds = [bytes([s + 1]) * 32 for s in range(3)]
    with pytest.raises(ValueError):
        batch.ResidentFavBatch(idx, offs, tb, bytes(sigs), chunks=2, msg_ids=ids)
    good = batch.ResidentFavBatch(idx, offs, tb, bytes(sigs), msg_ids=ids)
    bad = batch.ResidentFavBatch(idx, offs, tb, bytes(forged), msg_ids=ids)
    plain_good = batch.ResidentFavBatch(idx, offs, _expand(table, ids), bytes(sigs))
    plain_bad = batch.ResidentFavBatch(idx, offs, _expand(table, ids), bytes(forged))
    try:
        assert good.run_pipelined(seeds[:1]) == [True] and good.verdicts().all()
        assert bad.run_pipelined(seeds[1:2]) == [False]
        assert (bad.verdicts() == expect_bad).all()
        assert good.run_pipelined(seeds[2:]) == [True] and good.verdicts().all()
        # every job below lands on slot 0 (depth 1): shared + bisection, then unshared; unshared + bisection, then shared
        assert bad.run_pipelined(seeds[:1], depth=1) == [False]
        assert plain_good.run_pipelined(seeds[1:2], depth=1) == [True]
        assert (bad.verdicts() == expect_bad).all() and plain_good.verdicts().all()
        assert plain_bad.run_pipelined(seeds[2:], depth=1) == [False]
        assert good.run_pipelined(seeds[:1], depth=1) == [True]
        assert (plain_bad.verdicts() == expect_bad).all() and good.verdicts().all()
        assert (bad.run() == expect_bad).all()
    finally:
        for rb in (good, bad, plain_good, plain_bad):
            rb.free()


BLOCK_SRC = """
def process_attestation(shim, pks, m, sig):             # specs/phase0/beacon-chain.md:2005 (via :790)
    assert is_valid_indexed_attestation(shim, pks, m, sig)


def is_valid_indexed_attestation(shim, pks, m, sig):    # :776-790
    return shim.FastAggregateVerify(pks, m, sig)
"""


def test_sigsets_share_messages(batch):
    """deferred(registry, share_messages=True) over spec-shaped calls: 40 sets on 3 messages, one invalid.  The
    AssertionError names it and the verdicts equal the default mode's.  (Last in the module: it loads a registry
    of its own.)"""
    from bls_mi355x import bls as shim
    from bls_mi355x import sigsets

    name = "<generated shared-message block spec>"
    linecache.cache[name] = (len(BLOCK_SRC), None, BLOCK_SRC.splitlines(True), name)
    f = {}
    exec(compile(BLOCK_SRC, name, "exec"), f)
    shim.use_mi355x()
    shim.bls_active = True
    reg = batch.Registry()
    sks = list(range(1, 161))
    raw = batch.sk_to_pk_batch(b"".join(k.to_bytes(32, "big") for k in sks))
    pks = [raw[48 * i: 48 * i + 48] for i in range(len(sks))]
    reg.load(raw)
    msgs = [hashlib.sha256(b"slot" + bytes([i])).digest() for i in range(3)]
    sets = []
    for j in range(40):
        c = list(range(4 * j, 4 * j + 4))
        m = msgs[j % 3]
        sets.append(([pks[k] for k in c], m, sum(sks[k] for k in c) % O.R))
    sigs = _sign(batch, [a for _, _, a in sets], [m for _, m, _ in sets])
    sigs = [sigs[96 * j: 96 * j + 96] for j in range(40)]
    sigs[17] = sigs[20]  # the same message (17 % 3 == 20 % 3), other keys
    results = {}
    for share in (False, True):
        with pytest.raises(AssertionError, match="signature set 17 "):
            with sigsets.deferred(reg, share_messages=share) as col:
                for (pkl, m, _), s in zip(sets, sigs):
                    f["process_attestation"](shim, pkl, m, s)
        results[share] = col.results
        assert batch.batch_work() == ((3, 67) if share else (40, 104))
    assert results[True] == results[False] == [j != 17 for j in range(40)]
