"""GPU tests of the key-table FAV batches (bls_fav_batch_keys, bls_verify_batch_keys, bls_fav_job_submit_keys_dev,
bls_deposits_verify): batches whose keys come as bytes and are decoded and KeyValidated by the batch
itself.  Verdicts are known by construction (sign_batch on the sum of the members' secrets), equal those of the
indexed batch on a registry loaded with the same table -- the defining property -- and, for items of at most three
keys, the C oracle's FastAggregateVerify.  Requires an MI355X."""
import hashlib

import numpy as np
import pytest

from dispatch_edge_inputs import WIDE_KEYS_MAX, bad_keys
from oracle import bls_oracle as O
from oracle import bls_oracle_c as OC

pytestmark = pytest.mark.gpu

NKEYS = WIDE_KEYS_MAX + 1


@pytest.fixture(scope="module")
def b():
    from bls_mi355x import batch
    return batch


@pytest.fixture(scope="module")
def pool(b):
    """pk_i = [i + 1] G1 for i < WIDE_KEYS_MAX + 1, computed once"""
    raw = b.sk_to_pk_batch(b"".join((i + 1).to_bytes(32, "big") for i in range(NKEYS)))
    return [raw[48 * i: 48 * i + 48] for i in range(NKEYS)]


def _msg(tag, j):
    return hashlib.sha256(tag + j.to_bytes(8, "little")).digest()


def _sign(b, agg_sks, msgs):
    raw = b.sign_batch(b"".join((int(a) % O.R or 1).to_bytes(32, "big") for a in agg_sks), b"".join(msgs))
    return [raw[96 * i: 96 * i + 96] for i in range(len(msgs))]


def _table_131(pool):
    """K = 131 with the four bad encodings at 0, 1, 64 and K - 1; entry t otherwise pk_t (secret t + 1)"""
    K = 131
    keys = list(pool[:K])
    for pos, enc in zip((0, 1, 64, K - 1), bad_keys().values()):
        keys[pos] = enc
    return keys, {0, 1, 64, K - 1}


def test_parity_over_sizes_and_bad_keys(b, pool):
    keys, bad = _table_131(pool)
    K = len(keys)
    good = [t for t in range(K) if t not in bad]
    rng = np.random.default_rng(7)
    items = [[int(t) for t in rng.choice(good, size=n, replace=False)] for n in (0, 1, 2, 3, 63, 64, 65)]
    items.append([t for t in range(K) if t != 5])       # 130 entries, bad ones among them -> False
    items.append([7, 7])                                # the same key twice counts twice
    items.append([9, 10, 9])                            # a repeat among others
    items.append([good[0], 0])                          # a member that fails KeyValidate
    items.append([int(t) for t in rng.choice(good, size=127, replace=False)] + [2, 2, 3])  # 130 good entries
    msgs = [_msg(b"kb1", j) for j in range(len(items))]
    sigs = _sign(b, [sum(t + 1 for t in it if t not in bad) for it in items], msgs)
    expect = [len(it) > 0 and not (set(it) & bad) for it in items]
    idx = np.array([t for it in items for t in it], dtype=np.uint32)
    offs = b.offsets_from_lengths([len(it) for it in items])
    table = b"".join(keys)
    out, valid = b.fast_aggregate_verify_batch_keys(table, idx, offs, b"".join(msgs), b"".join(sigs),
                                                    want_key_valid=True)
    assert list(out) == expect
    mask = b.Registry().load(table)
    assert (valid == mask).all() and [t for t in range(K) if not mask[t]] == sorted(bad)
    ref = b.fast_aggregate_verify_batch(idx, offs, b"".join(msgs), b"".join(sigs))
    assert (out == ref).all()
    for j, it in enumerate(items):
        if 0 < len(it) <= 3:
            assert OC.FastAggregateVerify([keys[t] for t in it], msgs[j], sigs[j]) is expect[j], j


@pytest.mark.parametrize("K", [1, 2, 3, 64, 65, WIDE_KEYS_MAX, WIDE_KEYS_MAX + 1])
def test_kernel_switch_and_odd_tails(b, pool, K):
    """an invalid key at entry 0 and at entry K - 1: the tail of the two-keys-per-workgroup kernel and the last lane
    of the last wave of the lane kernel; everything else valid"""
    enc = list(bad_keys().values())
    keys = list(pool[:K])
    keys[0] = enc[0]
    keys[K - 1] = enc[1 if K > 1 else 0]
    msgs = [_msg(b"kb2", j) for j in range(K)]
    raw = b.sign_batch(b"".join((i + 1).to_bytes(32, "big") for i in range(K)), b"".join(msgs))
    out = b.verify_batch_keys(b"".join(keys), b"".join(msgs), raw)
    expect = np.ones(K, dtype=bool)
    expect[0] = expect[K - 1] = False
    assert (out == expect).all(), np.nonzero(out != expect)
    if K <= 3:
        for j in range(K):
            assert OC.FastAggregateVerify([keys[j]], msgs[j], raw[96 * j: 96 * j + 96]) is bool(expect[j])


def test_out_of_range_and_empty(b, pool):
    K = 4
    items = [[0, 1], [2, K], [3, 0xFFFFFFFF], [1, 2, 3]]
    msgs = [_msg(b"kb3", j) for j in range(4)]
    sigs = _sign(b, [sum(t + 1 for t in it if t < K) for it in items], msgs)
    idx = np.array([t for it in items for t in it], dtype=np.uint32)
    offs = b.offsets_from_lengths([len(it) for it in items])
    out = b.fast_aggregate_verify_batch_keys(b"".join(pool[:K]), idx, offs, b"".join(msgs), b"".join(sigs))
    assert list(out) == [True, False, False, True]
    from bls_mi355x import _native
    c = _native.context()
    res = np.ones(3, dtype=np.uint8)
    i0 = np.zeros(3, dtype=np.uint32)
    o3 = np.arange(4, dtype=np.uint64)
    rc = c.lib.bls_fav_batch_keys(c.h, None, 0, i0.ctypes.data, o3.ctypes.data, 3, b"".join(msgs[:3]), 0, None,
                                  b"".join(sigs[:3]), res.ctypes.data, None)
    assert rc == 1 and list(res) == [0, 0, 0]


def test_no_registry_needed_and_none_touched(b, pool):
    from bls_mi355x import _native

    items = [[0, 1, 2], [3], [4, 5]]
    msgs = [_msg(b"kb4", j) for j in range(3)]
    sigs = _sign(b, [sum(t + 1 for t in it) for it in items], msgs)
    idx = np.array([t for it in items for t in it], dtype=np.uint32)
    offs = b.offsets_from_lengths([len(it) for it in items])
    table = b"".join(pool[:6])
    fresh = _native.Context()
    try:
        with pytest.raises(_native.NativeError, match="-3"):
            b.fast_aggregate_verify_batch(idx, offs, b"".join(msgs), b"".join(sigs), ctx=fresh)
        assert b.fast_aggregate_verify_batch_keys(table, idx, offs, b"".join(msgs), b"".join(sigs), ctx=fresh).all()
        assert fresh.lib.bls_registry_size(fresh.h) == 0
    finally:
        fresh.close()
    # a loaded registry (other keys at the same indices) and committee table are left as they were
    c = _native.context()
    reg = b.Registry()
    reg.load(b"".join(pool[100:164]))
    com = b.Committees().load([[0, 1, 2], [3, 4, 5, 6]])
    rsig = _sign(b, [101 + 102 + 103, 104 + 105 + 106 + 107], msgs[:2])
    ridx, roffs = np.arange(7, dtype=np.uint32), np.array([0, 3, 7], dtype=np.uint64)
    bits = [np.ones(3, dtype=bool), np.ones(4, dtype=bool)]
    before = (len(reg), int(c.lib.bls_registry_generation(c.h)))
    assert b.fast_aggregate_verify_batch_keys(table, idx, offs, b"".join(msgs), b"".join(sigs)).all()
    assert (len(reg), int(c.lib.bls_registry_generation(c.h))) == before
    assert b.fast_aggregate_verify_batch(ridx, roffs, b"".join(msgs[:2]), b"".join(rsig)).all()
    assert b.fast_aggregate_verify_batch_bits(com, [0, 1], bits, b"".join(msgs[:2]), b"".join(rsig)).all()


def test_shared_messages(b, pool):
    B, M = 96, 5
    keys = pool[:B + 1]  # the last entry unused
    table = [_msg(b"kb5", m) for m in range(M)]
    mids = np.array([(3 * j) % M for j in range(B)], dtype=np.uint32)
    items = [[j] if j % 3 else [j, (j + 1) % B] for j in range(B)]
    msgs = [table[m] for m in mids]
    sigs = _sign(b, [sum(t + 1 for t in it) for it in items], msgs)
    sigs[17] = sigs[18]
    idx = np.array([t for it in items for t in it], dtype=np.uint32)
    offs = b.offsets_from_lengths([len(it) for it in items])
    plain = b.fast_aggregate_verify_batch_keys(b"".join(keys), idx, offs, b"".join(msgs), b"".join(sigs))
    assert b.batch_work() == (B, B + 64)
    shared = b.fast_aggregate_verify_batch_keys(b"".join(keys), idx, offs, b"".join(table), b"".join(sigs),
                                                msg_ids=mids)
    assert b.batch_work() == (M, M + 64)
    expect = np.ones(B, dtype=bool)
    expect[17] = False
    assert (plain == expect).all() and (shared == expect).all()
    with pytest.raises(ValueError):
        b.fast_aggregate_verify_batch_keys(b"".join(keys), idx, offs, b"".join(table), b"".join(sigs),
                                           msg_ids=np.full(B, M, dtype=np.uint32))


def test_profile_shows_the_key_table_stage(b, pool):
    """one key_validate launch per keys batch (the table's stage), one gather; an indexed batch records none"""
    msgs = [_msg(b"kbp", j) for j in range(5)]
    raw = b.sign_batch(b"".join((i + 1).to_bytes(32, "big") for i in range(5)), b"".join(msgs))
    pr = b.Profiler()
    pr.start()
    try:
        assert b.verify_batch_keys(b"".join(pool[:5]), b"".join(msgs), raw).all()
        got = pr.read()
    finally:
        pr.stop()
    assert got["key_validate"][1] == 1 and got["fav_gather"][1] == 1


@pytest.mark.parametrize("nbad", [1, 3])
def test_bisection(b, pool, nbad):
    B = 300
    msgs = [_msg(b"kb6", j) for j in range(B)]
    raw = bytearray(b.sign_batch(b"".join((i + 1).to_bytes(32, "big") for i in range(B)), b"".join(msgs)))
    where = [11, 150, 299][:nbad]
    for w in where:
        raw[96 * w: 96 * w + 96] = raw[96 * (w - 1): 96 * w]
    out = b.verify_batch_keys(b"".join(pool[:B]), b"".join(msgs), bytes(raw))
    expect = np.ones(B, dtype=bool)
    expect[where] = False
    assert (out == expect).all()
    checks, rounds = b.fallback_stats()
    assert checks > 0 and rounds > 0


@pytest.mark.parametrize("job0_bisects", [False, True])
def test_jobs_own_their_tables(b, pool, job0_bisects):
    """two batches with different tables and the same index lists, both submitted before either is finished: with
    one table slot for the context each would be judged against the other's keys"""
    B = 40
    idx = np.arange(B, dtype=np.uint32)
    offs = np.arange(B + 1, dtype=np.uint64)
    tabs = (pool[:B], pool[B: 2 * B])
    msgs = [_msg(b"kb7", j) for j in range(B)]
    expects, rbs = [], []
    for k, tab in enumerate(tabs):
        raw = bytearray(b.sign_batch(b"".join((k * B + i + 1).to_bytes(32, "big") for i in range(B)), b"".join(msgs)))
        e = np.ones(B, dtype=bool)
        if k == 0 and job0_bisects:
            raw[96 * 5: 96 * 6] = raw[96 * 6: 96 * 7]
            e[5] = False
        expects.append(e)
        rbs.append(b.ResidentFavBatch(idx, offs, b"".join(msgs), bytes(raw), keys=b"".join(tab)))
    try:
        for job, rb in enumerate(rbs):
            rb.submit(job, bytes([job + 1]) * 32)
        for job, rb in enumerate(rbs):
            ok = rb.job_check_own(job)
            assert ok == bool(expects[job].all())
            rb.job_finish(job, ok)
        for job, rb in enumerate(rbs):
            assert (rb.verdicts() == expects[job]).all(), job
    finally:
        for rb in rbs:
            rb.free()


def test_resident_keys_chunks_and_shared(b, pool):
    B, n = 24, 2
    idx = np.array([(2 * j + d) % 30 for j in range(B) for d in range(n)], dtype=np.uint32)
    offs = np.arange(B + 1, dtype=np.uint64) * n
    table = [_msg(b"kb8", m) for m in range(3)]
    mids = np.array([j % 3 for j in range(B)], dtype=np.uint32)
    msgs = [table[m] for m in mids]
    sigs = _sign(b, [int(idx[2 * j]) + int(idx[2 * j + 1]) + 2 for j in range(B)], msgs)
    sigs[20] = sigs[21]
    expect = np.ones(B, dtype=bool)
    expect[20] = False
    for kw, m in (({"chunks": 3}, msgs), ({"msg_ids": mids}, table)):
        rb = b.ResidentFavBatch(idx, offs, b"".join(m), b"".join(sigs), keys=b"".join(pool[:30]), **kw)
        try:
            assert (rb.run() == expect).all(), kw
        finally:
            rb.free()


SPEC_SRC = """
def check_fav(shim, pks, m, sig):
    assert shim.FastAggregateVerify(pks, m, sig)


def check_verify(shim, pk, m, sig):
    assert shim.Verify(pk, m, sig)
"""


def test_deferred_key_batches_without_a_registry(b, pool, monkeypatch):
    import linecache

    from bls_mi355x import bls as shim
    from bls_mi355x import sigsets

    linecache.cache["<key batch spec>"] = (len(SPEC_SRC), None, SPEC_SRC.splitlines(True), "<key batch spec>")
    ns = {}
    exec(compile(SPEC_SRC, "<key batch spec>", "exec"), ns)
    favs = [[0, 1, 2], [3, 4], [1, 5, 6, 7]]
    calls = []
    for j, it in enumerate(favs):
        m = _msg(b"kb9", j)
        calls.append(("fav", [pool[t] for t in it], m, _sign(b, [sum(t + 1 for t in it)], [m])[0]))
    for j in (8, 9):
        m = _msg(b"kb9v", j)
        calls.append(("verify", pool[j], m, _sign(b, [j + 1], [m])[0]))
    calls.append(("verify", pool[10], b"5byte", shim.Sign(11, b"5byte")))      # not a 32-byte root: av route
    calls.append(("fav", [pool[0][:47]], _msg(b"kb9", 99), calls[0][3]))       # malformed
    calls.append(("verify", pool[11], _msg(b"kb9v", 11), calls[3][3]))         # a wrong signature
    direct = [shim.FastAggregateVerify(p, m, s) if k == "fav" else shim.Verify(p, m, s) for k, p, m, s in calls]
    assert direct == [True] * 6 + [False, False]
    count = []
    real = b.fast_aggregate_verify_batch_keys
    monkeypatch.setattr(b, "fast_aggregate_verify_batch_keys",
                        lambda *a, **kw: count.append(len(a[2]) - 1) or real(*a, **kw))
    with sigsets.deferred(key_batches=True, check=False) as s:
        for k, p, m, sig in calls:
            (ns["check_fav"] if k == "fav" else ns["check_verify"])(shim, p, m, sig)
    assert len(s) == len(calls) and s.eager == 0
    assert s.results == direct
    assert count == [6]  # the six well-formed 32-byte sets, one batch
    assert b.batch_work() == (6, 6 + 64)


def _deposit_root(pk, wc, amount, domain):
    h = lambda x: hashlib.sha256(x).digest()
    pk_root = h(pk[:32] + pk[32:] + bytes(16))
    msg_root = h(h(pk_root + wc) + h(amount.to_bytes(8, "little") + bytes(24) + bytes(32)))
    return h(msg_root + domain)


@pytest.mark.parametrize("N", [1, 2, 65])
def test_deposits(b, pool, N):
    domain = bytes([3, 0, 0, 0]) + hashlib.sha256(b"fork").digest()[:28]
    amounts = [(0, 32 * 10 ** 9, 2 ** 64 - 1)[i % 3] for i in range(N)]
    wcs = [hashlib.sha256(b"wc" + bytes([i])).digest() for i in range(N)]
    pks = list(pool[:N])
    roots = [_deposit_root(pks[i], wcs[i], amounts[i], domain) for i in range(N)]
    sigs = _sign(b, [i + 1 for i in range(N)], roots)
    expect = np.ones(N, dtype=bool)
    if N == 65:
        sigs[3] = sigs[4]                                   # a bad signature
        pks[9] = bad_keys()["flag_0x40"]                    # a key that fails KeyValidate
        roots[9] = _deposit_root(pks[9], wcs[9], amounts[9], domain)
        amounts[19] += 1                                    # changed after signing
        roots[19] = _deposit_root(pks[19], wcs[19], amounts[19], domain)
        expect[[3, 9, 19]] = False
    out, got = b.verify_deposits(pks, wcs, amounts, sigs, domain, want_roots=True)
    assert got == roots
    assert (out == expect).all(), np.nonzero(out != expect)
    for i in range(min(N, 2)):
        assert OC.Verify(pks[i], roots[i], sigs[i]) is bool(expect[i])
    if N == 65:
        for i in (3, 9, 19):
            assert OC.Verify(pks[i], roots[i], sigs[i]) is False
