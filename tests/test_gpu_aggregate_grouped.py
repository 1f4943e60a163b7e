"""GPU tests of grouped signature aggregation (bls_aggregate_grouped / bls_aggregate_grouped_dev):
B signatures into G aggregates through the segmented G2 sum of csrc/bls_g2_segsum.h.  Aggregates are known by
construction (members of a group sign one root, so the aggregate is the signature of the summed key), compared with
the per-call Aggregate, the C oracle and the Python oracle's curve arithmetic.  Requires an MI355X."""
import ctypes
import hashlib

import numpy as np
import pytest

from oracle import bls_oracle as O
from oracle import bls_oracle_c as OC

pytestmark = pytest.mark.gpu

N_REG = 1024
G2_INF = b"\xc0" + bytes(95)


@pytest.fixture(scope="module")
def batch():
    from bls_mi355x import batch as b
    return b


@pytest.fixture(scope="module")
def shim():
    from bls_mi355x import bls as s
    s.use_mi355x()
    s.bls_active = True
    return s


def _root(tag, m):
    return hashlib.sha256(b"grouped" + tag + m.to_bytes(8, "little")).digest()


def _sign(batch, sks, msgs):
    return batch.sign_batch(b"".join(int(s).to_bytes(32, "big") for s in sks), b"".join(msgs))


def _sig(sigs, i):
    return bytes(sigs[96 * i: 96 * i + 96])


def _neg(sig):
    """the encoding of -sigma: the sign bit of y flipped"""
    return bytes([sig[0] ^ 0x20]) + sig[1:]


def _non_g2():
    q = O.iso_map(O.map_to_curve_sswu((5, 7)))  # on E2, outside G2: decodes, fails the subgroup check
    assert not O.g2_in_subgroup(q)
    return q


def _oc_aggregate(members):
    """(ok, bytes) of the C oracle's Aggregate; raise = ok 0"""
    try:
        return OC.Aggregate(members)
    except ValueError:
        return None


def test_levels_and_launch_edges(batch, shim):
    """Group sizes [0, 1, 2, 15, 16, 17, 256, 257, 3] plus 130 singletons, shuffled: B = 697, G = 139 (no multiple
    of 8 or 64), more than 128 level-0 runs, three fold levels."""
    sizes = [0, 1, 2, 15, 16, 17, 256, 257, 3] + [1] * 130
    G = len(sizes)
    ids = np.repeat(np.arange(G, dtype=np.uint32), sizes)
    np.random.default_rng(7).shuffle(ids)
    B = ids.size
    assert (B, G) == (697, 139)
    rng = np.random.default_rng(8)
    sks = [int.from_bytes(rng.bytes(31), "big") + 1 for _ in range(B)]
    roots = [_root(b"lv", g) for g in range(G)]
    sigs = _sign(batch, sks, [roots[g] for g in ids])
    got = batch.aggregate_grouped(sigs, ids, n_groups=G)
    assert len(got) == G and got[0] is None
    members = [[i for i in range(B) if ids[i] == g] for g in range(G)]
    agg_sk = [sum(sks[i] for i in members[g]) % O.R for g in range(1, G)]
    expect = _sign(batch, agg_sk, roots[1:])
    for g in range(1, G):
        assert got[g] == _sig(expect, g - 1), g
        assert got[g] == shim.Aggregate([_sig(sigs, i) for i in members[g]]), g
        if sizes[g] <= 17:
            assert got[g] == OC.Aggregate([_sig(sigs, i) for i in members[g]]), g
    # n_groups defaults to max(id) + 1
    assert batch.aggregate_grouped(sigs, ids) == got


@pytest.fixture(scope="module")
def semantics(batch):
    """12 groups: even ones are three good signatures; the odd ones hold one special case each among good members.
    Returns (sigs, ids, G, bad items by group)."""
    cases = ["zero", "ff_tail", "non_g2", "inf_member", "duplicate", "sigma_neg_sigma"]
    G = 2 * len(cases)
    ids, sks = [], []
    for g in range(G):
        n = 2 if g == 11 else 3
        ids += [g] * n
    rng = np.random.default_rng(21)
    sks = [int.from_bytes(rng.bytes(31), "big") + 1 for _ in ids]
    sigs = bytearray(_sign(batch, sks, [_root(b"sem", g) for g in ids]))
    first = {g: ids.index(g) for g in range(G)}
    i = first[1]
    sigs[96 * i: 96 * i + 96] = bytes(96)
    i = first[3] + 1
    sigs[96 * i + 92: 96 * i + 96] = b"\xff" * 4
    i = first[5] + 2
    sigs[96 * i: 96 * i + 96] = O.g2_compress(_non_g2())
    i = first[7] + 1
    sigs[96 * i: 96 * i + 96] = G2_INF
    i = first[9]
    sigs[96 * (i + 2): 96 * (i + 3)] = sigs[96 * i: 96 * i + 96]
    i = first[11]
    sigs[96 * (i + 1): 96 * (i + 2)] = _neg(_sig(sigs, i))
    # interleave the groups so that none is contiguous
    perm = np.random.default_rng(22).permutation(len(ids))
    p_ids = np.asarray(ids, dtype=np.uint32)[perm]
    p_sigs = b"".join(_sig(sigs, int(j)) for j in perm)
    where = {int(j): k for k, j in enumerate(perm)}
    bad = {1: where[first[1]], 3: where[first[3] + 1], 5: where[first[5] + 2]}
    return p_sigs, p_ids, G, bad


def _members(sigs, ids, g, include=None):
    return [_sig(sigs, i) for i in range(len(ids)) if ids[i] == g and (include is None or include[i])]


def test_semantics_checked(batch, semantics):
    """Each group's (ok, bytes) is the C oracle's Aggregate of its members: the three bad members spoil only their
    own groups, the infinity member and the duplicate are accepted, sigma + -sigma is ok with c0 00.."""
    sigs, ids, G, bad = semantics
    got = batch.aggregate_grouped(sigs, ids, n_groups=G)
    for g in range(G):
        assert got[g] == _oc_aggregate(_members(sigs, ids, g)), g
    assert [g for g in range(G) if got[g] is None] == [1, 3, 5]
    assert got[11] == G2_INF
    assert got[7] is not None and got[9] is not None


def test_mask(batch, semantics):
    """Excluding the bad members makes their groups the aggregate of the rest; a fully excluded group is not ok;
    an excluded member's bytes are never judged."""
    sigs, ids, G, bad = semantics
    include = np.ones(len(ids), dtype=np.uint8)
    for i in bad.values():
        include[i] = 0
    include[ids == 4] = 0
    got = batch.aggregate_grouped(sigs, ids, n_groups=G, include=include)
    for g in range(G):
        assert got[g] == _oc_aggregate(_members(sigs, ids, g, include)), g
    assert [g for g in range(G) if got[g] is None] == [4]
    garbled = bytearray(sigs)
    for k, i in enumerate(list(bad.values()) + [int(np.nonzero(ids == 4)[0][0])]):
        garbled[96 * i: 96 * i + 96] = bytes([0x11 * (k + 1)]) * 96
    assert batch.aggregate_grouped(bytes(garbled), ids, n_groups=G, include=include) == got
    # a boolean mask is the same mask
    assert batch.aggregate_grouped(sigs, ids, n_groups=G, include=include.astype(bool)) == got


def test_unchecked_sum_outside_g2(batch):
    """subgroup_check = 0: a group holding a point of E2 outside G2 and two good signatures is the Python oracle's
    sum of the three curve points; the checked call refuses that group only."""
    sks = [5, 6, 7, 8]
    sigs = bytearray(_sign(batch, sks, [_root(b"un", 0)] * 2 + [_root(b"un", 1)] * 2))
    q = _non_g2()
    all_sigs = bytes(sigs[:96]) + O.g2_compress(q) + bytes(sigs[96:])
    ids = [0, 0, 0, 1, 1]
    got = batch.aggregate_grouped(all_sigs, ids, subgroup_check=False)
    s = O.g2_add(O.g2_add(O.g2_decompress(_sig(sigs, 0)), q), O.g2_decompress(_sig(sigs, 1)))
    assert got[0] == O.g2_compress(s)
    assert got[1] == OC.Aggregate([_sig(sigs, 2), _sig(sigs, 3)])
    assert batch.aggregate_grouped(all_sigs, ids) == [None, got[1]]


def test_verify_then_aggregate_then_verify(batch):
    """A registry of 1,024 keys, 300 Verify items on 5 roots with three corrupted items: the aggregates of the
    accepted items (mask = the batch's verdicts, no second subgroup check) pass FastAggregateVerify over each
    root's accepted keys, and the resident batch's aggregate_by_message returns the same bytes from HBM."""
    reg = batch.Registry()
    reg.generate(N_REG, first_sk=1)
    M, B = 5, 300
    table = [_root(b"vav", m) for m in range(M)]
    ids = np.repeat(np.arange(M, dtype=np.uint32), [1, 9, 40, 100, 150])
    np.random.default_rng(31).shuffle(ids)
    idx = np.random.default_rng(32).choice(np.arange(N_REG), size=B, replace=False).astype(np.uint32)
    sigs = bytearray(_sign(batch, [int(k) + 1 for k in idx], [table[m] for m in ids]))
    corrupted = [17, 140, 299]
    sigs[96 * 17: 96 * 18] = _sign(batch, [int(idx[17]) + 1], [table[(int(ids[17]) + 1) % M]])  # wrong message
    sigs[96 * 140: 96 * 141] = bytes(96)                                                       # undecodable
    sigs[96 * 299: 96 * 300] = O.g2_compress(_non_g2())                                       # outside G2
    verdicts = batch.verify_batch_shared(idx, b"".join(table), ids, bytes(sigs))
    assert sorted(np.nonzero(~verdicts)[0].tolist()) == corrupted
    aggs = batch.aggregate_grouped(bytes(sigs), ids, n_groups=M, include=verdicts, subgroup_check=False)
    assert all(a is not None for a in aggs)
    flat, lens = [], []
    for m in range(M):
        acc = [int(idx[i]) for i in range(B) if ids[i] == m and verdicts[i]]
        flat += acc
        lens.append(len(acc))
    out = batch.fast_aggregate_verify_batch(np.asarray(flat, dtype=np.uint32), batch.offsets_from_lengths(lens),
                                            b"".join(table), b"".join(aggs))
    assert out.all(), out
    rb = batch.ResidentFavBatch(idx, np.arange(B + 1, dtype=np.uint64), b"".join(table), bytes(sigs), msg_ids=ids)
    v = rb.run()
    assert (v == verdicts).all()
    assert rb.aggregate_by_message() == aggs
    # a caller's mask, with the subgroup check: the undecodable item now spoils its group, the others stand
    every = np.ones(B, dtype=bool)
    every[17] = every[299] = False
    by_mask = rb.aggregate_by_message(include=every, subgroup_check=True)
    assert [m for m in range(M) if by_mask[m] is None] == [int(ids[140])]
    assert all(by_mask[m] == aggs[m] for m in range(M) if m != int(ids[140]))
    rb.free()


def test_c_level_refusals(batch):
    from bls_mi355x import _native

    c = _native.context()
    sigs = np.frombuffer(_sign(batch, [3, 4], [_root(b"c", 0)] * 2), dtype=np.uint8)
    out = np.full(96 * 2, 0xEE, dtype=np.uint8)
    ok = np.full(2, 0xEE, dtype=np.uint8)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    ids = np.array([0, 2], dtype=np.uint32)
    d = batch.DeviceBuffer(c, sigs)
    d_out = batch.DeviceBuffer(c, nbytes=97 * 2)
    for fn, s, o, k in ((c.lib.bls_aggregate_grouped, p(sigs), p(out), p(ok)),
                        (c.lib.bls_aggregate_grouped_dev, d.ptr, d_out.ptr, d_out.ptr + 192)):
        assert fn(c.h, s, 2, p(ids), 2, None, 1, o, k) == _native.BLS_E_ARG  # an id >= G
        assert fn(c.h, s, 2, p(ids), 0, None, 1, o, k) == _native.BLS_E_ARG  # no groups, two signatures
        assert fn(c.h, s, 0, p(ids), 2, None, 1, o, k) == 1                   # an empty batch: every group not ok
    assert (out == 0).all() and (ok == 0).all()
    assert (d_out.to_host() == 0).all()
    assert batch.aggregate_grouped(b"", [], n_groups=3) == [None] * 3
    assert batch.aggregate_grouped(b"", []) == []
    d.free()
    d_out.free()


def test_grouped_between_job_partial_and_finish(batch):
    """A grouped aggregation on job 0 while a job-0 FAV batch sits between its partial and finish steps must not
    touch that batch's state: finish still rejects exactly the bad item (its bisection reads the batch's r_i apk_i
    and signatures back)."""
    reg = batch.Registry()
    reg.generate(N_REG, first_sk=1)
    B, n = 10, 8
    idx = np.random.default_rng(41).choice(np.arange(N_REG), size=(B, n), replace=False).astype(np.uint32)
    agg = [int(a) % O.R for a in (idx.astype(np.int64) + 1).sum(axis=1)]
    msgs = [_root(b"iso", j) for j in range(B)]
    sigs = bytearray(_sign(batch, agg, msgs))
    sigs[96 * 3: 96 * 4] = sigs[96 * 4: 96 * 5]  # item 3 invalid: the finish step bisects
    rb = batch.ResidentFavBatch(idx.reshape(-1), np.arange(B + 1, dtype=np.uint64) * n, b"".join(msgs), bytes(sigs))
    rb.submit(0, b"\x09" * 32)
    ok = rb.job_check(0, rb.job_partial(0))
    assert ok is False
    ids = [0, 1, 0, 1, 0, 1, 0, 1, 0, 1]
    got = batch.aggregate_grouped(bytes(sigs), ids)
    assert got == [OC.Aggregate([_sig(sigs, i) for i in range(B) if ids[i] == g]) for g in (0, 1)]
    rb.job_finish(0, ok)
    v = rb.verdicts()
    assert list(v) == [True] * 3 + [False] + [True] * 6
    rb.free()
