"""Host side of the shared-message batches: the segmented G1 sum's plan and per-lane fold (csrc/bls_g1_segsum.h)
in a host build with the digit form's column, value and subtraction checks compiled in (tests/hostcheck_segsum),
against the Python oracle's G1 arithmetic; batch.group_messages and the argument checks that precede any device
call; and the sigsets routing, with fakes in place of the batch executors."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

from oracle import bls_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "hostcheck_segsum")
LIB = os.path.join(DIR, "libhostcheck_segsum.so")
INC = os.path.join(os.path.dirname(HERE), "eth-consensus-specs_amd", "csrc")

_lib = None


def lib():
    global _lib
    if _lib is None:
        deps = [os.path.join(DIR, f) for f in ("hostcheck_segsum.cpp", "Makefile")]
        deps += [os.path.join(INC, f) for f in os.listdir(INC) if f.endswith(".h")]
        if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(d) for d in deps):
            subprocess.check_call(["make", "-C", DIR], timeout=2400)
        _lib = ctypes.CDLL(LIB)
        _lib.hc_seg_k.restype = ctypes.c_uint32
        _lib.hc_seg_sum.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_char_p,
                                    ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p]
    return _lib


def seg_sum(ids, M, points, status):
    """(rc, sums, ok, info): the host build's plan + fold over affine points (x, y); sums[m] is None for the
    identity."""
    B = len(ids)
    a_ids = np.ascontiguousarray(ids, dtype=np.uint32)
    a_st = np.ascontiguousarray(status, dtype=np.int32)
    rp = b"".join(p[0].to_bytes(48, "big") + p[1].to_bytes(48, "big") for p in points)
    out = ctypes.create_string_buffer(96 * max(M, 1))
    ok = np.full(max(M, 1), -1, dtype=np.int32)
    info = np.zeros(3, dtype=np.uint32)
    rc = lib().hc_seg_sum(a_ids.ctypes.data, B, M, rp, a_st.ctypes.data, out, ok.ctypes.data, info.ctypes.data)
    sums = []
    for m in range(M):
        raw = out.raw[96 * m: 96 * m + 96]
        sums.append(None if raw == bytes(96) else (int.from_bytes(raw[:48], "big"), int.from_bytes(raw[48:], "big")))
    return rc, sums, ok[:M].tolist(), info.tolist()


def test_plan_and_fold_match_oracle():
    """Groups of 1, 2, K-1, K, K+1, K^2 and K^2+1 random multiples of G1 in one shuffled batch, with some
    status-0 items, a group whose items are all status 0, a group holding P and -P (the identity, flagged) and
    an unused table entry: every group's sum equals the oracle's, ok marks exactly the non-identity sums."""
    K = lib().hc_seg_k()
    rng = random.Random(0x5E65)
    sizes = [1, 2, K - 1, K, K + 1, K * K, K * K + 1, 3, 2, 0]  # 7: all rejected; 8: P and -P; 9: unused
    M = len(sizes)
    ids = [m for m, s in enumerate(sizes) for _ in range(s)]
    rng.shuffle(ids)
    B = len(ids)
    # random multiples of G1 by a running sum (one oracle addition per item)
    step = O.g1_mul(O.G1_GEN, rng.randrange(1, O.R))
    pts, cur = [], O.g1_mul(O.G1_GEN, rng.randrange(1, O.R))
    for _ in range(B):
        pts.append(cur)
        cur = O.g1_add(cur, step)
    status = [1] * B
    for i in range(B):
        if ids[i] == 7 or (ids[i] in (4, 5, 6) and rng.random() < 0.1):
            status[i] = 0
    a, b = [i for i in range(B) if ids[i] == 8]
    pts[b] = (pts[a][0], (-pts[a][1]) % O.P)
    rc, sums, ok, info = seg_sum(ids, M, pts, status)
    assert rc == 0
    expect = [None] * M
    for i in range(B):
        if status[i]:
            expect[ids[i]] = O.g1_add(expect[ids[i]], pts[i])
    assert expect[7] is None and expect[8] is None and expect[9] is None and expect[6] is not None
    assert sums == expect
    assert ok == [0 if e is None else 1 for e in expect]
    # K^2 + 1 entries need three levels; level 0 writes one partial per run of the groups longer than K
    assert info[0] == 3
    assert info[2] == sum(-(-s // K) for s in sizes if s > K)


def test_plan_single_level_and_rejections():
    K = lib().hc_seg_k()
    g = O.G1_GEN
    # all singletons: one level, one run per item, no partials
    rc, sums, ok, info = seg_sum([2, 0, 1], 3, [g, g, g], [1, 1, 1])
    assert rc == 0 and sums == [g, g, g] and ok == [1, 1, 1] and info == [1, 3, 0]
    # one group of exactly K: still one level
    rc, sums, ok, info = seg_sum([0] * K, 1, [g] * K, [1] * K)
    assert rc == 0 and sums == [O.g1_mul(g, K)] and info == [1, 1, 0]
    # id >= M, and an empty table with items
    assert seg_sum([0, 3], 3, [g, g], [1, 1])[0] == -1
    assert seg_sum([0], 0, [g], [1])[0] == -1
    # an empty batch over a table: every entry is the identity
    rc, sums, ok, info = seg_sum([], 2, [], [])
    assert rc == 0 and sums == [None, None] and ok == [0, 0]


def test_group_messages_round_trip():
    from bls_mi355x import batch

    a, b, c = b"\x01" * 32, b"\x02" * 32, b"\x03" * 32
    msgs = [b, a, b, b, c, a]
    table, ids = batch.group_messages(b"".join(msgs))
    assert table == b + a + c  # first-occurrence order
    assert ids.dtype == np.uint32 and ids.tolist() == [0, 1, 0, 0, 2, 1]
    assert [table[32 * m: 32 * m + 32] for m in ids] == msgs
    t0, i0 = batch.group_messages(b"")
    assert t0 == b"" and i0.size == 0 and i0.dtype == np.uint32
    with pytest.raises(ValueError):
        batch.group_messages(b"\x00" * 33)


class _NoDevice:
    """a context whose use fails the test: the argument checks must come first"""

    def __getattr__(self, name):
        raise AssertionError("device call before the argument check")


def test_bad_ids_rejected_before_any_device_call():
    from bls_mi355x import batch

    idx = np.arange(3, dtype=np.uint32)
    offs = np.arange(4, dtype=np.uint64)
    sigs = bytes(96 * 3)
    table = bytes(64)  # M = 2
    nd = _NoDevice()
    with pytest.raises(ValueError):  # msg_id >= M
        batch.verify_batch_shared(idx, table, [0, 2, 1], sigs, ctx=nd)
    with pytest.raises(ValueError):
        batch.fast_aggregate_verify_batch_shared(idx, offs, table, [0, 1, 2], sigs, ctx=nd)
    with pytest.raises(ValueError):  # M == 0
        batch.verify_batch_shared(idx, b"", [0, 0, 0], sigs, ctx=nd)
    with pytest.raises(ValueError):
        batch.fast_aggregate_verify_batch_shared(idx, offs, b"", [0, 0, 0], sigs, ctx=nd)
    with pytest.raises(ValueError):  # negative, one id short, not integers
        batch.verify_batch_shared(idx, table, [0, -1, 1], sigs, ctx=nd)
    with pytest.raises(ValueError):
        batch.verify_batch_shared(idx, table, [0, 1], sigs, ctx=nd)
    with pytest.raises(ValueError):
        batch.verify_batch_shared(idx, table, [0.0, 1.0, 1.0], sigs, ctx=nd)
    with pytest.raises(ValueError):  # the pipelined form: bad id, and chunks with msg_ids
        batch.ResidentFavBatch(idx, offs, table, sigs, ctx=nd, msg_ids=[0, 1, 2])
    with pytest.raises(ValueError):
        batch.ResidentFavBatch(idx, offs, table, sigs, ctx=nd, chunks=3, msg_ids=[0, 1, 1])


class FakeRegistry:
    def __init__(self, keys):
        self.map = {k: i for i, k in enumerate(keys)}

    def indices(self, pubkeys):
        try:
            return np.array([self.map[bytes(k)] for k in pubkeys], dtype=np.uint32)
        except KeyError:
            return None


def _pk(i):
    return bytes([0x80 | (i & 0x1f)]) + i.to_bytes(47, "big")


@pytest.fixture
def fakes(monkeypatch):
    from bls_mi355x import batch, sigsets

    calls = []

    def fav(idx, offs, msgs, sigs, ctx=None):
        calls.append(("fav", np.asarray(idx).tolist(), np.asarray(offs).tolist(), bytes(msgs), bytes(sigs)))
        return np.ones(len(offs) - 1, dtype=bool)

    def shared(idx, offs, table, ids, sigs, ctx=None):
        calls.append(("shared", np.asarray(idx).tolist(), np.asarray(offs).tolist(), bytes(table),
                      np.asarray(ids).tolist(), bytes(sigs)))
        return np.ones(len(offs) - 1, dtype=bool)

    monkeypatch.setattr(batch, "fast_aggregate_verify_batch", fav)
    monkeypatch.setattr(batch, "fast_aggregate_verify_batch_shared", shared)
    return sigsets, calls


def _fill(s, keys, msgs):
    sigs = []
    for j, m in enumerate(msgs):
        sig = bytes([j + 1]) * 96
        sigs.append(sig)
        if j % 2:
            s.add_verify(keys[j], m, sig)
        else:
            s.add_fast_aggregate_verify(keys[j: j + 2], m, sig)
    return b"".join(sigs)


def test_sigsets_routing_shared_and_default(fakes):
    sigsets, calls = fakes
    keys = [_pk(i) for i in range(8)]
    a, b = b"\x0a" * 32, b"\x0b" * 32
    repeated = [a, b, a, a, b]
    want_idx, want_offs = [0, 1, 1, 2, 3, 3, 4, 5], [0, 2, 3, 5, 6, 8]
    # share_messages with repeated messages: the shared executor, first-occurrence table and the ids
    s = sigsets.SignatureSets(FakeRegistry(keys), share_messages=True)
    sigs = _fill(s, keys, repeated)
    assert s.verify() == [True] * 5
    assert calls == [("shared", want_idx, want_offs, a + b, [0, 1, 0, 0, 1], sigs)]
    # the default: today's executor with today's arguments
    calls.clear()
    s = sigsets.SignatureSets(FakeRegistry(keys))
    sigs = _fill(s, keys, repeated)
    assert s.verify() == [True] * 5
    assert calls == [("fav", want_idx, want_offs, b"".join(repeated), sigs)]
    # share_messages with all-distinct messages: nothing to share, today's call
    calls.clear()
    distinct = [bytes([0x10 + j]) * 32 for j in range(5)]
    s = sigsets.SignatureSets(FakeRegistry(keys), share_messages=True)
    sigs = _fill(s, keys, distinct)
    assert s.verify() == [True] * 5
    assert calls == [("fav", want_idx, want_offs, b"".join(distinct), sigs)]


def test_deferred_passes_share_messages(fakes):
    sigsets, calls = fakes
    with sigsets.deferred(FakeRegistry([_pk(0)]), share_messages=True) as col:
        pass
    assert col.share_messages is True and col.results == []
    with sigsets.deferred(FakeRegistry([_pk(0)])) as col:
        pass
    assert col.share_messages is False
