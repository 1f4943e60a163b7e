"""Host logic of the key-table batches (no device): batch.key_table's dedupe and offsets, the routing of
SignatureSets(key_batches=...) with fake executors, and the header declaring every new function _native.py binds."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FUNCTIONS = ("bls_fav_batch_keys", "bls_verify_batch_keys", "bls_fav_job_submit_keys_dev", "bls_deposits_verify")


def _pk(i):
    return bytes([0x80 | (i & 0x1f)]) + i.to_bytes(47, "big")


def test_key_table_dedupes_in_first_occurrence_order():
    from bls_mi355x import batch

    a, b, c, d = (_pk(i) for i in range(4))
    table, idx, offs = batch.key_table([[a, b, a], [], [c, b], [d], [a, a]])
    assert table == a + b + c + d
    assert idx.dtype == np.uint32 and idx.tolist() == [0, 1, 0, 2, 1, 3, 0, 0]  # a repeat inside a list stays
    assert offs.dtype == np.uint64 and offs.tolist() == [0, 3, 3, 5, 6, 8]
    table, idx, offs = batch.key_table([])
    assert table == b"" and idx.size == 0 and offs.tolist() == [0]
    with pytest.raises(ValueError):
        batch.key_table([[a[:47]]])


class FakeRegistry:
    def __init__(self, keys):
        self.map = {k: i for i, k in enumerate(keys)}

    def indices(self, pubkeys):
        try:
            return np.array([self.map[bytes(k)] for k in pubkeys], dtype=np.uint32)
        except KeyError:
            return None


@pytest.fixture
def fakes(monkeypatch):
    from bls_mi355x import batch, sigsets
    from bls_mi355x.backend import mi355x_bls

    calls = {"single": []}

    def fav(idx, offs, msgs, sigs, ctx=None):
        calls["fav"] = (np.asarray(idx).tolist(), np.asarray(offs).tolist())
        return np.ones(len(offs) - 1, dtype=bool)

    def av(pks, msgs, sigs, ctx=None):
        calls["av"] = [len(p) for p in pks]
        return np.array([len(p) == len(m) for p, m in zip(pks, msgs)])

    def keys(table, idx, offs, msgs, sigs, msg_ids=None, ctx=None, want_key_valid=False):
        assert "keys" not in calls  # ONE batch
        calls["keys"] = (len(table) // 48, np.asarray(idx).tolist(), np.asarray(offs).tolist(), len(msgs) // 32,
                         None if msg_ids is None else np.asarray(msg_ids).tolist())
        return np.ones(len(offs) - 1, dtype=bool)

    def single(pks, m, s):
        calls["single"].append(len(pks))
        return len(pks) > 0

    monkeypatch.setattr(batch, "fast_aggregate_verify_batch", fav)
    monkeypatch.setattr(batch, "aggregate_verify_batch", av)
    monkeypatch.setattr(batch, "fast_aggregate_verify_batch_keys", keys)
    monkeypatch.setattr(mi355x_bls, "FastAggregateVerify", staticmethod(single))
    return sigsets, calls


def _fill(s, keys):
    m32, m32b, sig = b"\x01" * 32, b"\x03" * 32, b"\x02" * 96
    s.add_fast_aggregate_verify(keys[:3], m32, sig)                 # 0 indexed
    s.add_verify(_pk(100), m32, sig)                                # 1 av (not resident)        -> keys
    s.add_verify(keys[0], b"short", sig)                            # 2 av (not a 32-byte root)
    s.add_aggregate_verify(keys[:2], [m32, m32], sig)               # 3 av
    s.add_fast_aggregate_verify(None, m32, sig)                     # 4 malformed -> False
    s.add_fast_aggregate_verify([], m32, sig)                       # 5 single (empty)
    s.add_fast_aggregate_verify([_pk(100), _pk(101)], m32b, sig)    # 6 single (not resident)    -> keys
    s.add_fast_aggregate_verify([_pk(101), keys[1]], m32, sig)      # 7 single (one not resident) -> keys
    s.add_fast_aggregate_verify([keys[1]], b"x" * 33, sig)          # 8 single (33-byte message)


def test_flag_off_is_todays_routing(fakes):
    sigsets, calls = fakes
    keys = [_pk(i) for i in range(8)]
    s = sigsets.SignatureSets(FakeRegistry(keys))
    assert s.key_batches is False
    _fill(s, keys)
    indexed, av, single = s.plan()
    assert [i for i, _ in indexed] == [0] and av == [1, 2, 3] and single == [5, 6, 7, 8]
    out = s.verify()
    assert "keys" not in calls
    assert calls["fav"] == ([0, 1, 2], [0, 3]) and calls["av"] == [1, 1, 2] and calls["single"] == [0, 2, 2, 1]
    assert out == [True, True, True, True, False, False, True, True, True]


@pytest.mark.parametrize("share", [False, True])
def test_flag_on_moves_the_32_byte_sets_to_one_keys_batch(fakes, share):
    sigsets, calls = fakes
    keys = [_pk(i) for i in range(8)]
    s = sigsets.SignatureSets(FakeRegistry(keys), share_messages=share, key_batches=True)
    _fill(s, keys)
    plan_on = s.plan()
    off = sigsets.SignatureSets(FakeRegistry(keys))
    _fill(off, keys)
    plan_off = off.plan()
    assert [i for i, _ in plan_on[0]] == [i for i, _ in plan_off[0]] and plan_on[1:] == plan_off[1:]  # plan() unchanged
    out = s.verify()
    # sets 1, 6, 7 in set order; table = pk100, pk101, keys[1] in order of first occurrence
    K, idx, offs, nmsg, mids = calls["keys"]
    assert (K, idx, offs) == (3, [0, 0, 1, 1, 2], [0, 1, 3, 5])
    assert (nmsg, mids) == ((2, [0, 1, 0]) if share else (3, None))
    assert calls["fav"] == ([0, 1, 2], [0, 3])
    assert calls["av"] == [1, 2] and calls["single"] == [0, 1]  # sets 2, 3 and 5, 8 keep their routes
    assert out == [True, True, True, True, False, False, True, True, True]


def test_deferred_passes_the_flag(fakes):
    sigsets, _ = fakes
    with sigsets.deferred(key_batches=True, check=False) as s:
        assert s.key_batches is True and s.registry is None
    with sigsets.deferred(check=False) as s:
        assert s.key_batches is False


def test_header_declares_what_native_binds():
    from bls_mi355x import _native

    with open(os.path.join(ROOT, "include", "blsmi355x.h")) as fh:
        hdr = fh.read()
    for name in NEW_FUNCTIONS:
        assert name in _native._SIGS, name
        m = re.search(r"^int %s\(([^;]*)\);" % name, hdr, re.M)
        assert m, name
        assert len(m.group(1).split(",")) == len(_native._SIGS[name][1]), name  # one ctypes type per C parameter
    lib = _native.load_library()
    for name in NEW_FUNCTIONS:
        assert hasattr(lib, name), name
