"""GPU tests of bls_g1_table_msm at the row counts where the call changes shape (tests/seam_sizes.py): one and two
scan blocks, one and two blocks of the final kernels, a full round of k_g1m_scan_top and a second round with its
carry.  Every row of every call has a known answer: the table holds [c] G for known c, the scalars are full-width
and pseudo-random but for the last of a row, which makes the row sum to [v + 1] G (g1_table_edge_inputs.
rows_with_known_sums), so the expected bytes are running sums of G by the oracle.  Each row's 48 bytes are compared,
and batch.g1_table_stats must advance by one call and by the non-zero bytes of the scalars, counted here."""
import ctypes
import random

import numpy as np
import pytest

import g1_table_edge_inputs as E
import seam_sizes as Z
from oracle import bls_oracle as O

pytestmark = pytest.mark.gpu

R = O.R
CROSS_N = 65  # the distinct Lagrange points of the cross-check with bls_multi_exp


@pytest.fixture(scope="module")
def batch():
    from bls_mi355x import batch as b

    return b


@pytest.fixture(scope="module")
def table(batch):
    """[c] G for c in E.LOGS at entries 0..2, then 65 Lagrange points of the fixture: one table for the module"""
    t = batch.G1Table()
    pts = E.known_log_table() + E.trusted_setup()[0][:CROSS_N]
    assert t.load(pts).all() and len(t) == 3 + CROSS_N
    return t


def stats(batch):
    return np.array(batch.g1_table_stats(), dtype=np.int64)


def special_rows(B, last_empty):
    """rows whose sum is the identity with non-zero scalars (a status-0 item of launch_g1_affine's batched inversion
    among live ones: first, on both sides of the 64-row block, last) and rows of zeros (256 empty buckets that share
    an offset with their successor: interior, across a scan block's end, near the end).  The last row is of the
    first kind, or with last_empty of the second: the call then ends in empty buckets."""
    zero_sum = {0, Z.FINAL_LANES - 1, Z.FINAL_LANES, B - 2 if last_empty else B - 1}
    empty = {2, Z.ROWS_PER_SCAN_BLK - 1, Z.ROWS_PER_SCAN_BLK, 33, B - 1 if last_empty else B - 3}
    return zero_sum - empty, empty


def run_case(batch, table, B, idx, seed, special=None):
    """special: None, or whether the last row is all zeros (special_rows)"""
    zero_sum, empty = special_rows(B, special) if special is not None else (set(), set())
    rows, want, nonzero = E.rows_with_known_sums(B, idx, seed, zero_sum, empty)
    assert len(want) == B and min(max(r) for v, r in enumerate(rows) if v not in empty).bit_length() > 200
    s0 = stats(batch)
    got = batch.g1_lincomb_batch(table, idx, rows)
    d = stats(batch) - s0
    assert len(got) == B
    wrong = [v for v in range(B) if got[v] != want[v]]
    assert not wrong, "B = %d: %d rows differ, the first at %d: %s != %s" % (
        B, len(wrong), wrong[0], got[wrong[0]].hex(), want[wrong[0]].hex())
    assert d.tolist() == [1, nonzero, 0]
    if special is not None:
        assert all(got[v] == E.G1_INF for v in zero_sum | empty) and got[1] != E.G1_INF


@pytest.mark.parametrize("B", Z.MSM_ROWS)
def test_every_row_of_a_many_row_call(batch, table, B):
    """n = 2 (G and [a] G), B = 4, 5 (one / two scan blocks of 1,024 counters), 64, 65 (one / two blocks of
    k_g1m_final and k_g1m_compress), 256, 257, and 1,024, 1,025 (256 / 257 scan blocks: one round of k_g1m_scan_top,
    then a second with the carry).  The largest case is about scan blocks, not memory: for B = 1,025, n = 2
    g1_msm_plan gives slots = 256 B = 262,400, entries = 32 n B = 65,600, two levels with level_runs =
    65,600 / 16 + 255 B = 265,475 and ceil(265,475 / 16) + 255 B = 277,968 partials (144 bytes each: 38 MB and
    40 MB), and u32_words = 5 * 262,400 + 3 + 257 + 1 + 65,600 = 1,377,861 (5.5 MB)."""
    run_case(batch, table, B, [0, 1], 0x5EA0 + B)


@pytest.mark.parametrize("B", Z.MSM_ROWS_SPECIAL)
def test_identity_and_empty_rows_among_live_rows(batch, table, B):
    """B = 65, 257, 1,025 with rows 0, 63, 64 and B - 1 summing to the identity under non-zero scalars, and rows 2,
    3, 4, 33 and B - 3 all zeros (rows 3 | 4 end and begin a scan block); then with the last row all zeros and the
    one before it summing to the identity"""
    run_case(batch, table, B, [0, 1], 0x1DE0 + B, special=False)
    run_case(batch, table, B, [0, 1], 0x2DE0 + B, special=True)


def test_second_fold_level_over_a_multi_block_scan(batch, table):
    """n = K + 1 = 17 entries naming three table points again and again, B = 257: a bucket can hold more than one
    run, so a second fold level exists while every scan of the call has 65 blocks; identity and empty rows as above"""
    n = E.K + 1
    idx = [i % 3 for i in range(n)]
    run_case(batch, table, Z.MSM_ROWS_DEEP, idx, 0xDEE9, special=False)
    run_case(batch, table, Z.MSM_ROWS_DEEP, idx, 0xDEEB, special=True)
    # every scalar of a row equal: each window's 17 entries share one bucket, which a second level must finish
    # (two runs of its 17 items).  k_v = (v + 1) / (sum of the 17 logarithms): row v sums to [v + 1] G again
    B = Z.MSM_ROWS_DEEP
    inv = pow(sum(E.LOGS[e] for e in idx) % R, -1, R)
    ks = [(v + 1) * inv % R for v in range(B)]
    assert min(ks).bit_length() > 200
    want, acc = [], None
    for _ in range(B):
        acc = O.g1_add(acc, O.G1_GEN)
        want.append(O.g1_compress(acc))
    s0 = stats(batch)
    got = batch.g1_lincomb_batch(table, idx, [[k] * n for k in ks])
    assert [v for v in range(B) if got[v] != want[v]] == []
    digits = sum(1 for k in ks for b in k.to_bytes(32, "big") if b)
    assert (stats(batch) - s0).tolist() == [1, n * digits, 0]


def test_refusals_before_any_device_work(batch, table, monkeypatch):
    """B = G1M_BMAX + 1 rows, and 32 B n = 2^31 scalar bytes: ValueError, and neither counts as a call.  The second
    goes through the same shim lines and the same C check; only the packing of 2^26 Python integers into 2 GiB of
    scalar bytes is replaced by zeroed bytes of that length, which the call refuses before it reads them."""
    s0 = stats(batch)
    with pytest.raises(ValueError, match="too many"):
        batch.g1_lincomb_batch(table, [0], [[1]] * (Z.G1M_BMAX + 1))
    assert batch.g1_lincomb_batch(table, [0], [[1]] * 2) == [E.known_log_table()[0]] * 2  # the same form, accepted
    assert (stats(batch) - s0).tolist() == [1, 2, 0]
    s1 = stats(batch)
    n = 1024
    B = Z.G1M_BMAX
    assert 32 * B * n == 1 << 31
    monkeypatch.setattr(batch, "_lincomb_rows", lambda rows, n_: bytes(32 * B * n_))
    with pytest.raises(ValueError, match="too many"):
        batch.g1_lincomb_batch(table, [0] * n, None)
    monkeypatch.undo()
    assert (stats(batch) - s1).tolist() == [0, 0, 0]
    c = table.ctx
    out = ctypes.create_string_buffer(48)
    idx0 = np.zeros(1, dtype=np.uint32)
    assert c.lib.bls_g1_table_msm(c.h, idx0.ctypes.data, 1, E.k32(1), Z.G1M_BMAX + 1, out) == batch._native.BLS_E_ARG
    assert (stats(batch) - s1).tolist() == [0, 0, 0]


def test_five_rows_of_65_points_equal_multi_exp(batch, table):
    """B = 5 (two scan blocks), n = 65 distinct Lagrange points, random full-width scalars: the bytes bls_multi_exp
    returns per row for the same point bytes (that route is pinned to the oracle by tests/test_gpu_curve.py) -- the
    one comparison of this module between two device routes"""
    L = E.trusted_setup()[0][:CROSS_N]
    rng = random.Random(0xC505)
    idx = [3 + i for i in rng.sample(range(CROSS_N), CROSS_N)]
    rows = [[rng.randrange(1 << 256) for _ in idx] for _ in range(5)]
    s0 = stats(batch)
    got = batch.g1_lincomb_batch(table, idx, rows)
    assert (stats(batch) - s0)[0] == 1
    c = batch._native.context()
    pts = b"".join(L[i - 3] for i in idx)
    for v, row in enumerate(rows):
        out = ctypes.create_string_buffer(48)
        rc = c.check(c.lib.bls_multi_exp(c.h, 1, pts, b"".join(E.k32(k) for k in row), len(idx), 0, out))
        assert rc == 1 and got[v] == out.raw, v
