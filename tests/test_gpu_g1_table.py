"""GPU tests of the resident G1 point table and its batched bucket MSM (bls_g1_table_*; batch.G1Table,
batch.g1_lincomb_indexed / g1_lincomb_batch, curve.use_g1_table): known answers at full size from the trusted-setup
fixture (sum_i omega^(i j) L[i] = M[j]), edge scalars and points against the Python oracle, skewed buckets around
the run length, byte equality with bls_multi_exp, the drop-in route with its counters, and the table's lifecycle
and refusals.  batch.g1_table_stats proves which route ran."""
import ctypes
import random

import numpy as np
import pytest

import g1_table_edge_inputs as E
from dispatch_edge_inputs import non_subgroup_g1
from oracle import bls_oracle as O

pytestmark = pytest.mark.gpu

R = O.R


@pytest.fixture(scope="module")
def batch():
    from bls_mi355x import batch as b

    return b


@pytest.fixture(scope="module")
def setup():
    return E.trusted_setup()


@pytest.fixture(scope="module")
def pool():
    """a few points of G1 (affine) by running sums: two oracle multiplications, then additions"""
    rng = random.Random(0x71AB)
    step = O.g1_mul(O.G1_GEN, rng.randrange(1, R))
    pts, cur = [], O.g1_mul(O.G1_GEN, rng.randrange(1, R))
    for _ in range(6):
        pts.append(cur)
        cur = O.g1_add(cur, step)
    return pts


def stats(batch):
    return np.array(batch.g1_table_stats(), dtype=np.int64)


def multi_exp_old(batch, pts48, ks, subgroup=0):
    """the parent's route on the same bytes, straight through the C ABI (scalars as given, not reduced)"""
    c = batch._native.context()
    out = ctypes.create_string_buffer(48)
    rc = c.check(c.lib.bls_multi_exp(c.h, 1, b"".join(pts48), b"".join(E.k32(k) for k in ks), len(pts48), subgroup,
                                     out))
    assert rc == 1
    return out.raw


# ---- known answers at full size ------------------------------------------------------------------------------------
JS = (0, 1, 65)


def test_known_answers_full_size(batch, setup):
    """T = the 4,096 Lagrange points in file order: sum_i omega^(i j) T[i] = g1_monomial[j] for j = 0, 1, 65, as one
    B = 3 call and as three B = 1 calls; full-width scalars, no oracle arithmetic."""
    L, M = setup
    n = len(L)
    w = E.root_of_unity(n)
    t = batch.G1Table()
    assert t.load(L).all() and len(t) == n
    idx = np.arange(n, dtype=np.uint32)
    rows = [[pow(w, i * j, R) for i in range(n)] for j in JS]
    s0 = stats(batch)
    assert batch.g1_lincomb_batch(t, idx, rows) == [M[j] for j in JS]
    s1 = stats(batch)
    assert (s1 - s0)[0] == 1 and n < (s1 - s0)[1] <= 3 * 32 * n
    for j, row in zip(JS, rows):
        assert batch.g1_lincomb_indexed(t, idx, row) == M[j]
    s2 = stats(batch)
    assert (s2 - s1).tolist() == [3, (s1 - s0)[1], 0]  # the same digits, whatever the batching
    before = stats(batch)
    assert batch.g1_lincomb_indexed(t, idx, [1] * n) == M[0]
    assert (stats(batch) - before).tolist() == [1, n, 0]  # scalar 1: one bucket entry per point


def test_bit_reversed_table_is_the_commitment_call_shape(batch, setup):
    """The table loaded in bit-reversed order, as blob_to_kzg_commitment passes the setup: naming natural order
    through idx = the bit-reversal permutation, and naming the table in its own order with the scalars permuted as
    the points are, both give g1_monomial[j]."""
    L, M = setup
    n = len(L)
    bits = n.bit_length() - 1
    brp = [E.bit_reverse(i, bits) for i in range(n)]
    w = E.root_of_unity(n)
    t = batch.G1Table()
    assert t.load([L[brp[i]] for i in range(n)]).all()
    natural = [[pow(w, i * j, R) for i in range(n)] for j in JS]
    assert batch.g1_lincomb_batch(t, np.array(brp, dtype=np.uint32), natural) == [M[j] for j in JS]
    permuted = [[row[brp[i]] for i in range(n)] for row in natural]
    assert batch.g1_lincomb_batch(t, np.arange(n, dtype=np.uint32), permuted) == [M[j] for j in JS]
    assert t.indices([L[5]]).tolist() == [brp[5]]


# ---- edges against the oracle --------------------------------------------------------------------------------------
def test_edge_scalars_and_points_against_oracle(batch, pool):
    """n = 1, 2, 37 over a table holding the identity, P, -P, a point outside G1 (loaded unchecked) and two more:
    every edge scalar on P and on the non-subgroup point (integer multiples: 2^256 - 1 is not reduced), P and -P
    with equal scalars (the identity, c0 00..), a row of zeros, the same index many times."""
    p, q = pool[0], non_subgroup_g1()
    pts = [None, p, O.g1_neg(p), q, pool[1], pool[2]]
    enc = [O.g1_compress(x) for x in pts]
    assert enc[2] == E.neg48(enc[1])
    t = batch.G1Table()
    assert t.load(enc, subgroup_check=False).tolist() == [1] * 6
    ident = O.g1_compress(None)
    assert ident == E.G1_INF
    # n = 1: each edge scalar alone, on P and on the point outside G1
    for e in (1, 3):
        got = batch.g1_lincomb_batch(t, [e], [[k] for k in E.EDGE_SCALARS])
        assert got == [O.g1_compress(O.g1_mul(pts[e], k)) for k in E.EDGE_SCALARS], e
    assert batch.g1_lincomb_batch(t, [1], [[0], [R]]) == [ident, ident]
    assert batch.g1_lincomb_indexed(t, [0], [(1 << 256) - 1]) == ident  # the identity entry
    # n = 2: P and -P cancel for every scalar; the identity entry beside a point adds nothing
    assert batch.g1_lincomb_batch(t, [1, 2], [[k, k] for k in E.EDGE_SCALARS]) == [ident] * len(E.EDGE_SCALARS)
    assert batch.g1_lincomb_batch(t, [0, 4], [[(1 << 256) - 1, 2], [5, 0]]) == [O.g1_compress(O.g1_mul(pool[1], 2)),
                                                                                ident]
    # n = 37: repeated indices, edge and random scalars, and a row of zeros
    rng = random.Random(37)
    idx = [rng.randrange(6) for _ in range(37)]
    assert len(set(idx)) == 6
    row = [rng.choice(E.EDGE_SCALARS) if i % 3 else rng.randrange(1 << 256) for i in range(37)]
    want = None
    for e in range(6):  # sum_i k_i T[idx_i] = sum_e (sum of the k_i naming e) T[e], one multiplication per entry
        want = O.g1_add(want, O.g1_mul(pts[e], sum(k for i, k in zip(idx, row) if i == e)))
    s0 = stats(batch)
    assert batch.g1_lincomb_batch(t, idx, [row, [0] * 37]) == [O.g1_compress(want), ident]
    assert (stats(batch) - s0)[0] == 1


def test_skewed_buckets_around_the_run_length(batch, pool):
    """All scalars of a call equal, so every window has ONE bucket holding all its entries: n = K - 1, K, K + 1 and
    K^2 + 1 (runs of every length up to K, a second and a third level).  sum_i [k] P_i = [k] sum_i P_i, one
    oracle multiplication per case; m repeats of one index are [m k] P."""
    K = E.K
    enc = [O.g1_compress(x) for x in pool[:5]]
    t = batch.G1Table()
    assert t.load(enc).all()
    rng = random.Random(0x5CE)
    for n in (K - 1, K, K + 1, K * K + 1):
        k = rng.randrange(1 << 254, R)
        idx = [i % 5 for i in range(n)]
        total = None
        for e in range(5):
            total = O.g1_add(total, O.g1_mul(pool[e], idx.count(e)))
        s0 = stats(batch)
        got = batch.g1_lincomb_batch(t, idx, [[k] * n, [1] * n])
        assert got == [O.g1_compress(O.g1_mul(total, k)), O.g1_compress(total)], n
        digits = sum(1 for w in range(32) if (k >> (8 * w)) & 0xFF)
        assert (stats(batch) - s0).tolist() == [1, n * digits + n, 0]
        assert batch.g1_lincomb_indexed(t, [3] * n, [k] * n) == O.g1_compress(O.g1_mul(pool[3], n * k % R)), n


# ---- against the existing route ------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
def test_bytes_equal_multi_exp(batch, setup, B):
    """n = 63, 64, 65, 129 distinct points, random full-width scalars: the bytes bls_multi_exp returns for the same
    point bytes (that route is pinned to the oracle by tests/test_gpu_curve.py)."""
    L, _ = setup
    t = batch.G1Table()
    assert t.load(L[:129]).all()
    rng = random.Random(0xAB + B)
    for n in (63, 64, 65, 129):
        idx = rng.sample(range(129), n)
        rows = [[rng.randrange(1 << 256) for _ in range(n)] for _ in range(B)]
        s0 = stats(batch)
        got = batch.g1_lincomb_batch(t, idx, rows)
        assert (stats(batch) - s0)[0] == 1
        assert got == [multi_exp_old(batch, [L[i] for i in idx], row) for row in rows], n


# ---- drop-in -------------------------------------------------------------------------------------------------------
def g1_lincomb(bls, points, scalars):
    """the body of the spec's g1_lincomb (specs/deneb/polynomial-commitments.md:266-286), bytes out"""
    assert len(points) == len(scalars)
    if len(points) == 0:
        return bls.G1_to_bytes48(bls.Z1())
    points_g1 = []
    for point in points:
        points_g1.append(bls.bytes48_to_G1(point))
    result = bls.multi_exp(points_g1, scalars)
    return bytes(bls.G1_to_bytes48(result))


def test_drop_in_route_and_counters(batch, setup):
    from bls_mi355x import bls, curve

    bls.use_mi355x()
    bls.bls_active = True
    L, M = setup
    n = 48
    rng = random.Random(0xD0)
    ks = [rng.randrange(R) for _ in range(n)]
    pts = L[:n]
    # no table set: the reference results
    objs = [bls.bytes48_to_G1(p) for p in pts]
    want = bls.G1_to_bytes48(bls.multi_exp(objs, ks))
    assert want == multi_exp_old(batch, pts, ks) and g1_lincomb(bls, pts, ks) == want
    outside = pts[:-1] + [M[3]]
    want_out = g1_lincomb(bls, outside, ks)
    g2 = [bls.G2(), bls.multiply(bls.G2(), 5)]
    want_g2 = bls.G2_to_bytes96(bls.multi_exp(g2, [3, 4]))
    t = batch.G1Table()
    assert t.load(L[:64]).all()
    curve.use_g1_table(t)
    try:
        s0 = stats(batch)
        assert bls.G1_to_bytes48(bls.multi_exp(objs, ks)) == want
        assert (stats(batch) - s0)[[0, 2]].tolist() == [1, 0]
        s1 = stats(batch)
        assert g1_lincomb(bls, pts, ks) == want
        assert (stats(batch) - s1)[[0, 2]].tolist() == [1, n]  # one table MSM, every decode a hit
        # one point outside the table: its decode goes to the device and the whole list takes the old route
        s2 = stats(batch)
        assert g1_lincomb(bls, outside, ks) == want_out
        assert (stats(batch) - s2).tolist() == [0, 0, n - 1]
        # the checked multiexp of an unchecked table keeps the old route
        s3 = stats(batch)
        assert bytes(curve.G1Point.multiexp(objs, [curve.Scalar(k) for k in ks])) == want
        assert (stats(batch) - s3).tolist() == [0, 0, 0]
        with pytest.raises(Exception):
            bls.multi_exp([], [])
        with pytest.raises(ValueError):
            curve.G1Point.multiexp_unchecked([], [])
        assert bls.G2_to_bytes96(bls.multi_exp(g2, [3, 4])) == want_g2
        assert (stats(batch) - s3).tolist() == [0, 0, 0]
    finally:
        curve.use_g1_table(None)
    s4 = stats(batch)
    assert g1_lincomb(bls, pts, ks) == want
    assert (stats(batch) - s4).tolist() == [0, 0, 0]


# ---- lifecycle and errors ------------------------------------------------------------------------------------------
def test_lifecycle_and_refusals(batch, setup):
    from bls_mi355x import _native

    L, M = setup
    ctx = _native.Context(0)  # a context of its own: no table yet
    try:
        lib, h = ctx.lib, ctx.h
        out = ctypes.create_string_buffer(48)
        idx0 = np.zeros(1, dtype=np.uint32)
        assert lib.bls_g1_table_size(h) == 0
        assert lib.bls_g1_table_msm(h, idx0.ctypes.data, 1, E.k32(1), 1, out) == _native.BLS_E_NOREG
        assert b"no G1 table" in lib.bls_last_error(h)
        assert lib.bls_g1_table_append(h, L[0], 1, 0, None) == _native.BLS_E_NOREG
        t = batch.G1Table(ctx)
        gen0 = int(lib.bls_g1_table_generation(h))
        bad = b"\x80" + bytes(47)  # x = 0 without the infinity flag
        assert t.load(L[:3] + [bad, E.G1_INF]).tolist() == [1, 1, 1, 0, 1]
        assert int(lib.bls_g1_table_generation(h)) == gen0 + 1
        assert t.append(M[:40]).all() and len(t) == 45  # beyond the first allocation: every window's slab moves
        assert int(lib.bls_g1_table_generation(h)) == gen0 + 1
        assert t.indices([M[39], L[1], E.G1_INF]).tolist() == [44, 1, 4]
        rng = random.Random(5)
        idx = [44, 1, 4, 0, 20, 1]
        ks = [rng.randrange(1 << 256) for _ in idx]
        named = [M[39], L[1], E.G1_INF, L[0], M[15], L[1]]
        assert batch.g1_lincomb_indexed(t, idx, ks) == multi_exp_old(batch, named, ks)
        # an invalid entry named; indices out of range; empty calls
        with pytest.raises(ValueError, match="invalid"):
            batch.g1_lincomb_indexed(t, [0, 3], [1, 2])
        with pytest.raises(ValueError, match="outside"):
            batch.g1_lincomb_indexed(t, [0, 45], [1, 2])
        with pytest.raises(ValueError):
            batch.g1_lincomb_indexed(t, [], [])
        big = np.array([0, 45], dtype=np.uint32)
        assert lib.bls_g1_table_msm(h, big.ctypes.data, 2, E.k32(1) * 2, 1, out) == _native.BLS_E_ARG
        assert lib.bls_g1_table_msm(h, big.ctypes.data, 0, E.k32(1), 1, out) == _native.BLS_E_ARG
        assert lib.bls_g1_table_msm(h, idx0.ctypes.data, 1, E.k32(1), 0, out) == _native.BLS_E_ARG
        assert lib.bls_g1_table_msm(h, idx0.ctypes.data, 1 << 20, E.k32(1), 64, out) == _native.BLS_E_ARG  # 2^31
        # a reload: the old object's indices are refused, the new table answers
        t2 = batch.G1Table(ctx)
        assert t2.load(M[:2], subgroup_check=True).all() and t2.checked and len(t2) == 2
        assert t.indices([L[1]]) is None and int(lib.bls_g1_table_generation(h)) == gen0 + 2
        assert lib.bls_g1_table_msm(h, np.array([4], dtype=np.uint32).ctypes.data, 1, E.k32(1), 1, out) == \
            _native.BLS_E_ARG
        assert batch.g1_lincomb_indexed(t2, [1, 0], [7, 9]) == multi_exp_old(batch, [M[1], M[0]], [7, 9])
        calls, entries, _ = batch.g1_table_stats(ctx)
        assert calls == 2 and entries > 0
    finally:
        ctx.close()
