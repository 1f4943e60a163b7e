"""GPU tests of the bucket MSM over a call's own G1 points (bls_g1_msm; batch.g1_msm / g1_msm_stats): known answers
at full size from the trusted-setup fixture (sum_i omega^(i j) L[i] = M[j]), byte equality with bls_multi_exp on
both sides of every batch size the kernels cut at, one-bucket windows around the run length, the window chain's
edges, identities and the call's refusals.  batch.g1_msm_stats proves that the bucket route ran: bls_g1_msm has no
size switch, so every call here runs the new kernels."""
import ctypes
import random

import numpy as np
import pytest

import g1_table_edge_inputs as E
from dispatch_edge_inputs import non_subgroup_g1
from oracle import bls_oracle as O

pytestmark = pytest.mark.gpu

R = O.R
BIG = (1 << 256) - 1
IDENT = E.G1_INF
BMAX = 256  # rows per call (include/blsmi355x.h)


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
    rng = random.Random(0x71AC)
    step = O.g1_mul(O.G1_GEN, rng.randrange(1, R))
    pts, cur = [], O.g1_mul(O.G1_GEN, rng.randrange(1, R))
    for _ in range(6):
        pts.append(cur)
        cur = O.g1_add(cur, step)
    return pts


def stats(batch):
    return np.array(batch.g1_msm_stats(), dtype=np.int64)


def digits(k):
    return sum(1 for b in E.k32(k) if b)


def enc(p):
    return O.g1_compress(p)


def multi_exp_old(batch, pts48, ks, subgroup=0):
    """the per-point chain route on the same bytes, straight through the C ABI (scalars as given, not reduced)"""
    c = batch._native.context()
    out = ctypes.create_string_buffer(48)
    rc = c.check(c.lib.bls_multi_exp(c.h, 1, b"".join(pts48), b"".join(E.k32(k) for k in ks), len(pts48), subgroup,
                                     out))
    assert rc == 1
    return out.raw


def oracle_row(points, row):
    want = None
    for p, k in zip(points, row):
        if p is not None and k:
            want = O.g1_add(want, O.g1_mul(p, k))
    return enc(want)


# ---- known answers at full size ------------------------------------------------------------------------------------
JS = (0, 1, 65)


def test_known_answers_full_size(batch, setup):
    """Over the 4,096 Lagrange points in file order: sum_i omega^(i j) L[i] = g1_monomial[j] for j = 0, 1, 65, as one
    B = 3 call and as three B = 1 calls that place the same bucket entries; full-width scalars, no oracle
    arithmetic."""
    L, M = setup
    n = len(L)
    w = E.root_of_unity(n)
    rows = [[pow(w, i * j, R) for i in range(n)] for j in JS]
    s0 = stats(batch)
    assert batch.g1_msm(L, rows) == [M[j] for j in JS]
    s1 = stats(batch)
    assert (s1 - s0)[0] == 1 and (s1 - s0)[1] == sum(digits(k) for row in rows for k in row)
    for j, row in zip(JS, rows):
        assert batch.g1_msm(L, [row]) == [M[j]]
    s2 = stats(batch)
    assert (s2 - s1).tolist() == [3, (s1 - s0)[1]]  # the same digits, whatever the batching
    assert (s1 - s0)[1] > n  # row j = 0 alone is n entries


# ---- against the per-point chains ----------------------------------------------------------------------------------
@pytest.mark.parametrize("subgroup", [0, 1])
@pytest.mark.parametrize("B", [1, 3])
def test_bytes_equal_multi_exp(batch, setup, B, subgroup):
    """n = 1, 2, 63, 64, 65, 129 distinct points, random 256-bit scalars (not reduced), decoded with and without the
    subgroup check: the bytes bls_multi_exp returns for the same point and scalar bytes (that route is pinned to the
    oracle by tests/test_gpu_curve.py)."""
    L, _ = setup
    rng = random.Random(0xAC + 2 * B + subgroup)
    for n in (1, 2, 63, 64, 65, 129):
        pts = [L[i] for i in rng.sample(range(256), n)]
        rows = [[rng.randrange(1 << 256) for _ in range(n)] for _ in range(B)]
        s0 = stats(batch)
        got = batch.g1_msm(pts, rows, subgroup_check=bool(subgroup))
        assert (stats(batch) - s0).tolist() == [1, sum(digits(k) for row in rows for k in row)]
        assert got == [multi_exp_old(batch, pts, row, subgroup) for row in rows], n


# ---- one bucket per window, around the run length ------------------------------------------------------------------
def test_one_bucket_per_window_around_the_run_length(batch, pool):
    """All scalars of a row equal, so every window has ONE bucket holding every point: n = K - 1, K, K + 1 and
    K^2 + 1 (one, two and three levels of the fold).  sum_i [k] P_i = [k] sum_i P_i, one oracle multiplication per
    case; the sort placed n entries per non-zero digit of k."""
    K = E.K
    rng = random.Random(0x5CF)
    for n in (K - 1, K, K + 1, K * K + 1):
        k = rng.randrange(1 << 254, R)
        pick = [i % 5 for i in range(n)]
        total = None
        for e in range(5):
            total = O.g1_add(total, O.g1_mul(pool[e], pick.count(e)))
        s0 = stats(batch)
        got = batch.g1_msm([enc(pool[e]) for e in pick], [[k] * n])
        assert got == [enc(O.g1_mul(total, k))], n
        assert (stats(batch) - s0).tolist() == [1, n * digits(k)]


# ---- the window chain ----------------------------------------------------------------------------------------------
def test_window_chain_edges(batch, pool):
    """One non-zero digit in window 0, 1, 15, 16, 30 and 31 (the chain starts there and doubles 8 w times); 2^(8w) - 1
    beside 2^(8w); all digits 255 on a point of G1 and on a point outside G1 decoded unchecked (an integer multiple,
    not reduced mod r); a 128-bit row and a full-width row in one call, whose chains start at different windows; a
    row whose only non-zero scalar is 1."""
    p, q = pool[0], pool[1]
    ep, eq = enc(p), enc(q)
    ws = (0, 1, 15, 16, 30, 31)
    single = [[d << (8 * w)] for w in ws for d in (1, 255)]
    s0 = stats(batch)
    assert batch.g1_msm([ep], single) == [enc(O.g1_mul(p, k)) for (k,) in single]
    assert (stats(batch) - s0).tolist() == [1, len(single)]
    around = [[(1 << (8 * w)) - 1, 1 << (8 * w)] for w in ws[1:]]
    assert batch.g1_msm([ep, eq], around) == [oracle_row([p, q], row) for row in around]
    assert batch.g1_msm([eq, ep], around) == [oracle_row([q, p], row) for row in around]
    out = non_subgroup_g1()
    assert batch.g1_msm([ep], [[BIG]]) == [enc(O.g1_mul(p, BIG))] == [enc(O.g1_mul(p, BIG % R))]
    got = batch.g1_msm([enc(out)], [[BIG], [R], [1]])
    assert got == [enc(O.g1_mul(out, k)) for k in (BIG, R, 1)] and got[1] != IDENT
    assert got[0] == multi_exp_old(batch, [enc(out)], [BIG])
    rng = random.Random(0x128)
    mixed = [[rng.randrange(1 << 127, 1 << 128) for _ in range(3)],
             [rng.randrange(1 << 255, 1 << 256) for _ in range(3)]]
    pts = [p, q, pool[2]]
    assert batch.g1_msm([enc(x) for x in pts], mixed) == [oracle_row(pts, row) for row in mixed]
    assert batch.g1_msm([enc(x) for x in pts], mixed[::-1]) == [oracle_row(pts, row) for row in mixed[::-1]]
    s1 = stats(batch)
    assert batch.g1_msm([enc(x) for x in pts], [[0, 1, 0], [0, 0, 1]]) == [eq, enc(pool[2])]
    assert (stats(batch) - s1).tolist() == [1, 2]


# ---- identities ----------------------------------------------------------------------------------------------------
def test_identities_and_repeated_points(batch, pool):
    """Scalars 0 and r on a point of G1 and a row of zeros give the identity encoding c0 00..; P and -P with equal
    scalars cancel; the identity point among others adds nothing and leaves no bucket entry; the same point bytes
    listed many times: n = 37 drawn from 6 points equals the oracle's sum over the points of (sum of scalars) P."""
    p = pool[0]
    ep = enc(p)
    assert enc(None) == IDENT
    s0 = stats(batch)
    assert batch.g1_msm([ep], [[0], [R]]) == [IDENT, IDENT]
    assert (stats(batch) - s0).tolist() == [1, digits(R)]
    assert batch.g1_msm([ep, enc(pool[1])], [[0, 0]]) == [IDENT]
    assert enc(O.g1_neg(p)) == E.neg48(ep)
    rows = [[k, k] for k in E.EDGE_SCALARS]
    assert batch.g1_msm([ep, E.neg48(ep)], rows) == [IDENT] * len(rows)
    s1 = stats(batch)
    assert batch.g1_msm([IDENT, enc(pool[1]), IDENT], [[BIG, 2, 7], [5, 0, BIG]]) == [enc(O.g1_mul(pool[1], 2)), IDENT]
    assert (stats(batch) - s1).tolist() == [1, 1]
    assert batch.g1_msm([IDENT], [[BIG]]) == [IDENT]
    # n = 37 from six points, the identity and a point outside G1 among them
    pts = [None, p, O.g1_neg(p), non_subgroup_g1(), pool[1], pool[2]]
    rng = random.Random(37)
    pick = [rng.randrange(6) for _ in range(37)]
    assert len(set(pick)) == 6
    row = [rng.choice(E.EDGE_SCALARS) if i % 3 else rng.randrange(1 << 256) for i in range(37)]
    want = None
    for e in range(1, 6):
        want = O.g1_add(want, O.g1_mul(pts[e], sum(k for i, k in zip(pick, row) if i == e)))
    s2 = stats(batch)
    assert batch.g1_msm([enc(pts[e]) for e in pick], [row, [0] * 37]) == [enc(want), IDENT]
    assert (stats(batch) - s2).tolist() == [1, sum(digits(k) for i, k in zip(pick, row) if i)]


# ---- refusals ------------------------------------------------------------------------------------------------------
def test_refusals_and_a_fresh_context(batch, setup):
    from bls_mi355x import _native

    L, M = setup
    ctx = _native.Context(0)  # a context of its own: no table loaded, and the entry needs none
    try:
        lib, h = ctx.lib, ctx.h
        out = ctypes.create_string_buffer(48 * 4)
        assert lib.bls_g1_table_size(h) == 0 and batch.g1_msm_stats(ctx) == (0, 0)
        rng = random.Random(9)
        ks = [rng.randrange(1 << 256) for _ in range(5)]
        assert batch.g1_msm(L[:5], [ks], ctx=ctx) == [multi_exp_old(batch, L[:5], ks)]
        assert batch.g1_msm_stats(ctx) == (1, sum(digits(k) for k in ks))
        bad = b"\x80" + bytes(47)  # x = 0 without the infinity flag
        assert lib.bls_g1_msm(h, L[0] + bad, 2, E.k32(1) * 2, 1, 0, out) == 0
        with pytest.raises(ValueError, match="invalid"):
            batch.g1_msm([L[0], bad], [[1, 2]], ctx=ctx)
        outside = O.g1_compress(non_subgroup_g1())
        assert lib.bls_g1_msm(h, L[0] + outside, 2, E.k32(1) * 2, 1, 1, out) == 0
        with pytest.raises(ValueError, match="invalid"):
            batch.g1_msm([L[0], outside], [[1, 2]], subgroup_check=True, ctx=ctx)
        assert batch.g1_msm([L[0], outside], [[1, 2]], ctx=ctx) == [multi_exp_old(batch, [L[0], outside], [1, 2])]
        # empty input, B = 0, B above the cap, too many scalars (sizes only), null pointers
        assert lib.bls_g1_msm(h, L[0], 0, E.k32(1), 1, 0, out) == 0
        with pytest.raises(ValueError):
            batch.g1_msm([], [[]], ctx=ctx)
        with pytest.raises(ValueError):
            batch.g1_msm([L[0]], [], ctx=ctx)
        assert lib.bls_g1_msm(h, L[0], 1, E.k32(1), 0, 0, out) == _native.BLS_E_ARG
        assert lib.bls_g1_msm(h, L[0], 1, E.k32(1), BMAX + 1, 0, out) == _native.BLS_E_ARG
        assert lib.bls_g1_msm(h, L[0], 1 << 20, E.k32(1), 64, 0, out) == _native.BLS_E_ARG  # 32 B n = 2^31
        assert lib.bls_g1_msm(h, L[0], 1, E.k32(1), 1, 0, None) == _native.BLS_E_ARG
        assert lib.bls_g1_msm(h, None, 1, E.k32(1), 1, 0, out) == _native.BLS_E_ARG
        assert lib.bls_g1_msm(h, L[0], 1, None, 1, 0, out) == _native.BLS_E_ARG
        assert batch.g1_msm_stats(ctx) == (2, sum(digits(k) for k in ks) + 2)  # refused calls count nothing
        # the cap itself is taken: BMAX rows of one scalar each
        rows = [[v + 1] for v in range(BMAX)]
        got = batch.g1_msm([L[0]], rows, ctx=ctx)
        assert got[0] == L[0] and got[1] == multi_exp_old(batch, [L[0]], [2]) and len(set(got)) == BMAX
        assert got[BMAX - 1] == multi_exp_old(batch, [L[0]], [BMAX])
        assert lib.bls_g1_table_size(h) == 0
    finally:
        ctx.close()
