"""GPU tests of the per-call sums and key checks on both sides of every kernel switch (inputs and lane maps:
tests/dispatch_edge_inputs.py).

G1 sums (launch_g1_sum_aff, csrc/bls_kernels.hip): k_g1_sum_q, one workgroup of 256 lanes, up to 2,048 points, and
k_g1_sum_aff<64> + k_jac_sum above, through AggregatePKs, per-call FastAggregateVerify (its verdict is True exactly
when the Jacobian sum and the pz the Miller loop scales by are right) and the two multi-exponentiations --
batch.g1_multi_exp (bls_multi_exp: k_pt_scale, k_pt_sum, k_pt_sum_jac) and bls_g1_multi_exp (k_g1_scale, then the
same launch_g1_sum_aff with the live mask).  Plain sums at every size around the switch and the lane counts, then
the degenerate layouts at 2,048 and 2,049 keys: which branch each reaches --
  repeat_same_lane     2,048: g1q_add_aff doubling in one lane; 2,049: equal points in two blocks, generic adds
  repeat_neighbours / repeat_half / repeat_eighth   the pair meets inside larger sums at tree level s = 1 / 128 / 32
  cancel_same_lane     2,048: the lane's accumulator returns to the identity (0 : 1 : 0) and goes on
  cancel_neighbours    P, -P in lanes 3 and 4
  cancel_blocked       2,048: every lane ends at the identity, g1q_add of identities at all 8 levels, the Z == 0 exit;
                       2,049 (two-pass): partial b + 16 = -partial b, so k_jac_sum's jac_add meets P + (-P) in 15
                       lanes at s = 16 and adds identities after; the lone key of block 32 is the whole sum;
                       2,050: k_jac_sum's lanes 1 .. 15 all reach [64] G1, so jac_add doubles at s = 8, 4, 2, adds
                       [512] G1 and its negation at s = 1 and returns the identity (dispatch_edge_inputs.cancel_blocked)
  cancel_interleaved   g1q_add(P, -P) at tree level s = 1 in every pair of lanes, identities above; the 64-lane tree's
                       jac_add the same
  equal_blocks         (2,048 and 4,096) equal sums in lanes 32 apart and in every block: g1q_add's and jac_add's
                       doubling at whole tree levels of k_g1_sum_q, k_g1_sum_aff<64>, k_jac_sum, k_pt_sum, k_pt_sum_jac
and k_g2_sum_aff / k_pt_sum / k_pt_sum_jac (Aggregate, multi_exp in G2) at 63, 64, 65, 129 points and, for the
grid-stride path, 65,537, where every lane and tree node adds equal points (jac_add's doubling branch).

Key checks (launch_keys, launch_pairs_decode, csrc/bls_capi_ctx.hip): two keys per wave up to 4,096, one per lane
above, with one invalid key in the first and the last slot.

Expected values: every sum is SkToPk / Sign of the sum of the secrets (C oracle); where a sum is the identity the
oracle is asked what it does with the same bytes.  Requires an MI355X."""
import ctypes

import pytest

import dispatch_edge_inputs as D
from oracle import bls_oracle as O
from oracle import bls_oracle_c as OC

pytestmark = pytest.mark.gpu

NKEYS = D.WIDE_KEYS_MAX + 4
MSG = bytes(range(7, 39))


@pytest.fixture(scope="module")
def M():
    from bls_mi355x.backend import mi355x_bls
    return mi355x_bls


@pytest.fixture(scope="module")
def batch():
    from bls_mi355x import batch as b
    return b


@pytest.fixture(scope="module")
def ctx():
    from bls_mi355x import _native
    return _native.context()


@pytest.fixture(scope="module")
def keys(batch):
    """pk_i = [i + 1] G1, i < 4,100, from one device call; three of them against the oracle"""
    pks = batch.sk_to_pk_batch(b"".join(D.sk(i).to_bytes(32, "big") for i in range(NKEYS)))
    for i in (0, D.G1Q_SUM_MAX, NKEYS - 1):
        assert pks[48 * i: 48 * i + 48] == OC.SkToPk(D.sk(i))
    return pks


def _oracle_or_raise(fn, *args):
    try:
        return fn(*args)
    except ValueError:
        return ValueError


def _kzg_multi_exp(ctx, pts, ks):
    """bls_g1_multi_exp: checked decode (identity accepted), k_g1_scale, launch_g1_sum_aff with the live mask"""
    out = ctypes.create_string_buffer(48)
    rc = ctx.check(ctx.lib.bls_g1_multi_exp(ctx.h, b"".join(pts), b"".join(k.to_bytes(32, "big") for k in ks),
                                            len(pts), out))
    assert rc == 1
    return out.raw


def _check_sum(M, batch, ctx, pks, s):
    """the three entry points (and the second multi-exponentiation) on one key list whose secrets sum to s"""
    n = len(pks)
    if s:
        want = OC.SkToPk(s)
        assert M._AggregatePKs(pks) == want
        sig = OC.Sign(s, MSG)
        assert M.FastAggregateVerify(pks, MSG, sig) is True
        assert M.FastAggregateVerify(pks[:-1], MSG, sig) is False
    else:  # the identity: whatever the oracle does with the same bytes
        want = D.G1_INF
        assert _oracle_or_raise(M._AggregatePKs, pks) == _oracle_or_raise(OC.AggregatePKs, pks)
        for sig in (OC.Sign(1, MSG), D.G2_INF):
            assert M.FastAggregateVerify(pks, MSG, sig) == OC.FastAggregateVerify(pks, MSG, sig)
    assert batch.g1_multi_exp(pks, [1] * n) == want
    assert _kzg_multi_exp(ctx, pks, [1] * n) == want


@pytest.mark.parametrize("n", D.G1_SUM_SIZES)
def test_plain_sums(M, batch, ctx, keys, n):
    """distinct keys: 1, 2 (254 idle lanes), 255 / 256 / 257 (a lane short, one each, one lane with two), 513, the
    last size of k_g1_sum_q and its neighbours, 2,049 (33 blocks of k_g1_sum_aff<64>, the last with one point;
    k_jac_sum folds 33 partials on 64 lanes) and 2,113 (34 blocks)"""
    lay = D.plain(n)
    assert D.expected_sum(lay) == n * (n + 1) // 2
    _check_sum(M, batch, ctx, D.key_bytes(keys, lay), D.expected_sum(lay))


def _degenerate_cases():
    cases = [(total, name) for total in D.DEGENERATE_TOTALS for name in D.layouts(total)]
    return cases + [(D.G1Q_SUM_MAX + 2, "cancel_blocked")]


@pytest.mark.parametrize("total,name", _degenerate_cases())
def test_degenerate_sums(M, batch, ctx, keys, total, name):
    lay = D.cancel_blocked(total) if total == D.G1Q_SUM_MAX + 2 else D.layouts(total)[name]
    assert len(lay) == total
    s = D.expected_sum(lay)
    assert (s == 0) == (name in ("cancel_blocked", "cancel_interleaved") and total % 2 == 0)
    _check_sum(M, batch, ctx, D.key_bytes(keys, lay), s)


@pytest.mark.parametrize("n", [D.G1Q_SUM_MAX, 2 * D.G1Q_SUM_MAX])
def test_sums_of_equal_blocks(M, batch, ctx, keys, n):
    """position p holds key p % 32, so equal sums meet wherever lanes 32 apart or whole blocks are added.  2,048
    (k_g1_sum_q): every lane adds one key 8 times (g1q_add_aff doubling, then P + 2P, ..) and lanes t, t + 128 / 64 /
    32 hold equal sums (g1q_add doubling at three tree levels).  4,096 (k_g1_sum_aff<64> + k_jac_sum; k_pt_sum +
    k_pt_sum_jac for batch.g1_multi_exp): the first tree level of every block doubles, the 64 partials are equal,
    and every level of the second kernel's tree is jac_add's doubling branch."""
    lay = D.equal_blocks(n)
    assert D.expected_sum(lay) == n // 32 * (32 * 33 // 2)
    _check_sum(M, batch, ctx, D.key_bytes(keys, lay), D.expected_sum(lay))


def _masked(keys, n):
    """(points, scalars, expected secret) of the multi_exp mask case at n points: unit scalars on distinct keys but
    for scalar 0 at positions 0 and 256, scalar r at 255 and n - 1 (live == 0 after scaling), the identity at
    positions 5, 300 and n - 2 (three lanes), key 10 again at 266 with scalar r - 1 (lane 10 of k_g1_sum_q: the
    cancellation exists only after scaling), and one 255-bit scalar at position 3"""
    pts = D.key_bytes(keys, D.plain(n))
    ks = [1] * n
    ks[0] = ks[256] = 0
    ks[255] = ks[n - 1] = D.R
    for p in (5, 300, n - 2):
        pts[p] = D.G1_INF
    ks[300] = 12345
    pts[266], ks[266] = pts[10], D.R - 1
    ks[3] = (1 << 254) + 0x1234567
    assert ks[3] < D.R and ks[3].bit_length() == 255
    live = [(D.sk(10) if p == 266 else D.sk(p), k) for p, k in enumerate(ks) if pts[p] != D.G1_INF]
    return pts, ks, sum(a * k for a, k in live) % D.R


@pytest.mark.parametrize("n", D.DEGENERATE_TOTALS)
def test_multi_exp_mask(batch, ctx, keys, n):
    pts, ks, s = _masked(keys, n)
    want = OC.SkToPk(s)
    assert batch.g1_multi_exp(pts, ks) == want       # reduces the scalars mod r on the host
    assert _kzg_multi_exp(ctx, pts, ks) == want      # takes r as it is: [r] P must come out as the identity
    if n == D.DEGENERATE_TOTALS[0]:  # the construction itself, on the first 8 entries, against the group law
        acc = None
        for p, k in zip(pts[:8], ks[:8]):
            acc = O.g1_add(acc, O.g1_mul(O.g1_decompress(p), k))
        assert batch.g1_multi_exp(pts[:8], ks[:8]) == O.g1_compress(acc) == _kzg_multi_exp(ctx, pts[:8], ks[:8])
        live8 = sum(D.sk(p) * k for p, k in enumerate(ks[:8]) if p != 5) % D.R
        assert O.g1_compress(acc) == OC.SkToPk(live8)


def _msm_pattern(n):
    """(base secret index per position or None for the identity, scalar per position) of the curve multi_exp cases:
    scalars k and r - k on one point at positions j, j + 64 (the same lane of neighbouring blocks, where n allows)
    and in neighbouring lanes 10 and 11, the identity at 20, a zero scalar at 21"""
    base = list(range(n))
    ks = [(0x9E3779B97F4A7C15 * (i + 1)) % (1 << 64) | 1 for i in range(n)]
    base[11], ks[11] = base[10], D.R - ks[10]
    base[20] = None
    ks[21] = 0
    for j in range(0, n - 64, 64):
        base[j + 64], ks[j + 64] = base[j], D.R - ks[j]
    s = sum(D.sk(b) * k for b, k in zip(base, ks) if b is not None) % D.R
    assert s
    return base, ks, s


@pytest.fixture(scope="module")
def g2_table():
    """Q_i = [i + 1] H(MSG) for i < 129, as the oracle's signatures"""
    sks = b"".join(D.sk(i).to_bytes(32, "big") for i in range(129))
    raw = OC.sign_batch(sks, MSG * 129, 8)
    assert raw[96 * 128:] == OC.Sign(129, MSG)
    return [raw[96 * i: 96 * i + 96] for i in range(129)]


@pytest.mark.parametrize("n", [63, 64, 65, 129])
def test_g2_multi_exp(ctx, g2_table, n):
    """bls_multi_exp in G2 (pt_msm: k_pt_scale, k_pt_sum on ceil(n / 64) blocks, k_pt_sum_jac): a block short of a
    lane, full, one point in a second block, one in a third"""
    base, ks, s = _msm_pattern(n)
    pts = [D.G2_INF if b is None else g2_table[b] for b in base]
    for flag in (0, 1):
        out = ctypes.create_string_buffer(96)
        rc = ctx.check(ctx.lib.bls_multi_exp(ctx.h, 2, b"".join(pts), b"".join(k.to_bytes(32, "big") for k in ks), n,
                                             flag, out))
        assert rc == 1 and out.raw == OC.Sign(s, MSG), flag


def test_g2_multi_exp_equal_blocks(ctx, g2_table):
    """128 points, position p the point and scalar p % 32: lanes t and t + 32 of k_pt_sum hold equal products and the
    two blocks' partials are equal, so its first tree level and k_pt_sum_jac's last take jac_add's doubling branch"""
    n = 128
    ks = [(0xD1B54A32D192ED03 * (i + 1)) % (1 << 64) | 1 for i in range(32)]
    s = 4 * sum(D.sk(i) * k for i, k in enumerate(ks)) % D.R
    out = ctypes.create_string_buffer(96)
    rc = ctx.check(ctx.lib.bls_multi_exp(ctx.h, 2, b"".join(g2_table[p % 32] for p in range(n)),
                                         b"".join(ks[p % 32].to_bytes(32, "big") for p in range(n)), n, 0, out))
    assert rc == 1 and out.raw == OC.Sign(s, MSG)


def test_g1_multi_exp_65(batch, ctx, keys):
    base, ks, s = _msm_pattern(65)
    pts = [D.G1_INF if b is None else keys[48 * b: 48 * b + 48] for b in base]
    assert batch.g1_multi_exp(pts, ks) == OC.SkToPk(s) == _kzg_multi_exp(ctx, pts, ks)


@pytest.mark.parametrize("n", [63, 64, 65])
def test_aggregate_degenerate(M, g2_table, n):
    """Aggregate (k_g2_sum_aff + k_jac_sum): signature 7 again at position 40 (lanes 7 and 40 meet at s = 1 inside
    larger sums), the negation of signature 9 at position 10, a signature and its negation 32 lanes apart (48, 16:
    jac_add(P, -P) at the tree's first level) and signature 0 again at the lone position 64 of a second block"""
    sigs = list(g2_table[:n])
    sigs[40] = sigs[7]
    sigs[10] = D.neg(sigs[9])
    sigs[48] = D.neg(sigs[16])
    if n > 64:
        sigs[64] = sigs[0]
    assert M.Aggregate(sigs) == OC.Aggregate(sigs)


def test_aggregate_grid_stride(M, g2_table):
    """65,537 signatures, position p the signature p % 64: 1,024 blocks of the same 64 signatures, thread (0, 0)
    takes position 65,536 as well (its accumulator doubles), every lane of k_jac_sum adds 16 equal partials and every
    node of its tree two equal sums (jac_add's doubling branch).  Expected from the construction: every secret
    1,024 times and secret 1 once more; only the device decodes the 65,537 points."""
    n = D.SUM_BLOCK * D.SUM_MAX_BLOCKS + 1
    s = (1024 * sum(D.sk(j) for j in range(64)) + D.sk(0)) % D.R
    assert s == sum(D.sk(p % 64) for p in range(n)) % D.R
    assert M.Aggregate([g2_table[p % 64] for p in range(n)]) == OC.Sign(s, MSG)


# ---- key validation across WIDE_KEYS_MAX ----
@pytest.mark.parametrize("n", D.KEY_SIZES)
def test_key_validate_switch(M, keys, n):
    """n valid keys (two per wave at 4,096, one per lane at 4,097), then each invalid key in the first slot, in slot
    4,095 (the second half of the wide kernel's last wave) and, at 4,097, in slot 4,096 (the lone lane of the lane
    kernel's last block): AggregatePKs raises and FastAggregateVerify is False exactly as the oracle's KeyValidate of
    the one changed key says (the other keys are valid by construction)"""
    pks = D.key_bytes(keys, D.plain(n))
    s = n * (n + 1) // 2
    sig = OC.Sign(s, MSG)
    assert M._AggregatePKs(pks) == OC.SkToPk(s)
    assert M.FastAggregateVerify(pks, MSG, sig) is True
    assert M.FastAggregateVerify(pks[:-1], MSG, sig) is False
    for name, enc in D.bad_keys().items():
        valid = OC.KeyValidate(enc)
        assert valid == O.KeyValidate(enc)
        for pos in sorted({0, D.WIDE_KEYS_MAX - 1, n - 1}):
            bad = list(pks)
            bad[pos] = enc
            if valid:
                M._AggregatePKs(bad)
            else:
                with pytest.raises(ValueError):
                    M._AggregatePKs(bad)
                assert M.FastAggregateVerify(bad, MSG, sig) is False, (name, pos)


@pytest.fixture(scope="module")
def outside_pair(keys, g2_table):
    """(the G1 encodings -P_7 and the non-subgroup point, Q, the oracle's verdict on e(-P_7, Q) e(ns, Q) == 1): the
    only two pairs of the pairing-check lists that need the oracle"""
    ns = D.non_subgroup_g1()
    q = g2_table[6]
    minus = D.neg(keys[48 * 7: 48 * 8])
    Q = O.g2_decompress(q)
    verdict = O.pairing_product_is_one([(O.g1_decompress(minus), Q), (ns, Q)])
    return minus, O.g1_compress(ns), q, verdict


@pytest.mark.parametrize("n", D.KEY_SIZES)
def test_pairing_check_decode_switch(ctx, keys, outside_pair, n):
    """bls_pairing_check_ex over n pairs: (P_i, Q), (-P_i, Q) with one Q, and (identity, Q) for the odd one -- the
    product is 1.  With the subgroup checks the wide decoders run up to 4,096 pairs and the lane decoders above;
    the non-subgroup point in the last slot is rejected by either (0), and without the checks the verdict is the
    oracle's on the last two pairs (all others cancel)."""
    minus, ns, q, verdict = outside_pair
    g1 = []
    for i in range(n // 2 - 1):
        k = keys[48 * i: 48 * i + 48]
        g1 += [k, D.neg(k)]
    if n % 2:
        g1.insert(1, D.G1_INF)
    tail = keys[48 * 7: 48 * 8]
    good = b"".join(g1 + [minus, tail])
    outside = b"".join(g1 + [minus, ns])
    g2 = q * n
    assert len(good) == 48 * n
    for flag in (1, 0):
        assert ctx.check(ctx.lib.bls_pairing_check_ex(ctx.h, good, g2, n, flag)) == 1
    assert ctx.check(ctx.lib.bls_pairing_check_ex(ctx.h, outside, g2, n, 1)) == 0
    assert ctx.check(ctx.lib.bls_pairing_check_ex(ctx.h, outside, g2, n, 0)) == int(verdict)
