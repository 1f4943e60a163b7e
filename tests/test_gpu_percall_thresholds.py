"""GPU tests of the per-call pairings on both sides of their kernel switches (thresholds and inputs:
tests/dispatch_edge_inputs.py):

  wide_h2c_max = 1,024 messages (bls_aggregate_verify): k_h2c_wide with H Jacobian (hz) / the lane hash kernels with
      H affine (launch_h2c for 32-byte messages, launch_h2c_msgs otherwise);
  wide_miller_max = 1,100 pairs (launch_miller_call): k_miller_wide on ceil(n / 2) workgroups / the wave-program
      kernel; between them, 1,025 <= n <= 1,099 keys, the lane hash feeds the wide Miller kernel with qz == nullptr;
  npair >= 256 (bls_aggregate_verify_batch): launch_miller_wave below, launch_miller_fused from there.

Keys pk_i = [i + 1] G1; the signatures come from the C oracle (the device does not check its own), the aggregates
of their prefixes from the device's Aggregate, compared once per set with the oracle's.  The knob table is read
once per process, so no test sets a BLS_* knob; with BLS_WIDE_H2C_MAX or BLS_WIDE_MILLER_MAX in the environment the
sizes here no longer straddle the switches and the tests skip.  Requires an MI355X."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

import dispatch_edge_inputs as D
from oracle import bls_oracle as O
from oracle import bls_oracle_c as OC

pytestmark = pytest.mark.gpu

N = D.WIDE_MILLER_MAX + 1
THREADS = 8

_KNOBS = [k for k in ("BLS_WIDE_H2C_MAX", "BLS_WIDE_MILLER_MAX") if k in os.environ]
needs_default_thresholds = pytest.mark.skipif(
    bool(_KNOBS), reason="%s set in the environment: the sizes of these tests assume the thresholds 1,024 and 1,100"
    % ", ".join(_KNOBS))


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
def pks(batch):
    raw = batch.sk_to_pk_batch(b"".join(D.sk(i).to_bytes(32, "big") for i in range(N)))
    for i in (0, D.WIDE_H2C_MAX, N - 1):
        assert raw[48 * i: 48 * i + 48] == OC.SkToPk(D.sk(i))
    return [raw[48 * i: 48 * i + 48] for i in range(N)]


class _Set:
    """1,101 (key, message, signature) triples; aggregate(n) is the device's Aggregate of the first n signatures"""

    def __init__(self, M, pks, msgs, sigs):
        self.M, self.pks, self.msgs, self.sigs = M, pks, msgs, sigs
        self._agg = {}

    def aggregate(self, n):
        if n not in self._agg:
            self._agg[n] = self.M.Aggregate(self.sigs[:n])
        return self._agg[n]


def _checked(s):
    n = D.WIDE_H2C_MAX + 1
    assert s.aggregate(n) == OC.Aggregate(s.sigs[:n])
    return s


@pytest.fixture(scope="module")
def set32(M, pks):
    msgs = [hashlib.sha256(b"percall-thresholds" + i.to_bytes(4, "little")).digest() for i in range(N)]
    raw = OC.sign_batch(b"".join(D.sk(i).to_bytes(32, "big") for i in range(N)), b"".join(msgs), THREADS)
    assert raw[96 * (N - 1):] == OC.Sign(D.sk(N - 1), msgs[N - 1])
    return _checked(_Set(M, pks, msgs, [raw[96 * i: 96 * i + 96] for i in range(N)]))


@pytest.fixture(scope="module")
def set_mixed(M, pks):
    msgs = D.mixed_messages(N)
    return _checked(_Set(M, pks, msgs, [OC.Sign(D.sk(i), m) for i, m in enumerate(msgs)]))


def _aggregate_verify_cases(M, s, n):
    pks, msgs, agg = s.pks[:n], s.msgs[:n], s.aggregate(n)
    assert msgs[n - 2] != msgs[n - 1] and msgs[0] != msgs[1]
    assert M.AggregateVerify(pks, msgs, agg) is True
    # the last message pair and the signature's pair share the tail workgroup of k_miller_wide or split, by parity
    assert M.AggregateVerify(pks, msgs[:n - 2] + [msgs[n - 1], msgs[n - 2]], agg) is False
    assert M.AggregateVerify(pks, [msgs[1], msgs[0]] + msgs[2:], agg) is False
    assert M.AggregateVerify(pks[:n - 1], msgs[:n - 1], agg) is False
    assert M.AggregateVerify(pks, msgs, s.aggregate(n - 1)) is False


@needs_default_thresholds
@pytest.mark.parametrize("n", D.AV_SIZES_32)
def test_aggregate_verify_32_byte_messages(M, set32, n):
    """1,023 / 1,024: k_h2c_wide, hz, k_miller_wide; 1,025 / 1,099: launch_h2c, H affine, k_miller_wide with
    qz == nullptr (1,026 and 1,100 pairs); 1,100 / 1,101: launch_h2c and the wave-program kernel"""
    _aggregate_verify_cases(M, set32, n)


@needs_default_thresholds
@pytest.mark.parametrize("n", D.AV_SIZES_MIXED)
def test_aggregate_verify_mixed_lengths(M, set_mixed, n):
    """messages of 0, 1, 31, 32, 33, 100 and 200 bytes: k_h2c_wide's byte-streaming path at 1,024, launch_h2c_msgs
    into the wide Miller kernel at 1,025 and into the wave-program kernel at 1,100"""
    _aggregate_verify_cases(M, set_mixed, n)


@needs_default_thresholds
def test_aggregate_verify_1025_against_the_oracle(M, set32):
    """the one full-size oracle call (the slowest item of the file: 1,026 pairings on the CPU): the lane hash into
    the wide Miller kernel, on identical bytes"""
    n = D.WIDE_H2C_MAX + 1
    pks, msgs, agg = set32.pks[:n], set32.msgs[:n], set32.aggregate(n)
    assert OC.AggregateVerify(pks, msgs, agg) is True
    assert M.AggregateVerify(pks, msgs, agg) is True


# ---- bls_multi_pairing across wide_miller_max ----
MP_MSG = b"\x3c" * 32
MP_SUM = 0x1D2C3B4A59687F6E5D4C3B2A19080706F5E4D3C2B1A0 % D.R  # sum a_i b_i of every list below
MP_CYCLE = 16


def _gt_bytes(f):
    return b"".join(c[0].to_bytes(48, "big") + c[1].to_bytes(48, "big") for c in O.f12_to_coeffs(f))


@pytest.fixture(scope="module")
def mp(pks):
    """lists(n) -> (G1 encodings, G2 encodings) of n pairs ([a_i] G1, [b_i] H(m)) with a_i = i + 1, b_i = i % 16 + 1
    but for the last, chosen so that sum a_i b_i = MP_SUM for every n; and the Python oracle's e([MP_SUM] G1, H(m))"""
    cycle = [OC.Sign(b + 1, MP_MSG) for b in range(MP_CYCLE)]

    def lists(n):
        head = sum(D.sk(i) * (i % MP_CYCLE + 1) for i in range(n - 1)) % D.R
        last = (MP_SUM - head) * pow(D.sk(n - 1), -1, D.R) % D.R
        assert last and (head + D.sk(n - 1) * last) % D.R == MP_SUM
        return pks[:n], [cycle[i % MP_CYCLE] for i in range(n - 1)] + [OC.Sign(last, MP_MSG)]

    want = _gt_bytes(O.pairing(O.g1_mul(O.G1_GEN, MP_SUM), O.g2_decompress(OC.hash_to_g2(MP_MSG))))
    return lists, want


def _multi_pairing(ctx, g1, g2, flag):
    out = ctypes.create_string_buffer(576)
    rc = ctx.check(ctx.lib.bls_multi_pairing(ctx.h, b"".join(g1), b"".join(g2), len(g1), flag, out))
    return rc, out.raw


@needs_default_thresholds
@pytest.mark.parametrize("n", D.MULTI_PAIRING_SIZES)
def test_multi_pairing_matches_one_oracle_pairing(ctx, mp, n):
    """k_miller_wide at 1, 2, 3 pairs (a half-filled workgroup, one, one and a half), 1,099 (an odd tail) and 1,100
    (the last size): the 576 bytes are the oracle's e([sum a_i b_i] G1, H(m))"""
    lists, want = mp
    g1, g2 = lists(n)
    for flag in (0, 1):
        assert _multi_pairing(ctx, g1, g2, flag) == (1, want), flag


@needs_default_thresholds
def test_multi_pairing_1101_wave_kernel_matches_wide_kernel(ctx, mp):
    """1,100 pairs and an identity pair: the wave-program kernel on 1,101 pairs must return the wide kernel's bytes for
    the 1,100 -- the two Miller kernels compared value for value after the final exponentiation"""
    lists, want = mp
    g1, g2 = lists(D.WIDE_MILLER_MAX)
    for flag in (0, 1):
        wide = _multi_pairing(ctx, g1, g2, flag)
        assert wide == (1, want)
        assert _multi_pairing(ctx, g1 + [D.G1_INF], g2 + [g2[0]], flag) == wide
        assert _multi_pairing(ctx, g1 + [g1[0]], g2 + [D.G2_INF], flag) == wide


@needs_default_thresholds
@pytest.mark.parametrize("n", [D.WIDE_MILLER_MAX, D.WIDE_MILLER_MAX + 1])
def test_pairing_check_cancelling_list(batch, ctx, pks, mp, n):
    """batch.pairing_check on (P_i, Q), (-P_i, Q) for 550 keys -- and (identity, Q) at 1,101 --: True; with the sign
    flag of the last live pair flipped the product is e(P, Q)^2: False"""
    q = mp[0](1)[1][0]
    g1 = [e for k in pks[:D.WIDE_MILLER_MAX // 2] for e in (k, D.neg(k))]
    if n % 2:
        g1.append(D.G1_INF)
    assert len(g1) == n
    assert batch.pairing_check([(p, q) for p in g1], ctx=ctx) is True
    last_live = D.WIDE_MILLER_MAX - 1
    g1[last_live] = D.neg(g1[last_live])
    assert batch.pairing_check([(p, q) for p in g1], ctx=ctx) is False


# ---- bls_aggregate_verify_batch across npair = 256 ----
@pytest.mark.parametrize("B,per_item", [(15, 16), (16, 15)])
@pytest.mark.parametrize("which", ["set32", "set_mixed"])
def test_aggregate_verify_batch_across_256_pairs(batch, request, which, B, per_item):
    """npair = keys + items: 15 x 16 + 15 = 255 (launch_miller_wave), 16 x 15 + 16 = 256 (launch_miller_fused).  All
    valid: no fallback; then the last item's last two messages swapped: only that item fails, in one round."""
    s = request.getfixturevalue(which)
    assert B * per_item + B == D.AVB_FUSED_MIN_NPAIR - (1 if B == 15 else 0)
    items = [range(b * per_item, (b + 1) * per_item) for b in range(B)]
    pk = [[s.pks[i] for i in it] for it in items]
    msgs = [[s.msgs[i] for i in it] for it in items]
    sigs = [OC.Aggregate([s.sigs[i] for i in it]) for it in items]
    out = batch.aggregate_verify_batch(pk, msgs, sigs)
    assert out.all() and batch.fallback_stats() == (0, 0)
    bad = [list(m) for m in msgs]
    bad[B - 1][-2:] = bad[B - 1][-1], bad[B - 1][-2]
    assert bad[B - 1] != msgs[B - 1]
    out = batch.aggregate_verify_batch(pk, bad, sigs)
    assert np.nonzero(~out)[0].tolist() == [B - 1] and batch.fallback_stats()[1] == 1
    for b in (0, B - 2, B - 1):
        assert OC.AggregateVerify(pk[b], bad[b], sigs[b]) is bool(out[b])
