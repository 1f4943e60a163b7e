"""CPU self-check of tests/dispatch_edge_inputs.py, the reference the dispatch-edge GPU tests stand on: every layout's
expected_sum is the Python oracle's actual point sum (at 8 and 9 keys over 4 lanes, the same lane arithmetic as 2,048
and 2,049 over 256), the lanes the layouts' comments name are the lanes the members land in, negation by flag flip is
the oracle's negation, the mixed-length messages verify under the C oracle, and the thresholds the GPU tests straddle
are still the ones in csrc/."""
import os
import re

import pytest

import dispatch_edge_inputs as D
from oracle import bls_oracle as O
from oracle import bls_oracle_c as OC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANES = 4


@pytest.fixture(scope="module")
def keys():
    return b"".join(O.SkToPk(D.sk(i)) for i in range(10))


def _point_sum(encs):
    acc = None
    for e in encs:
        acc = O.g1_add(acc, O.g1_decompress(e))
    return acc


def _small_layouts():
    out = []
    for total in (2 * LANES, 2 * LANES + 1):
        out += [(name, total, lay) for name, lay in D.layouts(total, LANES).items()]
        out.append(("plain", total, D.plain(total)))
        out.append(("equal_blocks", total, D.equal_blocks(total, LANES)))
    out.append(("cancel_blocked", 2 * LANES + 2, D.cancel_blocked(2 * LANES + 2)))
    return out


@pytest.mark.parametrize("name,total,lay", _small_layouts(), ids=lambda v: str(v) if not isinstance(v, list) else "")
def test_expected_sum_is_the_oracles_point_sum(keys, name, total, lay):
    assert len(lay) == total
    s = D.expected_sum(lay)
    got = _point_sum(D.key_bytes(keys, lay))
    want = O.g1_mul(O.G1_GEN, s) if s else None
    assert O.g1_compress(got) == O.g1_compress(want)
    if s:
        assert O.g1_compress(got) == O.SkToPk(s)


def _lane_sums(lay, lanes):
    sums = [0] * lanes
    for p, (i, n) in enumerate(lay):
        sums[p % lanes] = (sums[p % lanes] + D.secret(i, n)) % D.R
    return sums


def _twice(lay):
    """the positions of the key that occurs twice (either sign)"""
    seen = {}
    for p, (i, _) in enumerate(lay):
        if i in seen:
            return seen[i], p
        seen[i] = p
    raise AssertionError("no repeated key")


@pytest.mark.parametrize("total", D.DEGENERATE_TOTALS)
def test_layouts_land_in_the_lanes_they_name(total):
    """at full size: the lane (k_g1_sum_q) and the block / lane (64-lane kernels) of every layout's members"""
    L = D.G1Q_SUM_NT
    lays = D.layouts(total)
    a, b = _twice(lays["repeat_same_lane"])
    assert a % L == b % L and a // 64 != b // 64
    a, b = _twice(lays["repeat_neighbours"])
    assert b == a + 1 and a // 64 == b // 64 and a % 4 == 3  # lanes 4t + 3 -> 1, 4t + 4 -> 0: they meet at s = 1
    a, b = _twice(lays["repeat_half"])
    assert b % L == a % L + L // 2 and a % L < L // 2        # the tree's first level adds lane t + 128 into lane t
    a, b = _twice(lays["repeat_eighth"])
    assert a // 64 == b // 64 and b % 64 == a % 64 + 32      # the 64-lane tree's first level
    a, b = _twice(lays["cancel_same_lane"])
    assert a % L == b % L and lays["cancel_same_lane"][b][1] and b + L < total  # and the lane goes on after -P
    a, b = _twice(lays["cancel_neighbours"])
    assert b == a + 1 and lays["cancel_neighbours"][b][1]
    blocked, inter = _lane_sums(lays["cancel_blocked"], L), _lane_sums(lays["cancel_interleaved"], L)
    extra = D.sk(total // 2) if total % 2 else 0
    assert blocked == [extra] + [0] * (L - 1)   # every lane cancels by itself; the odd key is alone in lane 0
    assert all(inter) and D.expected_sum(lays["cancel_interleaved"]) == extra  # no lane cancels: the tree does
    assert D.expected_sum(lays["cancel_blocked"]) == extra
    assert D.expected_sum(D.cancel_blocked(total + 2 - total % 2)) == 0


def test_negation_by_flag_flip_is_the_oracles_negation():
    for k in (1, 2, 77, O.R - 5):
        p, q = O.g1_mul(O.G1_GEN, k), O.g2_mul(O.G2_GEN, k)
        assert D.neg(O.g1_compress(p)) == O.g1_compress(O.g1_neg(p))
        assert D.neg(O.g2_compress(q)) == O.g2_compress(O.g2_neg(q))
        assert O.g1_decompress(D.neg(O.g1_compress(p))) == O.g1_neg(p)
        assert O.g2_decompress(D.neg(O.g2_compress(q))) == O.g2_neg(q)
        assert D.neg(D.neg(O.g1_compress(p))) == O.g1_compress(p)
    assert D.neg(D.G1_INF) == D.G1_INF and D.neg(D.G2_INF) == D.G2_INF
    assert D.secret(4, True) + D.secret(4, False) == D.R


def test_bad_keys_fail_key_validate_in_both_oracles():
    bad = D.bad_keys()
    assert sorted(bad) == ["flag_0x40", "identity", "non_subgroup", "x_is_p"]
    for name, enc in bad.items():
        assert len(enc) == 48 and not O.KeyValidate(enc) and not OC.KeyValidate(enc), name
    assert int.from_bytes(bad["x_is_p"], "big") & ((1 << 381) - 1) == O.P
    assert O.g1_on_curve(D.non_subgroup_g1())


def test_mixed_length_messages_verify_under_the_oracle():
    n = 8
    msgs = D.mixed_messages(n)
    assert [len(m) for m in msgs] == [D.MIXED_LENGTHS[i % 7] for i in range(n)]
    pks = [OC.SkToPk(D.sk(i)) for i in range(n)]
    agg = OC.Aggregate([OC.Sign(D.sk(i), m) for i, m in enumerate(msgs)])
    assert OC.AggregateVerify(pks, msgs, agg) is True
    swapped = msgs[:n - 2] + [msgs[n - 1], msgs[n - 2]]
    assert OC.AggregateVerify(pks, swapped, agg) is False


def test_thresholds_match_the_source():
    """The constants the GPU tests straddle against the text of csrc/: moving a threshold fails here, naming the
    size list to update, instead of leaving the GPU tests on one side of the switch."""
    assert D.G1Q_SUM_MAX == 2048 and D.DEGENERATE_TOTALS == (2048, 2049) and D.KEY_SIZES == (4096, 4097)
    text = {}
    for name, rel, pattern, lists in D.SOURCE_CONSTANTS:
        if rel not in text:
            with open(os.path.join(ROOT, "eth-consensus-specs_amd", rel)) as fh:
                text[rel] = fh.read()
        assert re.search(pattern, text[rel]), (
            "%s: %s no longer contains /%s/ -- update the constant in tests/dispatch_edge_inputs.py and %s"
            % (name, rel, pattern, lists))
    # every switch has a size on each side
    for sizes, edge in ((D.G1_SUM_SIZES, D.G1Q_SUM_MAX), (D.KEY_SIZES, D.WIDE_KEYS_MAX),
                        (D.AV_SIZES_32, D.WIDE_H2C_MAX), (D.AV_SIZES_MIXED, D.WIDE_H2C_MAX),
                        ([n + 1 for n in D.AV_SIZES_32], D.WIDE_MILLER_MAX)):  # n keys + the signature's pair
        assert edge in sizes and edge + 1 in sizes, (sizes, edge)
    assert D.WIDE_MILLER_MAX in D.MULTI_PAIRING_SIZES
    assert {n % D.MLF_PAIRS for n in D.AV_SIZES_32} == {0, 1}
