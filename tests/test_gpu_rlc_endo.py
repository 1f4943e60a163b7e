"""The RLC scalars' endomorphism form on the GPU: the batch reads its 64 random bits as r_i = a + b lambda, the G1
side through k_sig_lane2's joint chain on apk_i and phi(apk_i) (csrc/bls_g1_endo.h), the sigma side through the
-G1 comb whose upper four windows hold phi images (k_msm_upairs, k_neg_rg1).  A lambda on one side that is not the
phi of the other fails every valid batch, so valid batches over several seeds are the check; one forged item per
batch sends the bisection through k_neg_rg1 on the same comb.  Requires an MI355X."""
import hashlib

import numpy as np
import pytest

from oracle import bls_oracle as O

pytestmark = pytest.mark.gpu

N_REG = 192
B_MAX = 130
SHAPES = [1, 2, 5, 64, 65, 130]  # 64 and 65 straddle one wave of each half of k_sig_lane2
SEEDS = [hashlib.sha256(b"rlc-endo" + bytes([k])).digest() for k in range(8)]


@pytest.fixture(scope="module")
def batch():
    from bls_mi355x import batch as b
    return b


@pytest.fixture(scope="module")
def items(batch):
    """Registry sk_i = i + 1 (N_REG keys) and B_MAX valid items with committees of 1, 3 and 8 keys in turn; item j
    signs SHA256("endo" || j) with the sum of its secret keys.  A batch of B items is the first B of them."""
    rng = np.random.default_rng(0xE1D0)
    pks = batch.sk_to_pk_batch(b"".join((i + 1).to_bytes(32, "big") for i in range(N_REG)))
    assert batch.Registry().load(pks).all()
    lens = [(1, 3, 8)[j % 3] for j in range(B_MAX)]
    comms = [rng.choice(N_REG, size=n, replace=False) for n in lens]
    msgs = [hashlib.sha256(b"endo" + j.to_bytes(8, "little")).digest() for j in range(B_MAX)]
    agg = [sum(int(x) + 1 for x in c) % O.R for c in comms]
    sigs = batch.sign_batch(b"".join(a.to_bytes(32, "big") for a in agg), b"".join(msgs))
    idx = np.concatenate(comms).astype(np.uint32)
    offs = batch.offsets_from_lengths(lens)
    return idx, offs, msgs, bytes(sigs)


def _take(items, B):
    idx, offs, msgs, sigs = items
    return idx[: int(offs[B])], offs[: B + 1], b"".join(msgs[:B]), bytearray(sigs[: 96 * B])


@pytest.mark.parametrize("B", SHAPES)
def test_valid_batches_pass_under_every_seed(batch, items, B):
    idx, offs, msgs, sigs = _take(items, B)
    rb = batch.ResidentFavBatch(idx, offs, msgs, bytes(sigs))
    try:
        assert rb.run_pipelined(SEEDS) == [True] * len(SEEDS)  # jobs in flight, as the benchmark runs them
        assert rb.verdicts().all()
        for seed in SEEDS:
            assert rb.run_pipelined([seed]) == [True]
            assert rb.verdicts().all()
    finally:
        rb.free()


@pytest.mark.parametrize("B", [b for b in SHAPES if b >= 2])
def test_one_wrong_message_item_is_isolated(batch, items, B):
    """The last item carries its neighbour's signature (a valid G2 point for another message: only the pairing
    check catches it).  Every pass fails, and the bisection -- -r_i G1 from the comb -- rejects that item alone."""
    idx, offs, msgs, sigs = _take(items, B)
    j, k = B - 1, 0
    sigs[96 * j: 96 * j + 96] = sigs[96 * k: 96 * k + 96]
    expect = np.ones(B, dtype=bool)
    expect[j] = False
    rb = batch.ResidentFavBatch(idx, offs, msgs, bytes(sigs))
    try:
        for seed in SEEDS:
            assert rb.run_pipelined([seed]) == [False]
            v = rb.verdicts()
            assert (v == expect).all(), np.nonzero(v != expect)
    finally:
        rb.free()


@pytest.mark.parametrize("B", [1, 2, 5])
def test_small_batches_no_fallback(batch, items, B):
    """The shape of test_gpu_batches.py::test_fav_small_batch_msm_identities: with so few scalars most bit-sums U_b
    are the identity under the new weights too, and a valid batch must pass without any fallback work."""
    idx, offs, msgs, sigs = items
    sel = [j for j in range(B_MAX) if j % 3 == 2][:B]  # committees of 8 keys
    ix = np.concatenate([idx[int(offs[j]): int(offs[j + 1])] for j in sel])
    out = batch.fast_aggregate_verify_batch(ix, batch.offsets_from_lengths([8] * B), b"".join(msgs[j] for j in sel),
                                            b"".join(sigs[96 * j: 96 * j + 96] for j in sel))
    assert out.all()
    assert batch.fallback_stats() == (0, 0)
