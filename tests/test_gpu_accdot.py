"""GPU tests of the f accumulation with one reduction per output coefficient (csrc/bls_acc_dot.h on fq_mul_dot6:
k_miller_acc4q<G> and k_miller_fused<G> run it): every Miller-loop form of bls_test_miller_forms against form 0, the
wave-program form among them as the implementation that shares none of this code, at the pair counts where the
G = 4 kernel's grouping changes (a last group partly filled, one wave of 64 pairs and one pair past it), with an
identity pair inside a group and at the end; and one FastAggregateVerify batch just past the size from which the
pipeline lets four pairs share an f (BLS_ACC_SHARED_MIN = 4,096).  Requires an MI355X."""
import hashlib

import numpy as np
import pytest

from oracle import bls_oracle as O
from test_gpu_miller_forms import FORMS, _forms, _gt_bytes, _pairs  # the forms' list and encodings: one place

pytestmark = pytest.mark.gpu

COUNTS = [1, 4, 5, 63, 64, 65, 257]


@pytest.fixture(scope="module")
def pairs():
    """257 pairs, computed once; every case takes a prefix"""
    return _pairs(max(COUNTS), 0xACCD)


def _cases():
    for n in COUNTS:
        yield n, None
        if n > 1:
            yield n, 1      # position 1 of the first group of every G
        yield n, n - 1      # the last pair


@pytest.mark.parametrize("n,ident", list(_cases()))
def test_forms_agree(pairs, n, ident):
    ps, qs = list(pairs[0][:n]), list(pairs[1][:n])
    if ident is not None:
        ps[ident] = None
    got = _forms(ps, qs)
    for k in range(1, len(FORMS)):
        assert got[k] == got[0], FORMS[k]
    if n <= 3:  # the oracle's pairing product (slow in Python: small n only)
        f = O.F12_ONE
        for p, q in zip(ps, qs):
            if p is not None:
                f = O.f12_mul(f, O.miller_loop(p, q))
        assert got[0] == _gt_bytes(O.final_exponentiation(f))


# ---- the shared-f path end to end ----
B, NKEYS, REG = 4100, 2, 64
SWAPPED = 4097


@pytest.fixture(scope="module")
def fav():
    """4,100 items of 2 keys over a 64-key registry (sk_i = i + 1), each signed with the sum of its secret keys"""
    from bls_mi355x import batch

    reg = batch.Registry()
    reg.generate(REG, first_sk=1)
    rng = np.random.default_rng(0xACCD)
    committees = [rng.choice(REG, size=NKEYS, replace=False) for _ in range(B)]
    sks = [int(sum(int(k) + 1 for k in c)) % O.R for c in committees]
    msgs = b"".join(hashlib.sha256(b"accdot" + j.to_bytes(4, "little")).digest() for j in range(B))
    sigs = batch.sign_batch(b"".join(sk.to_bytes(32, "big") for sk in sks), msgs)
    idx = np.concatenate(committees).astype(np.uint32)
    return batch, idx, batch.offsets_from_lengths([NKEYS] * B), msgs, sigs


def test_shared_f_batch_all_valid(fav):
    batch, idx, offs, msgs, sigs = fav
    out = batch.fast_aggregate_verify_batch(idx, offs, msgs, sigs)
    assert len(out) == B and out.all(), np.nonzero(~out)


def test_shared_f_batch_one_swapped_signature(fav):
    """item 4,097 carries item 4,096's signature: only the pairing check can tell, and the verdicts name that item"""
    batch, idx, offs, msgs, sigs = fav
    bad = bytearray(sigs)
    bad[96 * SWAPPED: 96 * SWAPPED + 96] = sigs[96 * (SWAPPED - 1): 96 * SWAPPED]
    assert bad[96 * SWAPPED: 96 * SWAPPED + 96] != sigs[96 * SWAPPED: 96 * SWAPPED + 96]
    out = batch.fast_aggregate_verify_batch(idx, offs, msgs, bytes(bad))
    assert np.nonzero(~out)[0].tolist() == [SWAPPED]
