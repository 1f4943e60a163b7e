"""GPU checks of the homogeneous projective line steps (csrc/bls_miller_lines.h) behind k_miller_lines2 and
k_miller_fused: every Miller-loop form of bls_test_miller_forms -- the split and fused kernels that run the new
steps, and the wave-program kernel, an independent implementation -- must give the same GT element after the final
exponentiation, and for the smallest pair counts the oracle's pairing product.  Pair counts: one lane pair of a
wave, one and a half, a partial and a full 32-pair span plus one, and one past a 64-pair fused workgroup; each with
and without an identity pair (its lane pair leaves the line kernel early, its record rows are never read).

A batch whose one signature is a point of E2 outside G2 must reject that item and accept the rest: the Miller
loop's steps have no exceptional-case branch, so the verdict rests on the subgroup check and the per-item re-check.
The same through k_sig_validate (grouped aggregation, one group per signature), whose [|x|] sigma chain adds the
affine base with the mixed addition.
"""
import ctypes
import hashlib
import random

import numpy as np
import pytest

from oracle import bls_oracle as O
from test_gpu_miller_forms import FORMS, _gt_bytes  # the forms' list and the GT encoding: one place

pytestmark = pytest.mark.gpu

NFORMS = len(FORMS)


def _pairs(n, seed, identity):
    r = random.Random(seed)
    g2 = O.hash_to_g2(b"line steps %d" % seed)
    ps = [None if i == identity else O.g1_mul(O.G1_GEN, r.randrange(1, 1 << 40)) for i in range(n)]
    qs = [O.g2_mul(g2, r.randrange(1, 1 << 40)) for _ in range(n)]
    return ps, qs


@pytest.mark.parametrize("identity", [False, True])
@pytest.mark.parametrize("n", [1, 2, 3, 33, 65])
def test_line_forms_agree(n, identity):
    from bls_mi355x import _native

    ps, qs = _pairs(n, 4000 + n, n - 1 if identity else -1)
    ctx = _native.context()
    g1 = b"".join(O.g1_compress(p) for p in ps)
    g2 = b"".join(O.g2_compress(q) for q in qs)
    out = ctypes.create_string_buffer(NFORMS * 576)
    assert ctx.check(ctx.lib.bls_test_miller_forms(ctx.h, g1, g2, n, out)) == 1
    got = [out.raw[576 * k: 576 * k + 576] for k in range(NFORMS)]
    assert [k for k in range(NFORMS) if got[k] != got[0]] == []
    if n <= 3:
        f = O.F12_ONE
        for p, q in zip(ps, qs):
            if p is not None:
                f = O.f12_mul(f, O.miller_loop(p, q))
        assert got[0] == _gt_bytes(O.final_exponentiation(f))


def test_fav_batch_of_70_with_one_signature_outside_g2():
    """70 items (past one 64-lane workgroup of the lane kernels), item 37's signature on E2 but outside G2"""
    from bls_mi355x import batch as b

    n_reg, B, size = 64, 70, 3
    rng = np.random.default_rng(0x70)
    pks = b.sk_to_pk_batch(b"".join((i + 1).to_bytes(32, "big") for i in range(n_reg)))
    b.Registry().load(pks)
    idx, msgs, agg = [], [], []
    for j in range(B):
        c = rng.choice(n_reg, size=size, replace=False)
        idx.extend(int(x) for x in c)
        msgs.append(hashlib.sha256(b"mlines" + j.to_bytes(4, "little")).digest())
        agg.append(sum(int(x) + 1 for x in c) % O.R)
    sigs = bytearray(b.sign_batch(b"".join(k.to_bytes(32, "big") for k in agg), b"".join(msgs)))
    q = O.iso_map(O.map_to_curve_sswu((17, 19)))
    assert O.g2_on_curve(q) and not O.g2_in_subgroup(q)
    sigs[96 * 37: 96 * 38] = O.g2_compress(q)
    out = b.fast_aggregate_verify_batch(np.array(idx, dtype=np.uint32), b.offsets_from_lengths([size] * B),
                                        b"".join(msgs), bytes(sigs))
    assert [j for j in range(B) if not out[j]] == [37]


def test_sig_validate_batch_of_70_with_one_signature_outside_g2():
    """70 signatures through k_sig_validate (bls_aggregate_grouped with one group per signature, so each group's
    verdict is its signature's): item 37 on E2 but outside G2 is rejected, the other 69 are accepted and come back
    unchanged"""
    from bls_mi355x import batch as b

    B = 70
    msgs = [hashlib.sha256(b"validate" + j.to_bytes(4, "little")).digest() for j in range(B)]
    sigs = bytearray(b.sign_batch(b"".join((1000 + j).to_bytes(32, "big") for j in range(B)), b"".join(msgs)))
    q = O.iso_map(O.map_to_curve_sswu((23, 29)))
    assert O.g2_on_curve(q) and not O.g2_in_subgroup(q)
    sigs[96 * 37: 96 * 38] = O.g2_compress(q)
    got = b.aggregate_grouped(bytes(sigs), np.arange(B, dtype=np.uint32), n_groups=B)
    assert [j for j in range(B) if got[j] is None] == [37]
    assert all(got[j] == bytes(sigs[96 * j: 96 * j + 96]) for j in range(B) if j != 37)
