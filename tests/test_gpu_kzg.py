"""GPU tests of the device blob KZG functions (bls_kzg_*; bls_mi355x.kzg): evaluations against Horner and the
restatement of kzg_inputs.py, commitments and proofs against known answers from the monomial setup and against the
table MSM on the restatement's quotient, verification with every way of being wrong, batches with per-item verdicts,
the setup's lifecycle, verification batches at the sizes where the call changes shape (seam_sizes.py) and the Python
calls' chunking.  The blob size is the spec's 4,096 elements; no call has more than 6 blobs."""
import ctypes
import hashlib
import random

import numpy as np
import pytest

import kzg_inputs as K
import seam_sizes as Z
from dispatch_edge_inputs import non_subgroup_g1
from oracle import bls_oracle as O

pytestmark = pytest.mark.gpu

R = K.R
ID = K.IDENTITY48
ZERO_BLOB = bytes(32 * K.N)


def fe(v):
    return v.to_bytes(32, "big")


@pytest.fixture(scope="module")
def mods():
    from bls_mi355x import _native, batch, kzg

    return types_ns(native=_native, batch=batch, kzg=kzg)


def types_ns(**kw):
    import types

    return types.SimpleNamespace(**kw)


@pytest.fixture(scope="module")
def S(mods):
    """the trusted setup on the default context: a table of its own (whatever another module left there goes)"""
    L, _, G2 = K.trusted_setup()
    return mods.kzg.KzgSetup(L, G2[1])


@pytest.fixture(scope="module")
def ka():
    return K.known_answers()


@pytest.fixture(scope="module")
def rnd():
    f = K.random_blob(0x6B7A)
    return f, K.blob_bytes(f)


# ---- raw C ABI helpers ---------------------------------------------------------------------------------------------
def eval_blobs(ctx, blobs, zs):
    n = len(blobs)
    y, ok = ctypes.create_string_buffer(32 * n), np.full(n, 7, dtype=np.uint8)
    rc = ctx.lib.bls_kzg_eval_blobs(ctx.h, b"".join(blobs), n, b"".join(zs), y, ok.ctypes.data_as(ctypes.c_void_p))
    return rc, [int.from_bytes(y.raw[32 * i: 32 * i + 32], "big") for i in range(n)], ok.tolist()


def verify_batch(ctx, items, want_items=True):
    n = len(items)
    out = np.full(n, 7, dtype=np.uint8)
    rc = ctx.lib.bls_kzg_verify_batch(ctx.h, b"".join(i[0] for i in items), b"".join(fe(i[1]) for i in items),
                                      b"".join(fe(i[2]) for i in items), b"".join(i[3] for i in items), n,
                                      out.ctypes.data_as(ctypes.c_void_p) if want_items else None)
    return rc, out.tolist()


def commitments_rc(ctx, blobs):
    out = ctypes.create_string_buffer(48 * len(blobs))
    return ctx.lib.bls_kzg_blob_commitments(ctx.h, b"".join(blobs), len(blobs), out, None), out.raw


# ---- evaluation ----------------------------------------------------------------------------------------------------
def test_evaluation_four_blobs_per_call(S, ka, rnd):
    """a random, a constant, the zero and a degree-65 blob in one call, a different z per blob: random z, every
    in-domain index of the list, 0 and r - 1 (= omega^2048, domain index 1), each blob meeting each kind"""
    f, blob = rnd
    rng = random.Random(0xE7A1)
    D = [K.DOMAIN[k] for k in K.IN_DOMAIN_K]
    calls = [
        [rng.randrange(R), D[0], 0, R - 1],
        [D[1], D[2], D[3], rng.randrange(R)],
        [D[4], D[5], R - 1, 0],
        [0, rng.randrange(R), D[5], D[1]],
        [R - 1, 0, rng.randrange(R), D[4]],
    ]
    blobs = [blob, ka[0].blob, ZERO_BLOB, ka[2].blob]
    for zs in calls:
        rc, ys, ok = eval_blobs(S.ctx, blobs, [fe(z) for z in zs])
        assert rc == 1 and ok == [1, 1, 1, 1]
        assert ys[0] == K.evaluate(f, zs[0]), hex(zs[0])
        assert ys[1] == ka[0].coeffs[0]
        assert ys[2] == 0
        assert ys[3] == K.horner(ka[2].coeffs, zs[3]), hex(zs[3])
    assert K.evaluate(ka[2].f, calls[0][3]) == K.horner(ka[2].coeffs, calls[0][3])  # the restatement itself
    assert S.evaluate_polynomial_in_evaluation_form(f, calls[0][0]) == K.evaluate(f, calls[0][0])
    assert S.evaluate_polynomial_in_evaluation_form(ka[2].blob, D[3]) == ka[2].f[255]


def test_evaluation_marks_only_the_blob_with_a_noncanonical_element(S, ka, rnd):
    f, blob = rnd
    zs = [fe(5), fe(K.DOMAIN[16]), fe(0), fe(R - 1)]
    clean = [ka[1].blob, blob, ZERO_BLOB, ka[0].blob]
    rc, want, ok = eval_blobs(S.ctx, clean, zs)
    assert rc == 1 and ok == [1, 1, 1, 1]
    for v in (R, (1 << 256) - 1):
        for pos in (0, 2048, K.N - 1):
            bad = bytearray(blob)
            bad[32 * pos: 32 * pos + 32] = fe(v)
            rc, ys, ok = eval_blobs(S.ctx, [clean[0], bytes(bad), clean[2], clean[3]], zs)
            assert rc == 0 and ok == [1, 0, 1, 1], (hex(v), pos)
            assert ys == [want[0], 0, want[2], want[3]]
            with pytest.raises(AssertionError):
                S.evaluate_blobs([bytes(bad)], [5])
    for z in (R, (1 << 256) - 1):  # z is range-checked as well
        rc, _, _ = eval_blobs(S.ctx, clean, [fe(5), fe(z), fe(0), fe(1)])
        assert rc == 0


# ---- commitments and proofs ----------------------------------------------------------------------------------------
def test_known_commitments_and_proofs(S, ka, mods):
    blobs = [a.blob for a in ka] + [ZERO_BLOB]
    s0 = mods.batch.g1_table_stats(S.ctx)
    assert S.blob_to_kzg_commitments(blobs) == [a.commitment for a in ka] + [ID]
    s1 = mods.batch.g1_table_stats(S.ctx)
    # one MSM of four rows: three rows of 255-bit scalars (~32 non-zero bytes each) and a row of zeros
    assert s1[0] - s0[0] == 1 and 3 * 28 * K.N < s1[1] - s0[1] <= 3 * 32 * K.N
    zs = [0x1234567, K.DOMAIN[255], 99, K.DOMAIN[0]]  # outside, inside, (degree 65:) outside, zero blob: inside
    got = S.compute_kzg_proofs(blobs, zs)
    s2 = mods.batch.g1_table_stats(S.ctx)
    assert s2[0] - s1[0] == 1
    assert S.blob_to_kzg_commitment(ka[1].blob) == ka[1].commitment
    for a, z, (proof, y) in zip(ka, zs, got):
        want_y, want_proof = a.open(z)
        assert (int.from_bytes(y, "big"), proof) == (want_y, want_proof)
    assert got[0][0] == ID  # a constant's quotient is zero
    assert got[3] == (ID, bytes(32))
    proof, y = S.compute_kzg_proof(ka[1].blob, fe(K.DOMAIN[16]))
    assert (int.from_bytes(y, "big"), proof) == ka[1].open(K.DOMAIN[16])


def test_random_blob_proof_is_the_msm_of_the_restated_quotient(S, rnd, mods):
    f, blob = rnd
    idx = S.first + np.arange(K.N, dtype=np.uint32)
    for z in (0xABCDEF0123456789, K.DOMAIN[16], K.DOMAIN[4095], 0):
        y = K.evaluate(f, z)
        want = mods.batch.g1_lincomb_indexed(S.table, idx, K.quotient(f, z, y))
        assert S.compute_kzg_proof(blob, fe(z)) == (want, fe(y)), hex(z)
    assert S.blob_to_kzg_commitment(blob) == mods.batch.g1_lincomb_indexed(S.table, idx, f)


def test_blob_proof_round_trip(S, ka, rnd):
    f, blob = rnd
    c = S.blob_to_kzg_commitment(blob)
    proof = S.compute_blob_kzg_proof(blob, c)
    z = S.compute_challenge(blob, c)
    data = b"FSBLOBVERIFY_V1_" + (4096).to_bytes(16, "big") + blob + c
    assert z == int.from_bytes(hashlib.sha256(data).digest(), "big") % R
    assert proof == S.compute_kzg_proof(blob, fe(z))[0]
    assert S.verify_blob_kzg_proof(blob, c, proof) is True
    assert S.verify_blob_kzg_proof(blob, c, ka[1].commitment) is False
    assert S.verify_blob_kzg_proof(ka[1].blob, c, proof) is False
    other = S.compute_blob_kzg_proof(ka[1].blob, ka[1].commitment)
    assert S.verify_blob_kzg_proof_batch([blob, ka[1].blob], [c, ka[1].commitment], [proof, other]) is True
    assert S.verify_blob_kzg_proof_items([blob, ka[1].blob], [c, ka[1].commitment], [other, other]) == [False, True]
    assert S.verify_blob_kzg_proof_batch([], [], []) is True
    bad = bytearray(blob)
    bad[32 * 100: 32 * 101] = fe(R)
    with pytest.raises(AssertionError):
        S.verify_blob_kzg_proof(bytes(bad), c, proof)
    out = np.full(2, 7, dtype=np.uint8)
    rc = S.ctx.lib.bls_kzg_verify_blob_batch(S.ctx.h, blob + bytes(bad), c + c, proof + proof, fe(z) + fe(z), 2,
                                             out.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0 and out.tolist() == [1, 0]


# ---- verification --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def items(ka):
    """six valid (C, z, y, proof): degree 3 outside and inside the domain, a constant (identity proof), degree 65,
    the zero polynomial (identity commitment and proof), degree 3 again at z = 0"""
    out = []
    for a, z in ((ka[1], 0x5EED), (ka[1], K.DOMAIN[15]), (ka[0], 77), (ka[2], 99)):
        y, proof = a.open(z)
        out.append((a.commitment, z, y, proof))
    out.append((ID, 123456789, 0, ID))
    y, proof = ka[1].open(0)
    out.append((ka[1].commitment, 0, y, proof))
    return out


def test_verify_single(S, ka, items):
    c, z, y, proof = items[0]
    assert S.verify_kzg_proof(c, fe(z), fe(y), proof) is True
    assert S.verify_kzg_proof(c, fe(z), fe((y + 1) % R), proof) is False
    assert S.verify_kzg_proof(c, fe((z + 1) % R), fe(y), proof) is False
    assert S.verify_kzg_proof(c, fe(z), fe(y), items[3][3]) is False  # another blob's proof
    assert S.verify_kzg_proof(proof, fe(z), fe(y), c) is False  # swapped
    assert S.verify_kzg_proof(ID, fe(z), fe(0), ID) is True
    assert S.verify_kzg_proof(ID, fe(z), fe(1), ID) is False
    for it in items:
        assert S.verify_kzg_proof(it[0], fe(it[1]), fe(it[2]), it[3]) is True
    # the same case under the oracle's own pairing, on the two pairs e(C - [y] G1, -G2) e(proof, [tau - z] G2)
    tau = O.g2_decompress(K.trusted_setup()[2][1])
    x = O.g1_add(O.g1_decompress(c), O.g1_neg(O.g1_mul(O.G1_GEN, y)))
    q = O.g2_add(tau, O.g2_neg(O.g2_mul(O.G2_GEN, z)))
    assert O.pairing_product_is_one([(x, O.g2_neg(O.G2_GEN)), (O.g1_decompress(proof), q)])


def test_verify_invalid_inputs(S, items):
    c, z, y, proof = items[0]
    outside = O.g1_compress(non_subgroup_g1())
    forty = bytes([0x40]) + bytes(47)
    for bad in (outside, forty):
        for it in ((bad, z, y, proof), (c, z, y, bad)):
            assert verify_batch(S.ctx, [it]) == (0, [0])
            assert verify_batch(S.ctx, [items[1], it, items[2]]) == (0, [1, 0, 1])
            with pytest.raises(AssertionError):
                S.verify_kzg_proof(it[0], fe(it[1]), fe(it[2]), it[3])
    out = np.full(1, 7, dtype=np.uint8)
    for zb, yb in ((fe(z), fe(R)), (fe(R), fe(y)), (fe(z), b"\xff" * 32)):
        rc = S.ctx.lib.bls_kzg_verify_batch(S.ctx.h, c, zb, yb, proof, 1, out.ctypes.data_as(ctypes.c_void_p))
        assert (rc, out.tolist()) == (0, [0])
        with pytest.raises(AssertionError):
            S.verify_kzg_proof(c, zb, yb, proof)


def test_verify_batches(S, items, mods):
    ctx = S.ctx
    assert S.verify_kzg_proof_batch([], [], [], []) is True
    assert ctx.lib.bls_kzg_verify_batch(ctx.h, None, None, None, None, 0, None) == 1
    for n in (1, 2, 6):
        assert verify_batch(ctx, items[:n]) == (1, [1] * n)
        assert verify_batch(ctx, items[:n], want_items=False)[0] == 1
    cols = list(zip(*items))
    assert S.verify_kzg_proof_batch(cols[0], [fe(z) for z in cols[1]], [fe(y) for y in cols[2]], cols[3]) is True

    def spoil(it):
        return (it[0], it[1], (it[2] + 1) % R, it[3])

    for k in range(6):  # one bad item at each position: the batch fails and the per-item checks name exactly it
        bad = items[:k] + [spoil(items[k])] + items[k + 1:]
        assert verify_batch(ctx, bad) == (0, [int(i != k) for i in range(6)]), k
        assert verify_batch(ctx, bad, want_items=False)[0] == 0
    bad = [items[0], spoil(items[1]), items[2], items[3], (items[4][0], 5, 0, items[0][3]), items[5]]
    assert verify_batch(ctx, bad) == (0, [1, 0, 1, 1, 0, 1])
    assert S.verify_kzg_proof_items(*[list(c) for c in zip(*bad)]) == [True, False, True, True, False, True]
    assert verify_batch(ctx, [items[0]] * 6) == (1, [1] * 6)
    # the same bad item twice: with equal or opposite r_i its error would cancel or double out
    assert verify_batch(ctx, [spoil(items[0])] * 2) == (0, [0, 0])
    assert verify_batch(ctx, [spoil(items[0]), items[1], spoil(items[0])]) == (0, [0, 1, 0])


def test_batch_fails_closed_without_entropy(S, items, mods, tmp_path):
    ctx = S.ctx
    empty = tmp_path / "empty"
    empty.write_bytes(b"")
    try:
        assert ctx.lib.bls_set_entropy_source(str(empty).encode()) == 0
        rc, out = verify_batch(ctx, items[:2])
        assert rc == mods.native.BLS_E_DEVICE
        with pytest.raises(mods.native.NativeError):
            S.verify_kzg_proof(items[0][0], fe(items[0][1]), fe(items[0][2]), items[0][3])
    finally:
        assert ctx.lib.bls_set_entropy_source(b"/dev/urandom") == 0
    assert verify_batch(ctx, items[:2]) == (1, [1, 1])


# ---- lifecycle -----------------------------------------------------------------------------------------------------
def test_fav_batch_between_kzg_calls_keeps_its_verdicts(S, items, mods):
    batch = mods.batch
    assert verify_batch(S.ctx, items[:3]) == (1, [1, 1, 1])
    n = 8
    pks = batch.sk_to_pk_batch(b"".join((i + 1).to_bytes(32, "big") for i in range(n)))
    batch.Registry().load(pks)
    committees = [[0, 1, 2], [3, 4], [5, 6, 7]]
    msgs = [hashlib.sha256(bytes([j])).digest() for j in range(3)]
    agg = [sum(k + 1 for k in c) % R for c in committees]
    sigs = bytearray(batch.sign_batch(b"".join(a.to_bytes(32, "big") for a in agg), b"".join(msgs)))
    sigs[96:192] = sigs[192:288]  # item 1 invalid
    idx = [k for c in committees for k in c]
    offs = batch.offsets_from_lengths([len(c) for c in committees])
    out = batch.fast_aggregate_verify_batch(idx, offs, b"".join(msgs), bytes(sigs))
    assert list(out) == [True, False, True]
    assert verify_batch(S.ctx, items[:3]) == (1, [1, 1, 1])
    assert S.blob_to_kzg_commitment(ZERO_BLOB) == ID
    assert list(batch.fast_aggregate_verify_batch(idx, offs, b"".join(msgs), bytes(sigs))) == [True, False, True]


def test_setup_lifecycle(items, ka, mods):
    """on a context of its own: no setup, a verify-only setup, a full one, and a replaced table"""
    native, batch, kzg = mods.native, mods.batch, mods.kzg
    L, _, G2 = K.trusted_setup()
    ctx = native.Context()
    try:
        assert verify_batch(ctx, items[:1])[0] == native.BLS_E_NOREG
        assert commitments_rc(ctx, [ZERO_BLOB])[0] == native.BLS_E_NOREG
        assert ctx.lib.bls_kzg_setup(ctx.h, G2[1], 0, 4096) == native.BLS_E_NOREG  # no table to name entries of
        assert ctx.lib.bls_kzg_setup(ctx.h, G2[1], 0, 17) == native.BLS_E_ARG
        assert ctx.lib.bls_kzg_setup(ctx.h, bytes([0x40]) + bytes(95), 0, 0) == 0
        assert verify_batch(ctx, items[:1])[0] == native.BLS_E_NOREG  # a failed setup is no setup
        v = kzg.KzgSetup.verify_only(G2[1], ctx=ctx)
        assert verify_batch(ctx, items[:2]) == (1, [1, 1])
        assert v.verify_kzg_proof(items[0][0], fe(items[0][1]), fe(items[0][2] ^ 1), items[0][3]) is False
        assert commitments_rc(ctx, [ZERO_BLOB])[0] == native.BLS_E_NOREG
        with pytest.raises(native.NativeError):
            v.compute_kzg_proof(ka[1].blob, fe(5))
        assert eval_blobs(ctx, [ka[1].blob], [fe(5)])[:2] == (1, [K.horner(ka[1].coeffs, 5)])  # needs no setup
        # a full setup behind two entries that are already there
        t = batch.G1Table(ctx)
        assert t.load([L[0], L[1]], subgroup_check=True).all()
        assert ctx.lib.bls_kzg_setup(ctx.h, G2[1], 2, 4096) == native.BLS_E_ARG  # entries out of range
        assert t.append(kzg.bit_reversal_permutation(list(L)), subgroup_check=True).all()
        assert ctx.lib.bls_kzg_setup(ctx.h, G2[1], 2, 4096) == 1
        assert commitments_rc(ctx, [ka[1].blob]) == (1, ka[1].commitment)
        # the table is replaced: commitments are refused until the setup is made again; verification goes on
        assert batch.G1Table(ctx).load([L[0]]).all()
        assert commitments_rc(ctx, [ka[1].blob])[0] == native.BLS_E_ARG
        assert verify_batch(ctx, items[:2]) == (1, [1, 1])
        s = kzg.KzgSetup(L, G2[1], ctx=ctx)
        assert s.first == 0 and s.blob_to_kzg_commitment(ka[1].blob) == ka[1].commitment
    finally:
        ctx.close()


# ---- verification at size (tests/seam_sizes.py) --------------------------------------------------------------------
def spoil_y(it):
    return (it[0], it[1], (it[2] + 1) % R, it[3])


def shift_proof(it, k):
    """the item with its proof moved by [k] G1"""
    return (it[0], it[1], it[2], O.g1_compress(O.g1_add(O.g1_decompress(it[3]), O.g1_mul(O.G1_GEN, k % R))))


@pytest.mark.parametrize("n", Z.KZG_VALID)
def test_valid_batches_across_the_stride_and_the_sum_switches(S, n):
    """n = 256, 257 (a lane of k_kzg_rlc takes a second item), 1,023, 1,024 (the first sum's 2 n + 1 points pass
    2,048: k_g1_sum_q, then the two-pass sum), 2,048, 2,049 (the second sum's n points pass it); linear, cubic and
    zero polynomials mixed, a z of its own per item"""
    items = list(K.batch_items(n))
    assert verify_batch(S.ctx, items) == (1, [1] * n)
    assert verify_batch(S.ctx, items, want_items=False)[0] == 1


@pytest.mark.parametrize("n", Z.KZG_FAILING)
def test_failing_batches_name_exactly_the_bad_items(S, n):
    """y spoiled at 0, 255, 256 and n - 1: the batch check fails and the per-item path (2 n pairs on the two-pair
    kernel, n selected final checks) names those (three for n = 257, whose last item is 256) and no other"""
    items = list(K.batch_items(n))
    bad = sorted({p % n for p in Z.KZG_BAD_AT})
    assert bad == {257: [0, 255, 256], 1024: [0, 255, 256, 1023]}[n]
    for p in bad:
        items[p] = spoil_y(items[p])
    assert verify_batch(S.ctx, items) == (0, [int(i not in bad) for i in range(n)])
    assert verify_batch(S.ctx, items, want_items=False)[0] == 0


@pytest.mark.parametrize("distance", [Z.RLC_LANES, 64])
def test_offsetting_errors_across_the_lane_stride_fail(S, distance):
    """Items i and i + distance carry the same (C, z, y) with proofs pi + D and pi - D: their errors r_i D (tau - z)
    and -r_j D (tau - z) cancel exactly when r_i = r_j.  This test fails if r_i repeats with the lane count of
    k_kzg_rlc (i taken mod 256 in the hash input, or item i + 256 given lane i's scalar row): every valid batch
    and every batch with one bad item would still get its right verdict.  Distance 64 is the same for a wave."""
    n = 300
    i, j = 3, 3 + distance
    items = list(K.batch_items(n))
    base = items[i]
    assert base[3] != ID and i % 16 != 15
    items[i], items[j] = shift_proof(base, 11), shift_proof(base, -11)
    assert verify_batch(S.ctx, items) == (0, [int(k not in (i, j)) for k in range(n)])
    assert verify_batch(S.ctx, items, want_items=False)[0] == 0
    items[j] = base
    assert verify_batch(S.ctx, items) == (0, [int(k != i) for k in range(n)])


# ---- the Python calls' chunking -------------------------------------------------------------------------------------
def test_list_calls_join_their_chunks_in_order(S, ka, items, mods, monkeypatch):
    """MSM_ROWS_MAX = 2, BLOBS_MAX = 2 and ITEMS_MAX = 4 in place of 511, 1,024 and 65,536: five blobs and eleven
    items go through every list-taking call in three chunks each; the outputs are the known answers in order, and a
    bad item of the last chunk is named at its position in the whole list"""
    kzg = mods.kzg
    monkeypatch.setattr(kzg, "MSM_ROWS_MAX", 2)
    monkeypatch.setattr(kzg, "BLOBS_MAX", 2)
    monkeypatch.setattr(kzg, "ITEMS_MAX", 4)
    answers = [ka[1], ka[0], None, ka[2], ka[1]]  # None: the zero blob
    blobs = [a.blob if a else ZERO_BLOB for a in answers]
    zs = [0x5EED, 77, 5, 99, K.DOMAIN[15]]
    opened = [a.open(z) if a else (0, ID) for a, z in zip(answers, zs)]
    s0 = mods.batch.g1_table_stats(S.ctx)
    assert S.blob_to_kzg_commitments(blobs) == [a.commitment if a else ID for a in answers]
    s1 = mods.batch.g1_table_stats(S.ctx)
    assert s1[0] - s0[0] == 3  # chunks of 2, 2 and 1 rows
    assert S.compute_kzg_proofs(blobs, zs) == [(proof, fe(y)) for y, proof in opened]
    assert mods.batch.g1_table_stats(S.ctx)[0] - s1[0] == 3
    assert S.evaluate_blobs(blobs, zs) == [fe(y) for y, _ in opened]
    # eleven items in chunks of 4, 4 and 3
    eleven = (items + items)[:11]
    cols = [list(c) for c in zip(*eleven)]
    assert S.verify_kzg_proof_items(*cols) == [True] * 11
    for bad in (9, 10, 4):
        spoiled = eleven[:bad] + [spoil_y(eleven[bad])] + eleven[bad + 1:]
        assert S.verify_kzg_proof_items(*[list(c) for c in zip(*spoiled)]) == [k != bad for k in range(11)], bad
    # five blobs with their commitments and proofs at the Fiat-Shamir challenge, in chunks of 2, 2 and 1
    cms = [a.commitment if a else ID for a in answers]
    proofs = [a.open(kzg.compute_challenge(b, c))[1] if a else ID for a, b, c in zip(answers, blobs, cms)]
    assert S.verify_blob_kzg_proof_items(blobs, cms, proofs) == [True] * 5
    assert S.verify_blob_kzg_proof_batch(blobs, cms, proofs) is True
    for bad in (4, 2):
        wrong = proofs[:bad] + [ka[1].commitment] + proofs[bad + 1:]
        assert S.verify_blob_kzg_proof_items(blobs, cms, wrong) == [k != bad for k in range(5)], bad
