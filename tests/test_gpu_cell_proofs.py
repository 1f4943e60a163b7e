"""GPU tests of the G1 transform and the device cell proofs (bls_g1_fft, bls_kzg_cell_proofs_setup,
bls_kzg_compute_cells_and_proofs, bls_kzg_recover_cells_and_proofs; batch.g1_fft, kzg_cells.CellProofSetup): the
transform against the oracle's direct sums, the monomial setup derived from the Lagrange one against the fixture's 66
reference-made points, proofs against known answers that do not depend on the device, against the verification
equation (which has one solution per commitment and cell) and against the direct quotient form on the table MSM,
batches on both sides of the blobs-per-MSM seam, the zero padding's cost, recovery, the setup's lifecycle,
interleaving with the other KZG calls and the Python calls' chunking.  Every comparison is exact on bytes.  The
trusted setup comes from tests/golden/trusted_setup.json only."""
import ctypes
import functools
import os
import random
import re

import numpy as np
import pytest

import cell_inputs as C
import g1fft_inputs as G
import kzg_inputs as K
from dispatch_edge_inputs import non_subgroup_g1
from oracle import bls_oracle as O

pytestmark = pytest.mark.gpu

R = K.R
ID = K.IDENTITY48
BLS_E_ARG, BLS_E_NOREG = -2, -3
CELLS_BYTES, PROOFS_BYTES = C.EXT_N * 32, 128 * 48
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mods():
    import types

    from bls_mi355x import _native, batch, kzg, kzg_cells

    return types.SimpleNamespace(native=_native, batch=batch, kzg=kzg, kc=kzg_cells)


@pytest.fixture(scope="module")
def P(mods):
    """On the default context, in a table of its own: the blob setup (Lagrange points), the cell setup (64 monomial
    points appended) and the proof setup made from the Lagrange list (the 4,096 derived points appended) -- the
    derivation runs once, here.  ks / cs / ps: the three setups; mono: the derived monomial points."""
    import types

    from bls_mi355x import curve

    curve.use_g1_table(None)
    L, M, G2 = K.trusted_setup()
    ks = mods.kzg.KzgSetup(L, G2[1])
    cs = mods.kc.CellSetup(ks, M[:64], G2[64])
    gen = ks.table._generation()
    ps = mods.kc.CellProofSetup(cs, g1_lagrange=L)
    assert ps.table is ks.table and ps.first == 4096 + 64 and ks.table._generation() == gen
    assert len(ps.g1_monomial) == 4096 and ks.table.run_of(ps.g1_monomial) == ps.first
    return types.SimpleNamespace(ks=ks, cs=cs, ps=ps, mono=ps.g1_monomial, ctx=ps.ctx)


def proofs_raw(ctx, blobs, want_cells=True):
    B = len(blobs)
    cells = ctypes.create_string_buffer(max(CELLS_BYTES * B, 1))
    proofs = ctypes.create_string_buffer(max(PROOFS_BYTES * B, 1))
    ok = np.full(B, 7, dtype=np.uint8)
    rc = ctx.lib.bls_kzg_compute_cells_and_proofs(ctx.h, b"".join(blobs), B, cells if want_cells else None, proofs,
                                                  ok.ctypes.data_as(ctypes.c_void_p))
    return rc, cells.raw[:CELLS_BYTES * B], proofs.raw[:PROOFS_BYTES * B], ok.tolist()


def fft_raw(ctx, pts, n, B, inverse=0):
    out = ctypes.create_string_buffer(max(48 * n * B, 48))
    return ctx.lib.bls_g1_fft(ctx.h, b"".join(pts), n, B, inverse, out), out.raw


def a_k(k: int) -> int:
    """h_k^64 = w_128^brp7(k)"""
    return pow(C.shift(k), 64, R)


@functools.lru_cache(maxsize=None)
def degree_129():
    """(coefficients, blob bytes) of a seeded polynomial with 130 coefficients"""
    rng = random.Random(0xD129)
    coeffs = [rng.randrange(R) for _ in range(130)]
    return coeffs, K.blob_bytes(K.poly_blob(coeffs))


def monomial_blob(*exponents) -> bytes:
    """the blob of sum X^e"""
    return K.blob_bytes([sum(pow(w, e, R) for e in exponents) % R for w in K.DOMAIN])


@functools.lru_cache(maxsize=None)
def three_blobs():
    """random, zero, degree 129"""
    return C.blobs()[0][1], C.blobs()[1][1], degree_129()[1]


@pytest.fixture(scope="module")
def singles(P):
    """the single-blob results (cells, proofs) of three_blobs(), each from a call of its own"""
    return [P.ps.compute_cells_and_kzg_proofs(b) for b in three_blobs()]


# ---- 1. the transform ----------------------------------------------------------------------------------------------
def test_small_transforms_against_the_oracles_direct_sums(P, mods):
    seen = set()
    for n, inverse, vecs, wants in G.cases():
        for vec, want in zip(vecs, wants):
            assert mods.batch.g1_fft(vec, inverse=inverse, ctx=P.ctx) == want, (n, inverse)
        if len(vecs) == 3:  # B = 3 vectors in one call
            assert mods.batch.g1_fft(vecs, inverse=inverse, ctx=P.ctx) == wants
            rc, raw = fft_raw(P.ctx, [p for v in vecs for p in v], n, 3, int(inverse))
            assert rc == 1 and raw == b"".join(p for w in wants for p in w)
        seen.add(n)
    assert seen == {2, 4, 8}


def test_transform_refusals(P, mods):
    g, outside = O.g1_compress(O.G1_GEN), O.g1_compress(non_subgroup_g1())
    assert fft_raw(P.ctx, [g] * 3, 3, 1)[0] == BLS_E_ARG
    assert fft_raw(P.ctx, [g] * 1, 1, 1)[0] == BLS_E_ARG
    assert fft_raw(P.ctx, [g] * 4, 4, 0)[0] == BLS_E_ARG
    assert P.ctx.lib.bls_g1_fft(P.ctx.h, g * 4, 8192, 1, 0, ctypes.create_string_buffer(48)) == BLS_E_ARG
    assert fft_raw(P.ctx, [g, outside, g, ID], 4, 1)[0] == 0        # on the curve, not in G1
    assert fft_raw(P.ctx, [g, g, bytes(48), g], 4, 1)[0] == 0                  # no encoding
    assert fft_raw(P.ctx, [ID] * 4, 4, 1) == (1, ID * 4)                       # the identity is valid
    with pytest.raises(ValueError):
        mods.batch.g1_fft([g] * 3, ctx=P.ctx)
    with pytest.raises(ValueError):
        mods.batch.g1_fft([g, outside], ctx=P.ctx)


# ---- 2. the monomial points ----------------------------------------------------------------------------------------
def test_derived_monomial_points_are_the_fixtures(P, mods):
    """the 66 recorded monomial points are the reference's own: a known answer of the 4,096-point transform"""
    L, M, _ = K.trusted_setup()
    assert len(M) == 66 and P.mono[:66] == M
    assert P.mono[0] == O.g1_compress(O.G1_GEN)
    # the inverse transform gives the Lagrange list back: in the file's order, which is the natural order of the
    # domain (entry j belongs to w^j; the bit reversal is applied where the list meets a blob), so none is undone here
    assert mods.batch.g1_fft(P.mono, inverse=True, ctx=P.ctx) == L


# ---- 3. known answers ----------------------------------------------------------------------------------------------
def test_degree_129_against_the_oracle(P, singles):
    coeffs, _ = degree_129()
    h0 = O.g1_decompress(K.commit_monomial(coeffs[64:130]))
    h1 = O.g1_decompress(K.commit_monomial(coeffs[128:130]))
    want = [O.g1_compress(O.g1_add(h0, O.g1_mul(h1, a_k(k)))) for k in range(128)]
    cells, proofs = singles[2]
    assert proofs == want
    assert cells == C.cells_of(C.extend_coeffs(coeffs))


def test_cell_answers_of_degree_0_63_64_65(P):
    ans = C.cell_answers()
    out = P.ps.compute_cells_and_kzg_proofs_batch([K.blob_bytes(K.poly_blob(a.coeffs)) for a in ans])
    assert out[0][1] == [ID] * 128 and out[1][1] == [ID] * 128
    assert out[2][1] == [ans[2].proof] * 128 and out[3][1] == [ans[3].proof] * 128
    assert ans[2].proof != ID and ans[3].proof != ans[2].proof
    for a, (cells, _) in zip(ans, out):
        for k in C.EDGE_CELLS:
            assert cells[k] == a.cell(k)


# ---- 4. full degree, by uniqueness ---------------------------------------------------------------------------------
def test_full_degree_proofs_satisfy_the_verification_equation(P):
    """The equation has exactly one solution pi_k for a commitment and a cell, so an accepted proof is the right
    group element and its compression the canonical one."""
    blobs = [three_blobs()[0], three_blobs()[1], monomial_blob(4095), monomial_blob(4032, 64)]
    out = P.ps.compute_cells_and_kzg_proofs_batch(blobs)
    cms = P.ks.blob_to_kzg_commitments(blobs)
    items = [(cms[b], k, out[b][0][k], out[b][1][k]) for b in range(4) for k in range(128)]
    cols = lambda its: ([i[0] for i in its], [i[1] for i in its], [i[2] for i in its], [i[3] for i in its])
    assert P.cs.verify_cell_kzg_proof_items(*cols(items)) == [True] * 512
    assert out[1][1] == [ID] * 128 and cms[1] == ID  # the zero blob
    assert len(set(out[0][1])) == 128 and ID not in out[2][1]
    # a proof moved by G1 is another point of G1: that item alone fails
    moved = list(items[128 * 3:])
    c, i, cell, proof = moved[77]
    moved[77] = (c, i, cell, O.g1_compress(O.g1_add(O.g1_decompress(proof), O.G1_GEN)))
    assert P.cs.verify_cell_kzg_proof_items(*cols(moved)) == [j != 77 for j in range(128)]
    # one bit of one proof's x flipped: the item alone fails, or (x on no point of G1) the decode assertion
    flipped = list(items[:128])
    c, i, cell, proof = flipped[5]
    flipped[5] = (c, i, cell, proof[:47] + bytes([proof[47] ^ 1]))
    try:
        got = P.cs.verify_cell_kzg_proof_items(*cols(flipped))
    except AssertionError:
        got = None
    assert got is None or got == [j != 5 for j in range(128)]


# ---- 5. full degree, the direct form -------------------------------------------------------------------------------
def test_full_degree_proofs_equal_the_direct_quotients_commitment(P, mods, singles):
    coeffs = C.blob_coeffs(C.blobs()[0][0])
    idx = np.arange(P.ps.first, P.ps.first + 4032, dtype=np.uint32)
    for k in C.EDGE_CELLS:
        a = a_k(k)
        q = [0] * 4096  # p = (X^64 - a) q + I: q_i = p_{i + 64} + a q_{i + 64}
        for i in range(4031, -1, -1):
            q[i] = (coeffs[i + 64] + a * q[i + 64]) % R
        assert mods.batch.g1_lincomb_indexed(P.ps.table, idx, q[:4032]) == singles[0][1][k], k


# ---- 6. batches ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ["one", "per_msm", "per_msm_plus_one"])
def test_batches_on_both_sides_of_the_msm_seam(P, mods, singles, size):
    """B = 1, PROOF_BLOBS_PER_MSM and one more: every blob's result is its single-blob result"""
    per = mods.kc.PROOF_BLOBS_PER_MSM
    B = {"one": 1, "per_msm": per, "per_msm_plus_one": per + 1}[size]
    blobs = [three_blobs()[i % 3] for i in range(B)]
    out = P.ps.compute_cells_and_kzg_proofs_batch(blobs)
    assert out == [singles[i % 3] for i in range(B)]
    assert [o[0] for o in out] == P.cs.compute_cells_batch(blobs)
    rc, cells, proofs, ok = proofs_raw(P.ctx, blobs, want_cells=False)
    assert (rc, ok) == (1, [1] * B) and proofs == b"".join(b"".join(singles[i % 3][1]) for i in range(B))


def test_a_non_canonical_blob_is_marked_alone(P, singles):
    bad = bytearray(three_blobs()[0])
    bad[32 * 2048: 32 * 2049] = R.to_bytes(32, "big")
    blobs = [three_blobs()[2], bytes(bad), three_blobs()[0]]
    rc, cells, proofs, ok = proofs_raw(P.ctx, blobs)
    assert (rc, ok) == (0, [1, 0, 1])
    assert cells == b"".join(singles[2][0]) + bytes(CELLS_BYTES) + b"".join(singles[0][0])
    assert proofs == b"".join(singles[2][1]) + bytes(PROOFS_BYTES) + b"".join(singles[0][1])
    with pytest.raises(AssertionError):
        P.ps.compute_cells_and_kzg_proofs(bytes(bad))
    with pytest.raises(AssertionError):
        P.ps.compute_cells_and_kzg_proofs_batch(blobs)
    assert proofs_raw(P.ctx, []) == (1, b"", b"", [])
    assert P.ctx.lib.bls_kzg_compute_cells_and_proofs(P.ctx.h, blobs[0], 1, None, None, None) == BLS_E_ARG
    assert P.ctx.lib.bls_kzg_compute_cells_and_proofs(P.ctx.h, blobs[0], 129, None, ctypes.create_string_buffer(48),
                                                      None) == BLS_E_ARG


# ---- 7. the zero padding -------------------------------------------------------------------------------------------
def test_zero_padding_costs_no_additions(P, mods, singles):
    text = open(os.path.join(ROOT, "eth-consensus-specs_amd", "csrc", "bls_g1_msm.h")).read()
    digits = int(re.search(r"constexpr int G1M_WINDOWS = (\d+);", text).group(1))
    nonzero = sum(4096 - 64 * (m + 1) for m in range(63))
    assert nonzero == 129024
    calls0, entries0, _ = mods.batch.g1_table_stats(P.ctx)
    assert P.ps.compute_cells_and_kzg_proofs(three_blobs()[0]) == singles[0]
    calls1, entries1, _ = mods.batch.g1_table_stats(P.ctx)
    assert calls1 == calls0 + 1
    assert 0 < entries1 - entries0 <= digits * nonzero


# ---- 8. recovery ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["odd", "random_64", "none"])
def test_recovery_gives_the_computed_cells_and_proofs(P, singles, name):
    missing = set(C.missing_sets()[name])
    idx = [k for k in range(128) if k not in missing]
    cells = singles[0][0]
    assert P.ps.recover_cells_and_kzg_proofs(idx, [cells[k] for k in idx]) == singles[0]


def test_recovery_of_two_blobs_in_one_call(P, singles):
    idx = [k for k in range(128) if k not in set(C.missing_sets()["odd"])]
    a, b = singles[0][0], singles[2][0]
    out = P.ps.recover_cells_and_kzg_proofs_batch(idx, [[a[k] for k in idx], [b[k] for k in idx]])
    assert out == [singles[0], singles[2]]


def test_recovery_refusals(P, singles):
    cells = singles[0][0]
    with pytest.raises(AssertionError):
        P.ps.recover_cells_and_kzg_proofs(list(range(63)), cells[:63])
    with pytest.raises(AssertionError):
        P.ps.recover_cells_and_kzg_proofs([1, 0] + list(range(2, 64)), cells[:64])
    c = P.ctx
    out, pf = ctypes.create_string_buffer(CELLS_BYTES), ctypes.create_string_buffer(PROOFS_BYTES)
    for idx in (list(range(63)), [1, 0] + list(range(2, 64)), list(range(63)) + [62], list(range(63)) + [128]):
        a = np.asarray(idx, dtype=np.uint32)
        args = (c.h, a.ctypes.data_as(ctypes.c_void_p), len(idx), b"".join(cells[:64]), 1, out)
        assert c.lib.bls_kzg_recover_cells_and_proofs(*args, pf, None) == BLS_E_ARG, idx
        assert c.lib.bls_kzg_recover_cells(*args, None) == BLS_E_ARG, idx
    bad = bytearray(cells[5])
    bad[:32] = R.to_bytes(32, "big")
    a = np.arange(64, dtype=np.uint32)
    ok = np.full(2, 7, dtype=np.uint8)
    two = b"".join(cells[:64]) + b"".join(cells[:5] + [bytes(bad)] + cells[6:64])
    out2, pf2 = ctypes.create_string_buffer(2 * CELLS_BYTES), ctypes.create_string_buffer(2 * PROOFS_BYTES)
    rc = c.lib.bls_kzg_recover_cells_and_proofs(c.h, a.ctypes.data_as(ctypes.c_void_p), 64, two, 2, out2, pf2,
                                                ok.ctypes.data_as(ctypes.c_void_p))
    assert (rc, ok.tolist()) == (0, [1, 0])
    assert out2.raw == b"".join(cells) + bytes(CELLS_BYTES)
    assert pf2.raw == b"".join(singles[0][1]) + bytes(PROOFS_BYTES)
    assert c.lib.bls_kzg_recover_cells_and_proofs(c.h, a.ctypes.data_as(ctypes.c_void_p), 64, two, 2, out2, None,
                                                  None) == BLS_E_ARG


# ---- 9. lifecycle --------------------------------------------------------------------------------------------------
def test_setup_lifecycle(P, mods, singles):
    """on a context of its own: no setup, no table, a cell setup first, the proof setup appended behind it, the table
    replaced, the setup made again"""
    ctx = mods.native.Context(0)
    try:
        _, M, G2 = K.trusted_setup()
        blob = three_blobs()[2]
        want = (1, b"".join(singles[2][0]), b"".join(singles[2][1]), [1])
        assert proofs_raw(ctx, [blob])[0] == BLS_E_NOREG
        assert proofs_raw(ctx, [])[0] == BLS_E_NOREG
        assert ctx.lib.bls_kzg_cell_proofs_setup(ctx.h, 0, 4096) == BLS_E_NOREG  # no table
        cs = mods.kc.CellSetup(ctx, M[:64], G2[64])
        assert ctx.lib.bls_kzg_cell_proofs_setup(ctx.h, 0, 4096) == BLS_E_ARG   # past the table's end
        assert ctx.lib.bls_kzg_cell_proofs_setup(ctx.h, 0, 64) == BLS_E_ARG
        assert proofs_raw(ctx, [blob])[0] == BLS_E_NOREG
        gen = cs.table._generation()
        ps = mods.kc.CellProofSetup(cs, g1_monomial=P.mono)
        assert (ps.first, len(ps.table), cs.table._generation()) == (64, 64 + 4096, gen)
        assert proofs_raw(ctx, [blob]) == want
        # the cell setup made before it still verifies
        cm = C.cell_answers()[3]
        assert cs.verify_cell_kzg_proof_batch(*zip(*[cm.item(k) for k in C.EDGE_CELLS])) is True
        again = mods.kc.CellProofSetup(cs, g1_monomial=P.mono)  # found as a run: nothing appended
        assert (again.first, len(again.table)) == (64, 64 + 4096)
        assert ctx.lib.bls_kzg_cell_proofs_setup(ctx.h, 64, 4095) == BLS_E_ARG
        assert proofs_raw(ctx, [blob]) == want  # a call refused for its count leaves the setup
        assert ctx.lib.bls_kzg_cell_proofs_setup(ctx.h, 65, 4096) == BLS_E_ARG  # past the table's end ...
        assert proofs_raw(ctx, [blob])[0] == BLS_E_NOREG  # ... and the setup is gone, as after bls_kzg_cells_setup's
        again.setup()
        assert proofs_raw(ctx, [blob]) == want
        assert cs.table.load(M[:64], subgroup_check=True).all()  # the table is replaced
        assert proofs_raw(ctx, [blob])[0] == BLS_E_ARG
        idx = np.arange(64, dtype=np.uint32)
        out, pf = ctypes.create_string_buffer(CELLS_BYTES), ctypes.create_string_buffer(PROOFS_BYTES)
        assert ctx.lib.bls_kzg_recover_cells_and_proofs(ctx.h, idx.ctypes.data_as(ctypes.c_void_p), 64,
                                                        b"".join(singles[2][0][:64]), 1, out, pf, None) == BLS_E_ARG
        ps2 = mods.kc.CellProofSetup(ctx, g1_monomial=P.mono)  # a table of its own
        assert ps2.first == 0 and proofs_raw(ctx, [blob]) == want
    finally:
        ctx.close()


# ---- 10. interleaving ----------------------------------------------------------------------------------------------
def test_proof_calls_interleaved_with_the_other_kzg_calls(P, singles):
    """a proof call, a cell verification, a recovery and a blob verification, twice: the S_KP_*, S_KC_*, S_G1M_* and
    S_KB_* scratch do not collide"""
    blob = three_blobs()[0]
    cells, proofs = singles[0]
    cm = P.ks.blob_to_kzg_commitment(blob)
    blob_proof = P.ks.compute_blob_kzg_proof(blob, cm)
    ks = (0, 1, 64, 127, 63, 5)
    idx = list(range(0, 128, 2))
    for _ in range(2):
        assert P.ps.compute_cells_and_kzg_proofs_batch([blob, three_blobs()[2]]) == [singles[0], singles[2]]
        assert P.cs.verify_cell_kzg_proof_batch([cm] * len(ks), ks, [cells[k] for k in ks],
                                                [proofs[k] for k in ks]) is True
        assert P.cs.recover_cells(idx, [cells[k] for k in idx]) == cells
        assert P.ks.verify_blob_kzg_proof(blob, cm, blob_proof) is True
        assert P.ps.recover_cells_and_kzg_proofs(idx, [cells[k] for k in idx]) == singles[0]


# ---- 11. chunking --------------------------------------------------------------------------------------------------
def test_list_calls_join_their_chunks_in_order(P, mods, singles, monkeypatch):
    monkeypatch.setattr(mods.kc, "BLOBS_MAX", 2)
    order = [0, 2, 1, 2, 0]
    blobs = [three_blobs()[i] for i in order]
    assert P.ps.compute_cells_and_kzg_proofs_batch(blobs) == [singles[i] for i in order]
    idx = list(range(64, 128))
    given = [[singles[i][0][k] for k in idx] for i in order]
    assert P.ps.recover_cells_and_kzg_proofs_batch(idx, given) == [singles[i] for i in order]
