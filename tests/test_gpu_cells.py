"""GPU tests of the device cell KZG functions (bls_kzg_cells_setup, bls_kzg_verify_cells, bls_kzg_compute_cells,
bls_kzg_recover_cells; bls_mi355x.kzg_cells): batch verification of known answers from the monomial setup with every
way of being wrong and per-item verdicts, cells against the Python FFT of cell_inputs.py, recovery against the full
extension and against the restatement of the spec's algorithm, the setup's lifecycle, verification at the sizes where
the call changes shape (seam_sizes.py) and the Python calls' chunking.  The trusted setup comes from the fixture
tests/golden/trusted_setup.json only."""
import ctypes
import functools

import numpy as np
import pytest

import cell_inputs as C
import kzg_inputs as K
import seam_sizes as Z
from dispatch_edge_inputs import non_subgroup_g1
from oracle import bls_oracle as O

pytestmark = pytest.mark.gpu

R = K.R
ID = K.IDENTITY48
ZERO_CELL = bytes(2048)
BLS_E_ARG, BLS_E_NOREG = -2, -3


@pytest.fixture(scope="module")
def mods():
    import types

    from bls_mi355x import _native, batch, kzg, kzg_cells

    return types.SimpleNamespace(native=_native, batch=batch, kzg=kzg, kc=kzg_cells)


@pytest.fixture(scope="module")
def S(mods):
    """the cell setup on the default context, in a table of its own (whatever another module left there goes)"""
    from bls_mi355x import curve

    curve.use_g1_table(None)
    _, M, G2 = K.trusted_setup()
    table = mods.batch.G1Table(mods.native.context())
    assert table.load(M[:64], subgroup_check=True).all()
    curve.use_g1_table(table)
    try:
        yield mods.kc.CellSetup(None, M[:64], G2[64])
    finally:
        curve.use_g1_table(None)


# ---- raw C ABI helpers ---------------------------------------------------------------------------------------------
def verify_raw(ctx, items, want_items=True, commitments=None, index=None):
    """bls_kzg_verify_cells on (commitment, cell index, cell, proof) items; the commitment table is the items' own
    commitments one by one unless given"""
    n = len(items)
    cm = commitments if commitments is not None else [i[0] for i in items]
    idx = np.asarray(index if index is not None else list(range(n)), dtype=np.uint32)
    cells = np.asarray([i[1] for i in items], dtype=np.uint32)
    out = np.full(n, 7, dtype=np.uint8)
    rc = ctx.lib.bls_kzg_verify_cells(ctx.h, b"".join(cm), len(cm), idx.ctypes.data_as(ctypes.c_void_p),
                                      cells.ctypes.data_as(ctypes.c_void_p), b"".join(i[2] for i in items),
                                      b"".join(i[3] for i in items), n,
                                      out.ctypes.data_as(ctypes.c_void_p) if want_items else None)
    return rc, out.tolist()


def cells_raw(ctx, blobs):
    B = len(blobs)
    out, ok = ctypes.create_string_buffer(C.EXT_N * 32 * B), np.full(B, 7, dtype=np.uint8)
    rc = ctx.lib.bls_kzg_compute_cells(ctx.h, b"".join(blobs), B, out, ok.ctypes.data_as(ctypes.c_void_p))
    return rc, out.raw, ok.tolist()


def add_g1(p48: bytes, k: int) -> bytes:
    """p + [k] G1"""
    return O.g1_compress(O.g1_add(O.g1_decompress(p48), O.g1_mul(O.G1_GEN, k % R)))


def unzip(items):
    return [i[0] for i in items], [i[1] for i in items], [i[2] for i in items], [i[3] for i in items]


# ---- verification --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 65, 129, 257])
def test_valid_batches_of_mixed_degrees(S, n):
    """degrees 0, 63, 64 and 65 mixed: one item, two, past a wave, past one cell per index (every cell index with 0,
    1, 63, 64 and 127 first; four items share each index) and past a 256-lane workgroup"""
    items = C.batch_items(n)
    if n >= 65:
        assert {0, 1, 63, 64, 127} <= {i[1] for i in items}
    assert S.verify_cell_kzg_proof_batch(*unzip(items)) is True
    assert S.verify_cell_kzg_proof_items(*unzip(items)) == [True] * n
    rc, out = verify_raw(S.ctx, items)
    assert (rc, out) == (1, [1] * n)
    assert verify_raw(S.ctx, items, want_items=False)[0] == 1


@functools.lru_cache(maxsize=None)
def wrong_batches():
    """name -> (items, the indices that are wrong) on a batch of 9: each way of being wrong alone"""
    base = C.batch_items(9)  # items 0..3: cell 0 of the four polynomials, 4..7: cell 1, 8: cell 63 of degree 0
    out = {}
    it = list(base)
    cell = bytearray(it[5][2])
    cell[32 * 17 + 31] ^= 1  # element 17 off by one
    it[5] = (it[5][0], it[5][1], bytes(cell), it[5][3])
    out["element_off_by_one"] = (it, [5])
    it = list(base)  # items 3 (degree 65, cell 0) and 6 (degree 64, cell 1) swap their cell indices
    it[3], it[6] = (it[3][0], it[6][1], it[3][2], it[3][3]), (it[6][0], it[3][1], it[6][2], it[6][3])
    out["cell_indices_swapped"] = (it, [3, 6])
    it = list(base)  # the proof of another polynomial's cell (one polynomial's cells all share a proof)
    it[2] = (it[2][0], it[2][1], it[2][2], base[3][3])
    out["another_cells_proof"] = (it, [2])
    it = list(base)
    it[7] = (base[6][0], it[7][1], it[7][2], it[7][3])
    out["another_polynomials_commitment"] = (it, [7])
    it = list(base)
    it[0] = (it[0][0], it[0][1], it[0][2], add_g1(it[0][3], 3))
    out["proof_plus_small_multiple"] = (it, [0])
    return out


@pytest.mark.parametrize("name", ["element_off_by_one", "cell_indices_swapped", "another_cells_proof",
                                  "another_polynomials_commitment", "proof_plus_small_multiple"])
def test_each_way_of_being_wrong_is_named(S, name):
    items, bad = wrong_batches()[name]
    want = [k not in bad for k in range(len(items))]
    assert S.verify_cell_kzg_proof_items(*unzip(items)) == want
    assert S.verify_cell_kzg_proof_batch(*unzip(items)) is False
    rc, out = verify_raw(S.ctx, items)
    assert (rc, out) == (0, [int(v) for v in want])
    assert verify_raw(S.ctx, items, want_items=False)[0] == 0


def test_offsetting_errors_on_one_cell_index_fail(S):
    """two items with the same cell index whose proofs are pi + D and pi' - D: their errors cancel under equal
    coefficients, not under independent ones"""
    a, b = C.cell_answers()[2], C.cell_answers()[3]
    ia, ib = a.item(5), b.item(5)
    items = [(ia[0], 5, ia[2], add_g1(ia[3], 11)), (ib[0], 5, ib[2], add_g1(ib[3], -11)), C.cell_answers()[1].item(5)]
    assert S.verify_cell_kzg_proof_items(*unzip(items)) == [False, False, True]
    assert S.verify_cell_kzg_proof_batch(*unzip(items)) is False


def test_invalid_inputs_raise_in_python_and_are_named_by_the_c_call(S):
    base = C.batch_items(3)
    bad_cell = bytearray(base[1][2])
    bad_cell[32 * 63: 32 * 64] = R.to_bytes(32, "big")  # the last element is r
    off = O.g1_compress(non_subgroup_g1())
    cases = [
        [base[0], (base[1][0], base[1][1], bytes(bad_cell), base[1][3]), base[2]],
        [base[0], (base[1][0], base[1][1], base[1][2], off), base[2]],
        [base[0], (base[1][0], 128, base[1][2], base[1][3]), base[2]],
        [base[0], (off, base[1][1], base[1][2], base[1][3]), base[2]],
    ]
    for n, items in enumerate(cases):
        with pytest.raises(AssertionError):
            S.verify_cell_kzg_proof_batch(*unzip(items))
            pytest.fail("case %d reached no assertion" % n)
        assert verify_raw(S.ctx, items) == (0, [1, 0, 1]), n
    with pytest.raises(AssertionError):
        S.verify_cell_kzg_proof_batch(*unzip(base[:2] + [base[2][:3] + (base[2][3][:47],)]))
    assert verify_raw(S.ctx, base, index=[0, 1, 3])[0] == BLS_E_ARG  # a commitment index past the table


def test_identity_zero_cell_and_empty_batch(S):
    assert S.verify_cell_kzg_proof_batch([ID], [0], [ZERO_CELL], [ID]) is True
    assert S.verify_cell_kzg_proof_batch([ID, ID], [127, 64], [ZERO_CELL, ZERO_CELL], [ID, ID]) is True
    one = bytes(31) + b"\x01"
    assert S.verify_cell_kzg_proof_items([ID], [3], [ZERO_CELL[:-32] + one], [ID]) == [False]
    assert S.verify_cell_kzg_proof_batch([], [], [], []) is True
    assert verify_raw(S.ctx, [])[0] == 1


def test_duplicated_commitments_give_the_deduped_calls_verdicts(S):
    """33 items of two polynomials with one item wrong: the Python call (which dedupes), the C call on the distinct
    table and the C call on a table with every item's own copy agree"""
    a, b = C.cell_answers()[1], C.cell_answers()[3]
    items = [(a if k % 2 else b).item(k % 128) for k in range(33)]
    items[20] = (items[20][0], items[20][1], items[21][2], items[20][3])
    want = [k != 20 for k in range(33)]
    assert S.verify_cell_kzg_proof_items(*unzip(items)) == want
    distinct = [b.commitment, a.commitment]
    rc, out = verify_raw(S.ctx, items, commitments=distinct, index=[k % 2 for k in range(33)])
    assert (rc, out) == (0, [int(v) for v in want])
    assert verify_raw(S.ctx, items) == (0, [int(v) for v in want])
    good = [(a if k % 2 else b).item(k % 128) for k in range(33)]
    assert verify_raw(S.ctx, good, commitments=distinct, index=[k % 2 for k in range(33)]) == (1, [1] * 33)


# ---- cells ---------------------------------------------------------------------------------------------------------
def test_cells_of_one_and_three_blobs(S, mods):
    """a random blob alone, then random, zero and degree-65 in one call: the bytes are the restatement's, the first
    64 cells are the blob, and the degree-65 blob's cells are Horner on the extended domain"""
    blobs = C.blobs()
    got = mods.kc.compute_cells(blobs[0][1])
    assert got == blobs[0][3]
    out = S.compute_cells_batch([b[1] for b in blobs])
    assert len(out) == 3 and all(len(cells) == 128 for cells in out)
    for cells, (_, blob, _, want) in zip(out, blobs):
        assert cells == want
        assert b"".join(cells[:64]) == blob
    ka = C.cell_answers()[3]
    for k in (0, 1, 63, 64, 127):
        assert out[2][k] == ka.cell(k)
    rc, raw, ok = cells_raw(S.ctx, [b[1] for b in blobs])
    assert (rc, ok) == (1, [1, 1, 1]) and raw == b"".join(b"".join(b[3]) for b in blobs)


def test_a_non_canonical_blob_is_marked_alone(S):
    blobs = C.blobs()
    bad = bytearray(blobs[0][1])
    bad[32 * 4095: 32 * 4096] = R.to_bytes(32, "big")
    rc, raw, ok = cells_raw(S.ctx, [blobs[2][1], bytes(bad), blobs[0][1]])
    assert (rc, ok) == (0, [1, 0, 1])
    n = C.EXT_N * 32
    assert raw[:n] == b"".join(blobs[2][3]) and raw[n: 2 * n] == bytes(n) and raw[2 * n:] == b"".join(blobs[0][3])
    with pytest.raises(AssertionError):
        S.compute_cells(bytes(bad))
    with pytest.raises(AssertionError):
        S.compute_cells(blobs[0][1][:-1])


# ---- recovery ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.missing_sets()))
def test_recovery_from_every_missing_set(S, name):
    missing = set(C.missing_sets()[name])
    idx = [k for k in range(128) if k not in missing]
    cells = C.blobs()[0][3]
    assert S.recover_cells(idx, [cells[k] for k in idx]) == cells


@pytest.mark.parametrize("name", ["odd", "random_17"])
def test_recovery_of_two_blobs_in_one_call(S, name):
    missing = set(C.missing_sets()[name])
    idx = [k for k in range(128) if k not in missing]
    a, b = C.blobs()[0][3], C.blobs()[2][3]
    out = S.recover_cells_batch(idx, [[a[k] for k in idx], [b[k] for k in idx]])
    assert out == [a, b]


def test_recovery_of_inconsistent_cells_is_the_specs_algorithm(S):
    """100 cells present, one element corrupted: the output is what the restatement of the spec's algorithm gives
    on the same input (not the original extension)"""
    cells = list(C.blobs()[0][3])
    idx = sorted(set(range(128)) - set(C.missing_sets()["random_17"]))[:100]
    assert len(idx) == 100 and idx[-1] < 127
    bad = bytearray(cells[idx[40]])
    bad[32 * 9 + 31] ^= 1
    given = [bytes(bad) if k == idx[40] else cells[k] for k in idx]
    want = C.cells_of(C.recover(idx, [C.cell_ints(c) for c in given]))
    assert want != cells
    assert S.recover_cells(idx, given) == want


def test_recovery_refusals(S):
    cells = C.blobs()[0][3]
    with pytest.raises(AssertionError):
        S.recover_cells(list(range(63)), cells[:63])
    with pytest.raises(AssertionError):
        S.recover_cells([1, 0] + list(range(2, 64)), cells[:64])
    with pytest.raises(AssertionError):
        S.recover_cells(list(range(63)) + [62], cells[:64])
    c = S.ctx
    out = ctypes.create_string_buffer(C.EXT_N * 32)
    for idx in (list(range(63)), [1, 0] + list(range(2, 64)), list(range(63)) + [62], list(range(63)) + [128]):
        a = np.asarray(idx, dtype=np.uint32)
        rc = c.lib.bls_kzg_recover_cells(c.h, a.ctypes.data_as(ctypes.c_void_p), len(idx), b"".join(cells[:64]), 1,
                                         out, None)
        assert rc == BLS_E_ARG, idx
    bad = bytearray(cells[5])
    bad[:32] = R.to_bytes(32, "big")
    a = np.arange(64, dtype=np.uint32)
    ok = np.full(2, 7, dtype=np.uint8)
    two = b"".join(cells[:64]) + b"".join(cells[:5] + [bytes(bad)] + cells[6:64])
    out2 = ctypes.create_string_buffer(2 * C.EXT_N * 32)
    rc = c.lib.bls_kzg_recover_cells(c.h, a.ctypes.data_as(ctypes.c_void_p), 64, two, 2, out2,
                                     ok.ctypes.data_as(ctypes.c_void_p))
    assert (rc, ok.tolist()) == (0, [1, 0])
    assert out2.raw[: C.EXT_N * 32] == b"".join(cells) and out2.raw[C.EXT_N * 32:] == bytes(C.EXT_N * 32)


# ---- lifecycle -----------------------------------------------------------------------------------------------------
def test_deneb_and_cell_calls_interleaved_on_one_context(S, mods):
    """a blob evaluation and blob verification between cell calls: the S_KB_* and S_KC_* scratch do not collide"""
    ka = K.known_answers()[2]
    z = 0x1234567
    y, proof = ka.open(z)
    dk = mods.kzg.KzgSetup.verify_only(K.trusted_setup()[2][1], ctx=S.ctx)
    items = C.batch_items(5)
    for _ in range(2):
        assert S.verify_cell_kzg_proof_batch(*unzip(items)) is True
        assert dk.verify_kzg_proof(ka.commitment, z.to_bytes(32, "big"), y.to_bytes(32, "big"), proof) is True
        assert S.compute_cells(C.blobs()[2][1]) == C.blobs()[2][3]
        assert dk.evaluate_polynomial_in_evaluation_form(ka.blob, z) == y
        assert dk.verify_kzg_proof(ka.commitment, z.to_bytes(32, "big"), ((y + 1) % R).to_bytes(32, "big"),
                                   proof) is False


def test_setup_lifecycle(mods):
    """on a context of its own: no setup, a setup, the table replaced, the setup made again"""
    ctx = mods.native.Context(0)
    try:
        _, M, G2 = K.trusted_setup()
        items = C.batch_items(4)[2:]  # degree 64 and 65: their proofs are not the identity
        assert verify_raw(ctx, items)[0] == BLS_E_NOREG
        assert ctx.lib.bls_kzg_cells_setup(ctx.h, G2[64], 0, 64) == BLS_E_NOREG  # no table
        table = mods.batch.G1Table(ctx)
        assert table.load(M[:66], subgroup_check=True).all()
        assert ctx.lib.bls_kzg_cells_setup(ctx.h, G2[64], 0, 63) == BLS_E_ARG
        assert ctx.lib.bls_kzg_cells_setup(ctx.h, G2[64], 3, 64) == BLS_E_ARG  # past the table's end
        assert ctx.lib.bls_kzg_cells_setup(ctx.h, bytes(96), 0, 64) == 0  # not an encoding
        assert verify_raw(ctx, items)[0] == BLS_E_NOREG
        assert ctx.lib.bls_kzg_cells_setup(ctx.h, G2[64], 0, 64) == 1
        assert verify_raw(ctx, items) == (1, [1, 1])
        assert ctx.lib.bls_kzg_cells_setup(ctx.h, G2[63], 0, 64) == 1  # a wrong [tau^64] G2: nothing verifies
        assert verify_raw(ctx, items) == (0, [0, 0])
        assert ctx.lib.bls_kzg_cells_setup(ctx.h, G2[64], 0, 64) == 1
        assert table.load(M[:64], subgroup_check=True).all()  # the table is replaced
        assert verify_raw(ctx, items)[0] == BLS_E_ARG
        assert ctx.lib.bls_kzg_cells_setup(ctx.h, G2[64], 0, 64) == 1
        assert verify_raw(ctx, items) == (1, [1, 1])
        # cells and recovery need no setup
        rc, raw, ok = cells_raw(ctx, [C.blobs()[2][1]])
        assert (rc, ok) == (1, [1]) and raw == b"".join(C.blobs()[2][3])
    finally:
        ctx.close()


# ---- verification at size (tests/seam_sizes.py) --------------------------------------------------------------------
def deduped(items):
    """verify_raw's arguments for batch_items' four commitments as the table and every item's index into it"""
    distinct = [a.commitment for a in C.cell_answers()]
    assert len(set(distinct)) == Z.CELL_COMMITMENTS == len(distinct)
    return dict(commitments=distinct, index=[distinct.index(i[0]) for i in items])


def off_by_one(item, element):
    cell = bytearray(item[2])
    cell[32 * element + 31] ^= 1
    return (item[0], item[1], bytes(cell), item[3])


@pytest.mark.parametrize("n", Z.CELLS_VALID)
def test_valid_batches_across_the_sum_switches(S, n):
    """four commitments for n = 2,043 | 2,044 cells (the first sum's nc + n + 1 points pass 2,048: k_g1_sum_q, then
    the two-pass sum) and n = 2,048 | 2,049 (the second sum's n points pass it)"""
    items = C.batch_items(n)
    assert verify_raw(S.ctx, items, **deduped(items)) == (1, [1] * n)
    assert verify_raw(S.ctx, items, want_items=False, **deduped(items))[0] == 1


@pytest.mark.parametrize("n", Z.CELLS_FAILING)
def test_failing_batches_across_the_msm_chunks(S, n):
    """n = 511, 512, 1,023: the per-item path's interpolant commitments come from one table MSM of 511 rows, from
    511 + 1 and from 511 + 511 + 1, each chunk copied behind the one before.  One element of the cells at 0, 510,
    511 and n - 1 (those below n) is off by one: the call and the Python call name exactly those."""
    items = C.batch_items(n)
    bad = sorted({p % n for p in Z.CELLS_BAD_AT if p < n})
    assert len(bad) == {511: 2, 512: 3, 1023: 4}[n]
    for p in bad:
        items[p] = off_by_one(items[p], (7 * p + 3) % 64)
    want = [k not in bad for k in range(n)]
    assert verify_raw(S.ctx, items, **deduped(items)) == (0, [int(v) for v in want])
    assert verify_raw(S.ctx, items, want_items=False, **deduped(items))[0] == 0
    assert S.verify_cell_kzg_proof_items(*unzip(items)) == want
    # one bad cell alone, the first chunk's last row: a later chunk written over the first one's rows, or left out of
    # its own, would call good items bad (at n = 512 the positions above are exactly the rows that would hit)
    items = C.batch_items(n)
    lone = Z.KZC_MSM_ROWS - 1
    items[lone] = off_by_one(items[lone], 1)
    assert verify_raw(S.ctx, items, **deduped(items)) == (0, [int(k != lone) for k in range(n)])


def test_offsetting_errors_a_lane_stride_apart_fail(S):
    """items 7 and 7 + 256 name one cell index with proofs pi + D and pi' - D: the errors cancel exactly when both
    items get the same r.  This test fails if k_cells_rlc's r_k repeats with its 256 lanes, which no valid batch
    and no batch with a single bad item can show."""
    n = 300
    i, j = 7, 7 + Z.RLC_LANES
    a, b = C.cell_answers()[2], C.cell_answers()[3]
    ia, ib = a.item(5), b.item(5)
    items = C.batch_items(n)
    items[i] = (ia[0], 5, ia[2], add_g1(ia[3], 11))
    items[j] = (ib[0], 5, ib[2], add_g1(ib[3], -11))
    want = [k not in (i, j) for k in range(n)]
    assert verify_raw(S.ctx, items, **deduped(items)) == (0, [int(v) for v in want])
    assert S.verify_cell_kzg_proof_items(*unzip(items)) == want
    assert S.verify_cell_kzg_proof_batch(*unzip(items)) is False


def test_more_cells_than_a_call_takes_is_an_argument_error(S):
    item = C.cell_answers()[1].item(3)
    n = Z.KZC_ITEMS_MAX + 1
    assert verify_raw(S.ctx, [item] * n, commitments=[item[0]], index=[0] * n)[0] == BLS_E_ARG
    assert verify_raw(S.ctx, [item] * 2, commitments=[item[0]], index=[0] * 2) == (1, [1, 1])  # the same form, accepted


# ---- the Python calls' chunking -------------------------------------------------------------------------------------
def test_list_calls_join_their_chunks_in_order(S, mods, monkeypatch):
    """ITEMS_MAX = 5 and BLOBS_MAX = 2 in place of 8,192 and 128: twelve cells and five blobs go through every
    list-taking call in three chunks; the outputs are the known answers in order, and a bad cell of the last chunk is
    named at its position in the whole list"""
    monkeypatch.setattr(mods.kc, "ITEMS_MAX", 5)
    monkeypatch.setattr(mods.kc, "BLOBS_MAX", 2)
    items = C.batch_items(12)
    assert S.verify_cell_kzg_proof_items(*unzip(items)) == [True] * 12
    for bad in (11, 10, 5):
        spoiled = items[:bad] + [off_by_one(items[bad], 40)] + items[bad + 1:]
        assert S.verify_cell_kzg_proof_items(*unzip(spoiled)) == [k != bad for k in range(12)], bad
    blobs = C.blobs()
    order = [0, 1, 2, 0, 2]  # chunks (random, zero), (degree 65, random), (degree 65)
    assert S.compute_cells_batch([blobs[b][1] for b in order]) == [blobs[b][3] for b in order]
    missing = set(C.missing_sets()["random_17"])
    idx = [k for k in range(128) if k not in missing]
    given = [[blobs[b][3][k] for k in idx] for b in order]
    assert S.recover_cells_batch(idx, given) == [blobs[b][3] for b in order]
