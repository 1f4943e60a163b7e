"""Fulu cell KZG on the device (``bls_kzg_cells_setup``, ``bls_kzg_verify_cells``, ``bls_kzg_compute_cells``,
``bls_kzg_recover_cells``, ``bls_kzg_cell_proofs_setup``, ``bls_kzg_compute_cells_and_proofs``,
``bls_kzg_recover_cells_and_proofs``; specs/fulu/polynomial-commitments-sampling.md).

``CellSetup`` puts what cell verification needs on the device -- ``[tau^k] G1`` for k < 64 as entries of the
context's resident G1 table, ``[tau^64] G2`` negated -- and carries ``verify_cell_kzg_proof_batch``, ``compute_cells``
and ``recover_cells`` with the spec's semantics: wrong lengths, non-canonical field elements, cell indices out of
range and invalid G1 bytes raise ``AssertionError``; everything else returns bool or bytes.  ``install_cells(spec,
cell_setup)`` puts them in place of a spec module's own (``uninstall_cells`` restores them).

The transforms (inverse 4,096 and forward / inverse 8,192 points over F_r, one inverse 64-point transform per
verified cell), the range checks, the batch's random linear combination and the group side run on the device.  The
batch check draws its own coefficients, so ``compute_verify_cell_kzg_proof_batch_challenge`` is neither provided nor
used.

``CellProofSetup`` names the 4,096 monomial points ``[tau^i] G1`` in the context's G1 table and carries
``compute_cells_and_kzg_proofs`` and ``recover_cells_and_kzg_proofs``: 63 rows per blob of the table MSM and one
128-point transform over G1 (``batch.g1_fft``).  A caller that holds only the Lagrange half of the trusted setup gets
the monomial points from ``g1_monomial_from_lagrange``.  ``install_cell_proofs(spec, proof_setup)`` puts the two
functions in place of a spec module's own; ``install_cells`` and ``PUBLIC`` are what they were.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native, batch, curve, kzg

BLS_MODULUS = kzg.BLS_MODULUS
FIELD_ELEMENTS_PER_CELL = 64
CELLS_PER_EXT_BLOB = 128
BYTES_PER_CELL = 32 * FIELD_ELEMENTS_PER_CELL
BYTES_PER_EXT_BLOB = CELLS_PER_EXT_BLOB * BYTES_PER_CELL
ITEMS_MAX = 8192  # cells per verification call (128 columns x 64 blobs)
BLOBS_MAX = 128   # blobs per cell-computation / recovery call

PROOF_BLOBS_PER_MSM = 8  # blobs whose 63 rows share one table MSM of the proofs (504 of its 511 rows)

PUBLIC = ("verify_cell_kzg_proof_batch", "compute_cells", "recover_cells")
PUBLIC_PROOFS = ("compute_cells_and_kzg_proofs", "recover_cells_and_kzg_proofs")
_SAVED = "_bls_mi355x_kzg_cells_saved"
_SAVED_PROOFS = "_bls_mi355x_kzg_cell_proofs_saved"


def _cell_bytes(cell) -> bytes:
    b = bytes(cell)
    assert len(b) == BYTES_PER_CELL
    return b


def _cell_index(i) -> int:
    i = int(i)
    assert 0 <= i < CELLS_PER_EXT_BLOB
    return i


def dedupe_commitments(commitments):
    """(the distinct commitments in order of first appearance, every item's index into them): the spec's
    deduplicated_commitments / commitment_indices"""
    index, distinct, idx = {}, [], []
    for c in commitments:
        if c not in index:
            index[c] = len(distinct)
            distinct.append(c)
        idx.append(index[c])
    return distinct, idx


def _recover_indices(cell_indices, n_cells: int) -> list:
    """recover_cells_and_kzg_proofs' assertions on the index list"""
    idx = [int(i) for i in cell_indices]
    assert len(idx) == n_cells
    assert CELLS_PER_EXT_BLOB // 2 <= len(idx) <= CELLS_PER_EXT_BLOB
    assert all(0 <= i < CELLS_PER_EXT_BLOB for i in idx)
    assert len(idx) == len(set(idx))
    assert idx == sorted(idx)
    return idx


def _split_cells(raw: bytes) -> list:
    return [raw[BYTES_PER_CELL * k: BYTES_PER_CELL * (k + 1)] for k in range(len(raw) // BYTES_PER_CELL)]


class CellSetup:
    """The cell functions on one context.  ``kzg_setup_or_ctx``: a ``kzg.KzgSetup`` (its context, and its G1 table
    when it has one), a ``_native.Context``, or None for the default context.  ``g1_monomial_64``:
    KZG_SETUP_G1_MONOMIAL[0..64) (longer lists are cut); ``g2_monomial_64``: KZG_SETUP_G2_MONOMIAL[64].  The 64
    points become entries of the context's current G1 table (found there, or appended), else of a table of their
    own (``self.table``), which replaces the context's."""

    def __init__(self, kzg_setup_or_ctx, g1_monomial_64, g2_monomial_64):
        table = None
        if isinstance(kzg_setup_or_ctx, kzg.KzgSetup):
            self.ctx = kzg_setup_or_ctx.ctx
            table = kzg_setup_or_ctx.table
        else:
            self.ctx = kzg_setup_or_ctx or _native.context()
        pts = [kzg._g1_bytes(p) for p in list(g1_monomial_64)[:FIELD_ELEMENTS_PER_CELL]]
        if len(pts) != FIELD_ELEMENTS_PER_CELL:
            raise ValueError("the cell setup takes the first 64 monomial G1 points")
        g2 = bytes(g2_monomial_64)
        if len(g2) != 96:
            raise ValueError("KZG_SETUP_G2_MONOMIAL[64] is 96 bytes")
        if table is None and curve._g1_table is not None and curve._g1_table.ctx is self.ctx:
            table = curve._g1_table
        if table is not None and table._current():
            idx = table.indices(pts)
            if idx is not None and bool((idx == idx[0] + np.arange(len(pts), dtype=np.uint32)).all()):
                first = int(idx[0])
            else:
                first = len(table)
                if not table.append(pts, subgroup_check=True).all():
                    raise ValueError("invalid point in the trusted setup")
        else:
            table = batch.G1Table(self.ctx)
            first = 0
            if not table.load(pts, subgroup_check=True).all():
                raise ValueError("invalid point in the trusted setup")
        self.table, self.first = table, first
        c = self.ctx
        if c.check(c.lib.bls_kzg_cells_setup(c.h, g2, first, FIELD_ELEMENTS_PER_CELL)) != 1:
            raise ValueError("invalid point in the trusted setup")

    # ---- verification ----------------------------------------------------------------------------------------
    def _assert_g1(self, points) -> None:
        """validate_kzg_g1 on every encoding: the identity, or a point of G1"""
        if not points:
            return
        c = self.ctx
        rc = c.check(c.lib.bls_point_decode(c.h, 1, b"".join(points), len(points), 1, None))
        assert rc == 1, "invalid G1 encoding"

    def verify_cell_kzg_proof_items(self, commitments, cell_indices, cells, proofs) -> list:
        """per-item verdicts of (C_k, cell index k, cell_k, pi_k): one batch check, and each item's own only when
        that fails"""
        cm, pf = [kzg._g1_bytes(x) for x in commitments], [kzg._g1_bytes(x) for x in proofs]
        ci = [_cell_index(i) for i in cell_indices]
        ce = [_cell_bytes(x) for x in cells]
        assert len(cm) == len(ci) == len(ce) == len(pf)
        for cell in ce:
            assert kzg.blob_is_canonical(cell), "cell element not below the modulus"
        out = []
        c = self.ctx
        for s in range(0, len(cm), ITEMS_MAX):
            n = len(cm[s: s + ITEMS_MAX])
            distinct, idx = dedupe_commitments(cm[s: s + n])
            a_idx = np.asarray(idx, dtype=np.uint32)
            a_cell = np.asarray(ci[s: s + n], dtype=np.uint32)
            item = np.zeros(n, dtype=np.uint8)
            rc = c.check(c.lib.bls_kzg_verify_cells(
                c.h, b"".join(distinct), len(distinct), a_idx.ctypes.data_as(ctypes.c_void_p),
                a_cell.ctypes.data_as(ctypes.c_void_p), b"".join(ce[s: s + n]), b"".join(pf[s: s + n]), n,
                item.ctypes.data_as(ctypes.c_void_p)))
            if rc != 1:
                self._assert_g1(distinct + pf[s: s + n])
            out += [bool(v) for v in item]
        return out

    def verify_cell_kzg_proof_batch(self, commitments_bytes, cell_indices, cells, proofs_bytes) -> bool:
        return all(self.verify_cell_kzg_proof_items(commitments_bytes, cell_indices, cells, proofs_bytes))

    # ---- cells and recovery (no setup needed on the device) --------------------------------------------------
    def compute_cells_batch(self, blobs) -> list:
        return compute_cells_batch(blobs, self.ctx)

    def compute_cells(self, blob) -> list:
        return compute_cells_batch([blob], self.ctx)[0]

    def recover_cells_batch(self, cell_indices, cells_per_blob) -> list:
        return recover_cells_batch(cell_indices, cells_per_blob, self.ctx)

    def recover_cells(self, cell_indices, cells) -> list:
        return recover_cells_batch(cell_indices, [cells], self.ctx)[0]


def compute_cells_batch(blobs, ctx: _native.Context | None = None) -> list:
    """[compute_cells(blob)] : 128 cells of 2,048 bytes per blob"""
    bl = [kzg._blob_bytes(b) for b in blobs]
    for b in bl:
        assert kzg.blob_is_canonical(b), "blob element not below the modulus"
    c = ctx or _native.context()
    out = []
    for s in range(0, len(bl), BLOBS_MAX):
        n = len(bl[s: s + BLOBS_MAX])
        o = ctypes.create_string_buffer(BYTES_PER_EXT_BLOB * n)
        rc = c.check(c.lib.bls_kzg_compute_cells(c.h, b"".join(bl[s: s + n]), n, o, None))
        assert rc == 1, "blob element not below the modulus"
        raw = o.raw
        out += [_split_cells(raw[BYTES_PER_EXT_BLOB * i: BYTES_PER_EXT_BLOB * (i + 1)]) for i in range(n)]
    return out


def compute_cells(blob, ctx: _native.Context | None = None) -> list:
    return compute_cells_batch([blob], ctx)[0]


def recover_cells_batch(cell_indices, cells_per_blob, ctx: _native.Context | None = None) -> list:
    """The 128 cells of every blob from the same >= 64 present cells of each (the column case): ``cell_indices``
    ascending, ``cells_per_blob[b][p]`` blob b's cell ``cell_indices[p]``."""
    per_blob = [[_cell_bytes(x) for x in cells] for cells in cells_per_blob]
    idx = None
    for cells in per_blob:
        idx = _recover_indices(cell_indices, len(cells))
        for cell in cells:
            assert kzg.blob_is_canonical(cell), "cell element not below the modulus"
    if idx is None:
        return []
    c = ctx or _native.context()
    a_idx = np.asarray(idx, dtype=np.uint32)
    out = []
    for s in range(0, len(per_blob), BLOBS_MAX):
        n = len(per_blob[s: s + BLOBS_MAX])
        o = ctypes.create_string_buffer(BYTES_PER_EXT_BLOB * n)
        rc = c.check(c.lib.bls_kzg_recover_cells(
            c.h, a_idx.ctypes.data_as(ctypes.c_void_p), len(idx), b"".join(b"".join(x) for x in per_blob[s: s + n]), n,
            o, None))
        assert rc == 1, "cell element not below the modulus"
        raw = o.raw
        out += [_split_cells(raw[BYTES_PER_EXT_BLOB * i: BYTES_PER_EXT_BLOB * (i + 1)]) for i in range(n)]
    return out


def recover_cells(cell_indices, cells, ctx: _native.Context | None = None) -> list:
    return recover_cells_batch(cell_indices, [cells], ctx)[0]


def g1_monomial_from_lagrange(g1_lagrange, ctx: _native.Context | None = None) -> list:
    """KZG_SETUP_G1_MONOMIAL from KZG_SETUP_G1_LAGRANGE (4,096 points in the setup file's order, as ``KzgSetup``
    takes them): the file's entry j is [L_j(tau)] with L_j the Lagrange basis at w^j (the spec bit-reverses the
    list where it pairs it with a blob), and X^k = sum_j w^(j k) L_j, so [tau^k] = sum_j w^(j k) LAGRANGE[j] -- the
    forward 4,096-point transform of the list as it stands, without 1 / n: one ``bls_g1_fft`` call."""
    pts = [kzg._g1_bytes(p) for p in g1_lagrange]
    if len(pts) != kzg.FIELD_ELEMENTS_PER_BLOB:
        raise ValueError("the Lagrange setup has 4,096 G1 points")
    try:
        return batch.g1_fft(pts, ctx=ctx)
    except ValueError:
        raise ValueError("invalid point in the trusted setup") from None


def _split_proofs(raw: bytes) -> list:
    return [raw[48 * k: 48 * (k + 1)] for k in range(len(raw) // 48)]


class CellProofSetup:
    """The cell proof functions on one context.  ``cell_setup_or_ctx``: a ``CellSetup`` or ``kzg.KzgSetup`` (its
    context, and its G1 table when it has one), a ``_native.Context``, or None for the default context.  Exactly
    one of ``g1_monomial`` (KZG_SETUP_G1_MONOMIAL, 4,096 points) and ``g1_lagrange`` (KZG_SETUP_G1_LAGRANGE, 4,096
    points, from which ``g1_monomial_from_lagrange`` derives the former).  The 4,096 points become entries of the
    context's current G1 table -- found there as a consecutive run, or appended, which keeps a ``KzgSetup`` or
    ``CellSetup`` on that table valid -- else of a table of their own (``self.table``), which replaces the
    context's.  ``self.g1_monomial`` keeps the 4,096 encodings (the derived ones with ``g1_lagrange``)."""

    def __init__(self, cell_setup_or_ctx, g1_monomial=None, g1_lagrange=None):
        if (g1_monomial is None) == (g1_lagrange is None):
            raise ValueError("give exactly one of g1_monomial and g1_lagrange")
        given = list(g1_monomial if g1_monomial is not None else g1_lagrange)
        if len(given) != kzg.FIELD_ELEMENTS_PER_BLOB:
            raise ValueError("the cell proof setup takes 4,096 G1 points")
        given = [kzg._g1_bytes(p) for p in given]
        table = None
        if isinstance(cell_setup_or_ctx, (CellSetup, kzg.KzgSetup)):
            self.ctx = cell_setup_or_ctx.ctx
            table = cell_setup_or_ctx.table
        else:
            self.ctx = cell_setup_or_ctx or _native.context()
        pts = given if g1_monomial is not None else g1_monomial_from_lagrange(given, self.ctx)
        if table is None and curve._g1_table is not None and curve._g1_table.ctx is self.ctx:
            table = curve._g1_table
        if table is not None and table._current():
            first = table.run_of(pts)
            if first is None:
                first = len(table)
                if not table.append(pts, subgroup_check=True).all():
                    raise ValueError("invalid point in the trusted setup")
        else:
            table = batch.G1Table(self.ctx)
            first = 0
            if not table.load(pts, subgroup_check=True).all():
                raise ValueError("invalid point in the trusted setup")
        self.table, self.first, self.g1_monomial = table, first, pts
        self.setup()

    def setup(self) -> None:
        """(again) name the table's entries to the library: after another object replaced and reloaded the table"""
        c = self.ctx
        if c.check(c.lib.bls_kzg_cell_proofs_setup(c.h, self.first, kzg.FIELD_ELEMENTS_PER_BLOB)) != 1:
            raise ValueError("invalid point in the trusted setup")

    def compute_cells_and_kzg_proofs_batch(self, blobs) -> list:
        """[(cells, proofs)] per blob: 128 cells of 2,048 bytes and 128 proofs of 48 bytes"""
        bl = [kzg._blob_bytes(b) for b in blobs]
        for b in bl:
            assert kzg.blob_is_canonical(b), "blob element not below the modulus"
        c = self.ctx
        out = []
        for s in range(0, len(bl), BLOBS_MAX):
            n = len(bl[s: s + BLOBS_MAX])
            o = ctypes.create_string_buffer(BYTES_PER_EXT_BLOB * n)
            pf = ctypes.create_string_buffer(48 * CELLS_PER_EXT_BLOB * n)
            rc = c.check(c.lib.bls_kzg_compute_cells_and_proofs(c.h, b"".join(bl[s: s + n]), n, o, pf, None))
            assert rc == 1, "blob element not below the modulus"
            out += _cells_and_proofs(o.raw, pf.raw, n)
        return out

    def compute_cells_and_kzg_proofs(self, blob) -> tuple:
        return self.compute_cells_and_kzg_proofs_batch([blob])[0]

    def recover_cells_and_kzg_proofs_batch(self, cell_indices, cells_per_blob) -> list:
        """[(cells, proofs)] of every blob from the same >= 64 present cells of each, as ``recover_cells_batch``
        takes them"""
        per_blob = [[_cell_bytes(x) for x in cells] for cells in cells_per_blob]
        idx = None
        for cells in per_blob:
            idx = _recover_indices(cell_indices, len(cells))
            for cell in cells:
                assert kzg.blob_is_canonical(cell), "cell element not below the modulus"
        if idx is None:
            return []
        c = self.ctx
        a_idx = np.asarray(idx, dtype=np.uint32)
        out = []
        for s in range(0, len(per_blob), BLOBS_MAX):
            n = len(per_blob[s: s + BLOBS_MAX])
            o = ctypes.create_string_buffer(BYTES_PER_EXT_BLOB * n)
            pf = ctypes.create_string_buffer(48 * CELLS_PER_EXT_BLOB * n)
            rc = c.check(c.lib.bls_kzg_recover_cells_and_proofs(
                c.h, a_idx.ctypes.data_as(ctypes.c_void_p), len(idx),
                b"".join(b"".join(x) for x in per_blob[s: s + n]), n, o, pf, None))
            assert rc == 1, "cell element not below the modulus"
            out += _cells_and_proofs(o.raw, pf.raw, n)
        return out

    def recover_cells_and_kzg_proofs(self, cell_indices, cells) -> tuple:
        return self.recover_cells_and_kzg_proofs_batch(cell_indices, [cells])[0]


def _cells_and_proofs(cells_raw: bytes, proofs_raw: bytes, n: int) -> list:
    pb = 48 * CELLS_PER_EXT_BLOB
    return [(_split_cells(cells_raw[BYTES_PER_EXT_BLOB * i: BYTES_PER_EXT_BLOB * (i + 1)]),
             _split_proofs(proofs_raw[pb * i: pb * (i + 1)])) for i in range(n)]


def _check_sizes(spec) -> None:
    if (int(getattr(spec, "FIELD_ELEMENTS_PER_CELL", 0)) != FIELD_ELEMENTS_PER_CELL
            or int(getattr(spec, "CELLS_PER_EXT_BLOB", 0)) != CELLS_PER_EXT_BLOB):
        raise ValueError("the device cell functions are built for FIELD_ELEMENTS_PER_CELL = 64 and "
                         "CELLS_PER_EXT_BLOB = 128")


def install_cell_proofs(spec, proof_setup: CellProofSetup) -> None:
    """Replace ``compute_cells_and_kzg_proofs`` and ``recover_cells_and_kzg_proofs`` of a spec module object (the
    sizes ``install_cells`` takes; any other is refused) with ``proof_setup``'s, each only where the module has that
    name; cells and proofs come back as the module's own ``Cell`` and ``KZGProof`` types where it defines them."""
    _check_sizes(spec)
    if hasattr(spec, _SAVED_PROOFS):
        uninstall_cell_proofs(spec)

    def typed(result):
        cells, proofs = result
        return ([kzg._typed(spec, "Cell", x) for x in cells], [kzg._typed(spec, "KZGProof", x) for x in proofs])

    new = {
        "compute_cells_and_kzg_proofs": lambda blob: typed(proof_setup.compute_cells_and_kzg_proofs(blob)),
        "recover_cells_and_kzg_proofs": lambda cell_indices, cells: typed(
            proof_setup.recover_cells_and_kzg_proofs(cell_indices, cells)),
    }
    assert tuple(new) == PUBLIC_PROOFS
    new = {name: fn for name, fn in new.items() if hasattr(spec, name)}
    setattr(spec, _SAVED_PROOFS, {name: getattr(spec, name) for name in new})
    for name, fn in new.items():
        setattr(spec, name, fn)


def uninstall_cell_proofs(spec) -> None:
    """Put back what ``install_cell_proofs`` replaced."""
    saved = getattr(spec, _SAVED_PROOFS, None)
    if saved is None:
        return
    for name, old in saved.items():
        setattr(spec, name, old)
    delattr(spec, _SAVED_PROOFS)


def install_cells(spec, cell_setup: CellSetup) -> None:
    """Replace the cell functions of a spec module object (``FIELD_ELEMENTS_PER_CELL`` = 64 and
    ``CELLS_PER_EXT_BLOB`` = 128; any other size is refused) with ``cell_setup``'s; cells come back as the module's
    own ``Cell`` type where it defines one.  ``compute_cells`` is installed only where the module has that name
    (older texts have only the ``_and_kzg_proofs`` forms, which are left alone)."""
    if (int(getattr(spec, "FIELD_ELEMENTS_PER_CELL", 0)) != FIELD_ELEMENTS_PER_CELL
            or int(getattr(spec, "CELLS_PER_EXT_BLOB", 0)) != CELLS_PER_EXT_BLOB):
        raise ValueError("the device cell functions are built for FIELD_ELEMENTS_PER_CELL = 64 and "
                         "CELLS_PER_EXT_BLOB = 128")
    if hasattr(spec, _SAVED):
        uninstall_cells(spec)
    new = {
        "verify_cell_kzg_proof_batch": cell_setup.verify_cell_kzg_proof_batch,
        "compute_cells": lambda blob: [kzg._typed(spec, "Cell", x) for x in cell_setup.compute_cells(blob)],
        "recover_cells": lambda cell_indices, cells: [
            kzg._typed(spec, "Cell", x) for x in cell_setup.recover_cells(cell_indices, cells)],
    }
    assert tuple(new) == PUBLIC
    if not hasattr(spec, "compute_cells"):
        del new["compute_cells"]
    missing = object()
    setattr(spec, _SAVED, {name: getattr(spec, name, missing) for name in new} | {"": missing})
    for name, fn in new.items():
        setattr(spec, name, fn)


def uninstall_cells(spec) -> None:
    """Put back what ``install_cells`` replaced (attributes the module did not have are removed)."""
    saved = getattr(spec, _SAVED, None)
    if saved is None:
        return
    missing = saved[""]
    for name, old in saved.items():
        if not name:
            continue
        if old is missing:
            if hasattr(spec, name):
                delattr(spec, name)
        else:
            setattr(spec, name, old)
    delattr(spec, _SAVED)
