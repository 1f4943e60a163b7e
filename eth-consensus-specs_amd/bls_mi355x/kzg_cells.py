"""Fulu cell KZG on the device (``bls_kzg_cells_setup``, ``bls_kzg_verify_cells``, ``bls_kzg_compute_cells``,
``bls_kzg_recover_cells``; specs/fulu/polynomial-commitments-sampling.md).

``CellSetup`` puts what cell verification needs on the device -- ``[tau^k] G1`` for k < 64 as entries of the
context's resident G1 table, ``[tau^64] G2`` negated -- and carries ``verify_cell_kzg_proof_batch``, ``compute_cells``
and ``recover_cells`` with the spec's semantics: wrong lengths, non-canonical field elements, cell indices out of
range and invalid G1 bytes raise ``AssertionError``; everything else returns bool or bytes.  ``install_cells(spec,
cell_setup)`` puts them in place of a spec module's own (``uninstall_cells`` restores them).

The transforms (inverse 4,096 and forward / inverse 8,192 points over F_r, one inverse 64-point transform per
verified cell), the range checks, the batch's random linear combination and the group side run on the device.  The
cell proofs (``compute_cells_and_kzg_proofs`` and the proofs of ``recover_cells_and_kzg_proofs``) are not computed
here; the batch check draws its own coefficients, so ``compute_verify_cell_kzg_proof_batch_challenge`` is neither
provided nor used.
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

PUBLIC = ("verify_cell_kzg_proof_batch", "compute_cells", "recover_cells")
_SAVED = "_bls_mi355x_kzg_cells_saved"


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
