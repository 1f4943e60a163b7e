"""Deneb blob KZG on the device (``bls_kzg_*``; specs/deneb/polynomial-commitments.md).

``KzgSetup`` puts the trusted setup on the device -- the bit-reversal-permuted Lagrange points as 4,096 entries of
the context's resident G1 table (``batch.G1Table``), ``[tau] G2`` negated -- and carries the spec's public blob
functions with the spec's semantics: wrong lengths, non-canonical field elements and invalid G1 bytes raise
``AssertionError``; everything else returns bool or bytes.  ``install(spec, setup)`` puts them in place of a spec
module's own (``uninstall`` restores them).

The scalar-field work (range checks, barycentric evaluation, quotients, the batch's random linear combination) and
the group side run on the device.  The Fiat-Shamir challenge is computed here: it is one SHA-256 over a sequential
transcript of 131,152 bytes, which hashlib does in about 0.1 ms.
"""
from __future__ import annotations

import ctypes
import hashlib

import numpy as np

from . import _native, batch, curve

BLS_MODULUS = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
FIELD_ELEMENTS_PER_BLOB = 4096
BYTES_PER_FIELD_ELEMENT = 32
BYTES_PER_BLOB = FIELD_ELEMENTS_PER_BLOB * BYTES_PER_FIELD_ELEMENT
FIAT_SHAMIR_PROTOCOL_DOMAIN = b"FSBLOBVERIFY_V1_"
MSM_ROWS_MAX = 511  # blobs per commitment / proof call (bls_g1_table_msm's bound)
BLOBS_MAX = 1024    # blobs per evaluation / blob-verification call
ITEMS_MAX = 65536   # items per verification call

PUBLIC = (
    "blob_to_kzg_commitment", "compute_kzg_proof", "compute_blob_kzg_proof", "verify_kzg_proof",
    "verify_kzg_proof_batch", "verify_blob_kzg_proof", "verify_blob_kzg_proof_batch",
    "evaluate_polynomial_in_evaluation_form", "compute_challenge",
)
_SAVED = "_bls_mi355x_kzg_saved"


def bit_reversal_permutation(seq):
    """seq[brp(i)] for i < len(seq), a power of two (the spec's order of the domain and of the Lagrange setup)"""
    n = len(seq)
    bits = n.bit_length() - 1
    assert n == 1 << bits
    return [seq[int(format(i, "0%db" % bits)[::-1], 2)] if bits else seq[i] for i in range(n)]


def compute_challenge(blob, commitment) -> int:
    """The blob functions' Fiat-Shamir challenge: SHA-256 over the protocol domain, 4,096 as 16 big-endian bytes,
    the blob and the commitment, as a big-endian integer mod r."""
    blob, commitment = bytes(blob), bytes(commitment)
    assert len(blob) == BYTES_PER_BLOB and len(commitment) == 48
    h = hashlib.sha256(FIAT_SHAMIR_PROTOCOL_DOMAIN)
    h.update(FIELD_ELEMENTS_PER_BLOB.to_bytes(16, "big"))
    h.update(blob)
    h.update(commitment)
    return int.from_bytes(h.digest(), "big") % BLS_MODULUS


def _field_bytes(x) -> bytes:
    """a field element given as 32 bytes or as an integer; asserts it is canonical"""
    if isinstance(x, (bytes, bytearray, memoryview)):
        b = bytes(x)
        assert len(b) == BYTES_PER_FIELD_ELEMENT
        assert int.from_bytes(b, "big") < BLS_MODULUS
        return b
    v = int(x)
    assert 0 <= v < BLS_MODULUS
    return v.to_bytes(32, "big")


def _blob_bytes(blob) -> bytes:
    b = bytes(blob)
    assert len(b) == BYTES_PER_BLOB
    return b


def _g1_bytes(p) -> bytes:
    b = bytes(p)
    assert len(b) == 48
    return b


def blob_is_canonical(blob: bytes) -> bool:
    a = np.frombuffer(blob, dtype=">u8").reshape(-1, 4)
    m = [(BLS_MODULUS >> (64 * (3 - k))) & (2 ** 64 - 1) for k in range(4)]
    lt = np.zeros(a.shape[0], dtype=bool)
    eq = np.ones(a.shape[0], dtype=bool)
    for k in range(4):
        lt |= eq & (a[:, k] < m[k])
        eq &= a[:, k] == m[k]
    return bool(lt.all())


class KzgSetup:
    """The trusted setup on one context.  ``g1_lagrange``: the 4,096 KZG_SETUP_G1_LAGRANGE encodings in the setup
    file's order; ``g2_monomial_1``: KZG_SETUP_G2_MONOMIAL[1].  The permuted Lagrange points become entries of the
    table set with ``curve.use_g1_table`` when there is one on this context (found there, or appended), else of a
    table of their own (``self.table``), which replaces the context's."""

    def __init__(self, g1_lagrange, g2_monomial_1, ctx: _native.Context | None = None):
        self.ctx = ctx or _native.context()
        pts = [_g1_bytes(p) for p in g1_lagrange]
        if len(pts) != FIELD_ELEMENTS_PER_BLOB:
            raise ValueError("the Lagrange setup has 4,096 points")
        pts = bit_reversal_permutation(pts)
        table = curve._g1_table
        first = None
        if table is not None and table.ctx is self.ctx and table._current():
            idx = table.indices(pts)
            if idx is not None and bool((idx == idx[0] + np.arange(len(pts), dtype=np.uint32)).all()):
                first = int(idx[0])
            else:
                first = len(table)
                ok = table.append(pts, subgroup_check=True)
                if not ok.all():
                    raise ValueError("invalid point in the trusted setup")
        else:
            table = batch.G1Table(self.ctx)
            first = 0
            if not table.load(pts, subgroup_check=True).all():
                raise ValueError("invalid point in the trusted setup")
        self.table, self.first = table, first
        self._setup(g2_monomial_1, first, FIELD_ELEMENTS_PER_BLOB)

    @classmethod
    def verify_only(cls, g2_monomial_1, ctx: _native.Context | None = None) -> "KzgSetup":
        """A setup that verifies and evaluates; commitments and proofs need the Lagrange points."""
        self = cls.__new__(cls)
        self.ctx = ctx or _native.context()
        self.table, self.first = None, None
        self._setup(g2_monomial_1, 0, 0)
        return self

    def _setup(self, g2_monomial_1, first: int, n: int) -> None:
        g2 = bytes(g2_monomial_1)
        if len(g2) != 96:
            raise ValueError("KZG_SETUP_G2_MONOMIAL[1] is 96 bytes")
        c = self.ctx
        if c.check(c.lib.bls_kzg_setup(c.h, g2, first, n)) != 1:
            raise ValueError("invalid point in the trusted setup")

    # ---- the list-taking calls -------------------------------------------------------------------------------
    def evaluate_blobs(self, blobs, zs) -> list:
        """[p_b(z_b)] as 32-byte elements, for blobs as bytes and z as bytes or ints"""
        bl = [_blob_bytes(b) for b in blobs]
        z = [_field_bytes(x) for x in zs]
        assert len(bl) == len(z)
        out = []
        c = self.ctx
        for s in range(0, len(bl), BLOBS_MAX):
            n = len(bl[s: s + BLOBS_MAX])
            y = ctypes.create_string_buffer(32 * n)
            rc = c.check(c.lib.bls_kzg_eval_blobs(c.h, b"".join(bl[s: s + n]), n, b"".join(z[s: s + n]), y, None))
            assert rc == 1, "blob element not below the modulus"
            out += [y.raw[32 * i: 32 * i + 32] for i in range(n)]
        return out

    def blob_to_kzg_commitments(self, blobs) -> list:
        bl = [_blob_bytes(b) for b in blobs]
        out = []
        c = self.ctx
        for s in range(0, len(bl), MSM_ROWS_MAX):
            n = len(bl[s: s + MSM_ROWS_MAX])
            o = ctypes.create_string_buffer(48 * n)
            rc = c.check(c.lib.bls_kzg_blob_commitments(c.h, b"".join(bl[s: s + n]), n, o, None))
            assert rc == 1, "blob element not below the modulus"
            out += [o.raw[48 * i: 48 * i + 48] for i in range(n)]
        return out

    def compute_kzg_proofs(self, blobs, zs) -> list:
        """[(proof_b, y_b)] for the quotients of p_b by (X - z_b)"""
        bl = [_blob_bytes(b) for b in blobs]
        z = [_field_bytes(x) for x in zs]
        assert len(bl) == len(z)
        out = []
        c = self.ctx
        for s in range(0, len(bl), MSM_ROWS_MAX):
            n = len(bl[s: s + MSM_ROWS_MAX])
            p, y = ctypes.create_string_buffer(48 * n), ctypes.create_string_buffer(32 * n)
            rc = c.check(c.lib.bls_kzg_compute_proofs(c.h, b"".join(bl[s: s + n]), n, b"".join(z[s: s + n]), p, y,
                                                      None))
            assert rc == 1, "blob element not below the modulus"
            out += [(p.raw[48 * i: 48 * i + 48], y.raw[32 * i: 32 * i + 32]) for i in range(n)]
        return out

    def compute_blob_kzg_proofs(self, blobs, commitments) -> list:
        cm = [_g1_bytes(x) for x in commitments]
        bl = [_blob_bytes(b) for b in blobs]
        assert len(bl) == len(cm)
        self._assert_g1(cm)
        return [p for p, _ in self.compute_kzg_proofs(bl, [compute_challenge(b, k) for b, k in zip(bl, cm)])]

    def _assert_g1(self, points) -> None:
        """validate_kzg_g1 on every encoding: the identity, or a point of G1"""
        if not points:
            return
        c = self.ctx
        rc = c.check(c.lib.bls_point_decode(c.h, 1, b"".join(points), len(points), 1, None))
        assert rc == 1, "invalid G1 encoding"

    def verify_kzg_proof_items(self, commitments, zs, ys, proofs) -> list:
        """per-item verdicts of (C_i, z_i, y_i, pi_i): one batch check, and each item's own only when that fails"""
        cm, pf = [_g1_bytes(x) for x in commitments], [_g1_bytes(x) for x in proofs]
        z, y = [_field_bytes(x) for x in zs], [_field_bytes(x) for x in ys]
        assert len(cm) == len(z) == len(y) == len(pf)
        out = []
        c = self.ctx
        for s in range(0, len(cm), ITEMS_MAX):
            n = len(cm[s: s + ITEMS_MAX])
            item = np.zeros(n, dtype=np.uint8)
            rc = c.check(c.lib.bls_kzg_verify_batch(c.h, b"".join(cm[s: s + n]), b"".join(z[s: s + n]),
                                                    b"".join(y[s: s + n]), b"".join(pf[s: s + n]), n,
                                                    item.ctypes.data_as(ctypes.c_void_p)))
            if rc != 1:
                self._assert_g1(cm[s: s + n] + pf[s: s + n])
            out += [bool(v) for v in item]
        return out

    def verify_blob_kzg_proof_items(self, blobs, commitments, proofs) -> list:
        """per-item verdicts of verify_blob_kzg_proof_batch's items"""
        bl = [_blob_bytes(b) for b in blobs]
        cm, pf = [_g1_bytes(x) for x in commitments], [_g1_bytes(x) for x in proofs]
        assert len(bl) == len(cm) == len(pf)
        z = [compute_challenge(b, k).to_bytes(32, "big") for b, k in zip(bl, cm)]
        out = []
        c = self.ctx
        for s in range(0, len(bl), BLOBS_MAX):
            n = len(bl[s: s + BLOBS_MAX])
            item = np.zeros(n, dtype=np.uint8)
            rc = c.check(c.lib.bls_kzg_verify_blob_batch(c.h, b"".join(bl[s: s + n]), b"".join(cm[s: s + n]),
                                                         b"".join(pf[s: s + n]), b"".join(z[s: s + n]), n,
                                                         item.ctypes.data_as(ctypes.c_void_p)))
            if rc != 1:
                assert all(blob_is_canonical(b) for b in bl[s: s + n]), "blob element not below the modulus"
                self._assert_g1(cm[s: s + n] + pf[s: s + n])
            out += [bool(v) for v in item]
        return out

    # ---- the spec's public methods ---------------------------------------------------------------------------
    def blob_to_kzg_commitment(self, blob) -> bytes:
        return self.blob_to_kzg_commitments([blob])[0]

    def compute_kzg_proof(self, blob, z_bytes) -> tuple:
        assert len(bytes(z_bytes)) == BYTES_PER_FIELD_ELEMENT
        return self.compute_kzg_proofs([blob], [bytes(z_bytes)])[0]

    def compute_blob_kzg_proof(self, blob, commitment_bytes) -> bytes:
        return self.compute_blob_kzg_proofs([blob], [commitment_bytes])[0]

    def verify_kzg_proof(self, commitment_bytes, z_bytes, y_bytes, proof_bytes) -> bool:
        assert len(bytes(z_bytes)) == len(bytes(y_bytes)) == BYTES_PER_FIELD_ELEMENT
        return self.verify_kzg_proof_items([commitment_bytes], [bytes(z_bytes)], [bytes(y_bytes)], [proof_bytes])[0]

    def verify_kzg_proof_batch(self, commitments, zs, ys, proofs) -> bool:
        return all(self.verify_kzg_proof_items(commitments, zs, ys, proofs))

    def verify_blob_kzg_proof(self, blob, commitment_bytes, proof_bytes) -> bool:
        return self.verify_blob_kzg_proof_items([blob], [commitment_bytes], [proof_bytes])[0]

    def verify_blob_kzg_proof_batch(self, blobs, commitments_bytes, proofs_bytes) -> bool:
        return all(self.verify_blob_kzg_proof_items(blobs, commitments_bytes, proofs_bytes))

    def evaluate_polynomial_in_evaluation_form(self, polynomial, z) -> int:
        """p(z) for a polynomial given as its 4,096 evaluations (integers below the modulus, or a blob's bytes)"""
        if isinstance(polynomial, (bytes, bytearray, memoryview)):
            blob = _blob_bytes(polynomial)
        else:
            assert len(polynomial) == FIELD_ELEMENTS_PER_BLOB
            blob = b"".join(_field_bytes(int(v)) for v in polynomial)
        return int.from_bytes(self.evaluate_blobs([blob], [z])[0], "big")

    compute_challenge = staticmethod(compute_challenge)


def _typed(spec, name: str, value):
    """value as the spec module's own type of that name, where it has one"""
    t = getattr(spec, name, None)
    return t(value) if callable(t) else value


def install(spec, setup: KzgSetup) -> None:
    """Replace the blob functions of a spec module object (``FIELD_ELEMENTS_PER_BLOB`` = 4,096; any other size is
    refused) with ``setup``'s; results are wrapped in the module's own KZGCommitment / KZGProof / Bytes32 /
    BLSFieldElement types where it defines them."""
    if int(getattr(spec, "FIELD_ELEMENTS_PER_BLOB", 0)) != FIELD_ELEMENTS_PER_BLOB:
        raise ValueError("the device KZG functions are built for FIELD_ELEMENTS_PER_BLOB = 4096")
    if hasattr(spec, _SAVED):
        uninstall(spec)

    def proof_and_y(blob, z_bytes):
        p, y = setup.compute_kzg_proof(blob, z_bytes)
        return _typed(spec, "KZGProof", p), _typed(spec, "Bytes32", y)

    new = {
        "blob_to_kzg_commitment": lambda blob: _typed(spec, "KZGCommitment", setup.blob_to_kzg_commitment(blob)),
        "compute_kzg_proof": proof_and_y,
        "compute_blob_kzg_proof": lambda blob, commitment_bytes: _typed(
            spec, "KZGProof", setup.compute_blob_kzg_proof(blob, commitment_bytes)),
        "verify_kzg_proof": setup.verify_kzg_proof,
        "verify_kzg_proof_batch": setup.verify_kzg_proof_batch,
        "verify_blob_kzg_proof": setup.verify_blob_kzg_proof,
        "verify_blob_kzg_proof_batch": setup.verify_blob_kzg_proof_batch,
        "evaluate_polynomial_in_evaluation_form": lambda polynomial, z: _typed(
            spec, "BLSFieldElement", setup.evaluate_polynomial_in_evaluation_form(polynomial, z)),
        "compute_challenge": lambda blob, commitment: _typed(
            spec, "BLSFieldElement", compute_challenge(blob, commitment)),
    }
    assert tuple(new) == PUBLIC
    missing = object()
    setattr(spec, _SAVED, {name: getattr(spec, name, missing) for name in PUBLIC} | {"": missing})
    for name, fn in new.items():
        setattr(spec, name, fn)


def uninstall(spec) -> None:
    """Put back what ``install`` replaced (attributes the module did not have are removed)."""
    saved = getattr(spec, _SAVED, None)
    if saved is None:
        return
    missing = saved[""]
    for name in PUBLIC:
        if saved[name] is missing:
            if hasattr(spec, name):
                delattr(spec, name)
        else:
            setattr(spec, name, saved[name])
    delattr(spec, _SAVED)
