"""Batch / registry API (the throughput path).

The per-call drop-in API (``backend.mi355x_bls``) verifies one signature per
ctypes call.  Spec call sites that verify many aggregates against the
validator registry (``is_valid_indexed_attestation``,
specs/phase0/beacon-chain.md:776-790; ``process_sync_aggregate``,
specs/altair/beacon-chain.md:575-610) use these instead: the registry's
pubkeys are decoded and KeyValidated once into HBM and each aggregate is
named by registry indices.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from . import _native

# per-context job slots with streams: BLS_FAV_JOBS_INIT (default 10: two streams per job, the batch checks on the
# jobs' own streams, 21 of the 24 hardware queues -- profiles/r05h_jobs_streams_ab.txt: C2 +3 %, C3 +13 % over 7
# three-stream jobs with one shared FE stream; 11 jobs and more, or more streams than queues, collapse) of the
# BLS_FAV_JOBS = 16 in include/blsmi355x.h, read by the library at bls_ctx_create
FAV_JOBS = max(1, min(16, int(os.environ.get("BLS_FAV_JOBS_INIT", "10"))))
# batches kept in flight by run_pipelined (<= FAV_JOBS)
FAV_DEPTH = max(1, min(FAV_JOBS, int(os.environ.get("BLS_FAV_DEPTH", str(FAV_JOBS)))))
R_ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001  # the BLS12-381 group order r


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(ctypes.c_void_p)


def _u8(b) -> np.ndarray:
    return np.frombuffer(bytes(b), dtype=np.uint8) if not isinstance(b, np.ndarray) else np.ascontiguousarray(b, np.uint8)


class Registry:
    """HBM-resident affine pubkey table of one context.

    The host keeps a pubkey-bytes -> index map for the keys loaded or appended through this object.  It is
    tied to the library's registry generation (``bls_registry_generation``, bumped whenever any caller
    replaces the device table): after a replacement by another object or by ``generate()``, lookups return
    None instead of indices that now name other keys."""

    def __init__(self, ctx: _native.Context | None = None):
        self.ctx = ctx or _native.context()
        self._index: dict[bytes, int] = {}  # pubkey bytes -> first registry index (host-side lookup)
        self._gen = None  # library registry generation the map belongs to

    def _generation(self) -> int:
        return int(self.ctx.lib.bls_registry_generation(self.ctx.h))

    def _remember(self, buf: np.ndarray, first: int) -> None:
        raw = buf.tobytes()
        for i in range(len(raw) // 48):
            self._index.setdefault(raw[48 * i: 48 * i + 48], first + i)

    def load(self, pubkeys48: bytes | np.ndarray) -> np.ndarray:
        """Decode + KeyValidate ``n`` compressed keys; returns the validity mask."""
        buf = _u8(pubkeys48)
        if buf.size % 48:
            raise ValueError("pubkeys must be a multiple of 48 bytes")
        n = buf.size // 48
        valid = np.zeros(n, dtype=np.uint8)
        c = self.ctx
        self._index, self._gen = {}, None
        c.check(c.lib.bls_registry_load(c.h, buf.tobytes(), n, _ptr(valid)))
        self._remember(buf, 0)
        self._gen = self._generation()
        return valid

    def append(self, pubkeys48: bytes | np.ndarray) -> np.ndarray:
        """Deposits: append keys as validator indices len(self) .. (decode + KeyValidate on the
        device, existing indices unchanged; specs/phase0/beacon-chain.md:2037-2062).  Returns the
        validity mask of the new keys."""
        buf = _u8(pubkeys48)
        if buf.size % 48:
            raise ValueError("pubkeys must be a multiple of 48 bytes")
        n = buf.size // 48
        first = len(self)
        valid = np.zeros(n, dtype=np.uint8)
        c = self.ctx
        c.check(c.lib.bls_registry_append(c.h, buf.tobytes(), n, _ptr(valid)))
        if self._gen is not None and self._gen == self._generation():
            self._remember(buf, first)
        return valid

    def _current(self) -> bool:
        return self._gen is not None and self._gen == self._generation()

    def index_of(self, pubkey48: bytes) -> int | None:
        """Registry index of a compressed pubkey loaded or appended through this object, else None (also
        None once the device table was replaced)."""
        if not self._current():
            return None
        return self._index.get(bytes(pubkey48))

    def indices(self, pubkeys) -> np.ndarray | None:
        """u32 registry indices of every key, or None if any key is not resident (or the map is stale)."""
        if not self._current():
            return None
        out = np.empty(len(pubkeys), dtype=np.uint32)
        for i, pk in enumerate(pubkeys):
            k = self._index.get(bytes(pk))
            if k is None:
                return None
            out[i] = k
        return out

    def generate(self, n: int, first_sk: int = 1, want_bytes: bool = False):
        """Synthetic registry pk_i = (first_sk + i)*G1 built on the device (benchmarks).  With want_bytes the
        compressed keys are returned and the pubkey -> index map covers them."""
        c = self.ctx
        out = ctypes.create_string_buffer(48 * n) if want_bytes else None
        self._index, self._gen = {}, None
        c.check(c.lib.bls_registry_generate(c.h, first_sk, n, out))
        if want_bytes:
            self._remember(np.frombuffer(out.raw, dtype=np.uint8), 0)
            self._gen = self._generation()
            return out.raw
        return None

    def __len__(self):
        return int(self.ctx.lib.bls_registry_size(self.ctx.h))


def offsets_from_lengths(lengths) -> np.ndarray:
    offs = np.zeros(len(lengths) + 1, dtype=np.uint64)
    np.cumsum(np.asarray(lengths, dtype=np.uint64), out=offs[1:])
    return offs


def fast_aggregate_verify_batch(indices: np.ndarray, offsets: np.ndarray, msgs32, sigs96, ctx=None) -> np.ndarray:
    """B FastAggregateVerify calls over registry indices -> bool array."""
    c = ctx or _native.context()
    idx = np.ascontiguousarray(indices, dtype=np.uint32)
    offs = np.ascontiguousarray(offsets, dtype=np.uint64)
    B = offs.size - 1
    m, s = _u8(msgs32), _u8(sigs96)
    if m.size != 32 * B or s.size != 96 * B:
        raise ValueError("need 32-byte messages and 96-byte signatures, one per aggregate")
    out = np.zeros(B, dtype=np.uint8)
    c.check(c.lib.bls_fav_batch_indexed(c.h, _ptr(idx), _ptr(offs), B, m.tobytes(), s.tobytes(), _ptr(out)))
    return out.astype(bool)


def verify_batch(indices: np.ndarray, msgs32, sigs96, ctx=None) -> np.ndarray:
    """B Verify calls with registry-resident pubkeys -> bool array."""
    c = ctx or _native.context()
    idx = np.ascontiguousarray(indices, dtype=np.uint32)
    B = idx.size
    m, s = _u8(msgs32), _u8(sigs96)
    if m.size != 32 * B or s.size != 96 * B:
        raise ValueError("need 32-byte messages and 96-byte signatures")
    out = np.zeros(B, dtype=np.uint8)
    c.check(c.lib.bls_verify_batch_indexed(c.h, _ptr(idx), B, m.tobytes(), s.tobytes(), _ptr(out)))
    return out.astype(bool)


def group_messages(msgs32) -> tuple[bytes, np.ndarray]:
    """Deduplicate B 32-byte messages on the host: (table, msg_ids) with the distinct messages in order of first
    occurrence and msg_ids[b] (uint32) the table entry of message b, so that
    table[32 * msg_ids[b]: 32 * msg_ids[b] + 32] == msgs32[32 * b: 32 * b + 32]."""
    raw = _u8(msgs32).tobytes()
    if len(raw) % 32:
        raise ValueError("messages must be 32 bytes each")
    B = len(raw) // 32
    seen: dict[bytes, int] = {}
    ids = np.empty(B, dtype=np.uint32)
    for b in range(B):
        ids[b] = seen.setdefault(raw[32 * b: 32 * b + 32], len(seen))
    return b"".join(seen), ids


def _shared_args(table, msg_ids, B: int) -> tuple[np.ndarray, int, np.ndarray]:
    """(table bytes as u8, M, ids as uint32) of a shared-message batch of B items, checked on the host: the ids
    must name table entries (ValueError otherwise, before any device call)."""
    t = _u8(table)
    if t.size % 32:
        raise ValueError("the message table must be a multiple of 32 bytes")
    M = t.size // 32
    raw = np.asarray(msg_ids)
    if raw.ndim != 1 or raw.size != B:
        raise ValueError("need one message id per item")
    if B and raw.dtype.kind not in "ui":
        raise ValueError("message ids must be integers")
    if B and M == 0:
        raise ValueError("an empty message table")
    if B and (int(raw.min()) < 0 or int(raw.max()) >= M):
        raise ValueError("message id out of range")
    return t, M, np.ascontiguousarray(raw, dtype=np.uint32)


def fast_aggregate_verify_batch_shared(indices, offsets, table, msg_ids, sigs96, ctx=None) -> np.ndarray:
    """fast_aggregate_verify_batch for items that share messages: item b signs table[32 * msg_ids[b] ..] (see
    group_messages).  Same verdicts as the unshared call on the expanded messages, with one hash_to_G2 and one
    Miller pair per table entry instead of per item (bls_fav_batch_indexed_shared).  Worth it when the table is
    shorter than the batch."""
    idx = np.ascontiguousarray(indices, dtype=np.uint32)
    offs = np.ascontiguousarray(offsets, dtype=np.uint64)
    B = offs.size - 1
    t, M, ids = _shared_args(table, msg_ids, B)
    s = _u8(sigs96)
    if s.size != 96 * B:
        raise ValueError("need one 96-byte signature per aggregate")
    c = ctx or _native.context()
    out = np.zeros(B, dtype=np.uint8)
    c.check(c.lib.bls_fav_batch_indexed_shared(c.h, _ptr(idx), _ptr(offs), B, t.tobytes(), M, _ptr(ids), s.tobytes(),
                                               _ptr(out)))
    return out.astype(bool)


def verify_batch_shared(indices, table, msg_ids, sigs96, ctx=None) -> np.ndarray:
    """verify_batch for items that share messages (fast_aggregate_verify_batch_shared with one key per item)."""
    idx = np.ascontiguousarray(indices, dtype=np.uint32)
    B = idx.size
    t, M, ids = _shared_args(table, msg_ids, B)
    s = _u8(sigs96)
    if s.size != 96 * B:
        raise ValueError("need one 96-byte signature per item")
    c = ctx or _native.context()
    out = np.zeros(B, dtype=np.uint8)
    c.check(c.lib.bls_verify_batch_indexed_shared(c.h, _ptr(idx), B, t.tobytes(), M, _ptr(ids), s.tobytes(),
                                                  _ptr(out)))
    return out.astype(bool)


def key_table(pubkey_lists) -> tuple[bytes, np.ndarray, np.ndarray]:
    """Deduplicate the keys of B key lists on the host: (table, idx, offsets) with the distinct 48-byte keys in
    order of first occurrence, idx (uint32) the table entry of every key of every list in order, and offsets
    (uint64, B + 1) the lists' bounds in idx -- the arguments of fast_aggregate_verify_batch_keys.  A block's
    attestations over a small state reuse few keys, so the table (whose every entry costs the batch a KeyValidate)
    stays short.  A key repeated inside one list stays repeated in idx: it counts twice, as the per-call path counts
    it."""
    seen: dict[bytes, int] = {}
    flat, lens = [], []
    for keys in pubkey_lists:
        n = 0
        for k in keys:
            k = bytes(k)
            if len(k) != 48:
                raise ValueError("pubkeys must be 48 bytes each")
            flat.append(seen.setdefault(k, len(seen)))
            n += 1
        lens.append(n)
    return b"".join(seen), np.asarray(flat, dtype=np.uint32), offsets_from_lengths(lens)


def fast_aggregate_verify_batch_keys(table, idx, offsets, msgs32, sigs96, msg_ids=None, ctx=None,
                                     want_key_valid: bool = False):
    """B FastAggregateVerify calls on keys given as bytes, no registry needed or touched (bls_fav_batch_keys):
    `table` holds K compressed keys (see key_table) and item b uses entries idx[offsets[b]: offsets[b + 1]].  The
    verdicts are fast_aggregate_verify_batch's for the same idx / offsets on a registry loaded with `table`; with
    msg_ids, msgs32 is a message table and item b signs entry msg_ids[b] (group_messages), as in
    fast_aggregate_verify_batch_shared.  want_key_valid: returns (verdicts, KeyValidate mask of the table).

    The batch KeyValidates all K entries every time -- what the registry does once per key.  Keys that come back
    batch after batch (the validator set) belong in a Registry; this is for keys that are not in one."""
    t = _u8(table)
    if t.size % 48:
        raise ValueError("the key table must be a multiple of 48 bytes")
    K = t.size // 48
    ix = np.ascontiguousarray(idx, dtype=np.uint32)
    offs = np.ascontiguousarray(offsets, dtype=np.uint64)
    if offs.ndim != 1 or offs.size < 1 or np.any(offs[1:] < offs[:-1]) or int(offs[-1]) > ix.size:
        raise ValueError("offsets must be non-decreasing and end inside the index array")
    B = offs.size - 1
    s = _u8(sigs96)
    if s.size != 96 * B:
        raise ValueError("need one 96-byte signature per aggregate")
    if msg_ids is not None:
        m, M, ids = _shared_args(msgs32, msg_ids, B)
        ids_p = _ptr(ids)
    else:
        m, M, ids_p = _u8(msgs32), 0, None
        if m.size != 32 * B:
            raise ValueError("need one 32-byte message per aggregate")
    c = ctx or _native.context()
    out = np.zeros(B, dtype=np.uint8)
    valid = np.zeros(K, dtype=np.uint8) if want_key_valid else None
    c.check(c.lib.bls_fav_batch_keys(c.h, t.tobytes(), K, _ptr(ix), _ptr(offs), B, m.tobytes(), M, ids_p, s.tobytes(),
                                     _ptr(out), None if valid is None else _ptr(valid)))
    return (out.astype(bool), valid) if want_key_valid else out.astype(bool)


def verify_batch_keys(pubkeys48, msgs32, sigs96, msg_ids=None, ctx=None) -> np.ndarray:
    """B Verify calls on raw keys (bls_verify_batch_keys): item b's key is pubkeys48[48 b: 48 b + 48].  The keys
    batch with one key per item; msg_ids as in fast_aggregate_verify_batch_keys."""
    k = _u8(pubkeys48)
    if k.size % 48:
        raise ValueError("pubkeys must be a multiple of 48 bytes")
    B = k.size // 48
    s = _u8(sigs96)
    if s.size != 96 * B:
        raise ValueError("need one 96-byte signature per key")
    if msg_ids is not None:
        m, M, ids = _shared_args(msgs32, msg_ids, B)
        ids_p = _ptr(ids)
    else:
        m, M, ids_p = _u8(msgs32), 0, None
        if m.size != 32 * B:
            raise ValueError("need one 32-byte message per key")
    c = ctx or _native.context()
    out = np.zeros(B, dtype=np.uint8)
    c.check(c.lib.bls_verify_batch_keys(c.h, k.tobytes(), B, m.tobytes(), M, ids_p, s.tobytes(), _ptr(out)))
    return out.astype(bool)


def verify_deposits(pubkeys, withdrawal_credentials, amounts, signatures, domain, want_roots: bool = False, ctx=None):
    """N deposit signature checks (is_valid_deposit_signature; bls_deposits_verify): verdict i is
    Verify(pubkeys[i], compute_signing_root(DepositMessage(pubkeys[i], withdrawal_credentials[i], amounts[i]),
    domain), signatures[i]), the roots hashed on the device and the signatures checked as one keys batch.
    want_roots: returns (verdicts, the N signing roots).  An accepted new key is not added to any registry
    (Registry.append is the caller's: it knows which deposits are top-ups)."""
    pk = b"".join(bytes(k) for k in pubkeys)
    wc = b"".join(bytes(w) for w in withdrawal_credentials)
    sg = b"".join(bytes(s) for s in signatures)
    N = len(pubkeys)
    if len(pk) != 48 * N or any(len(bytes(k)) != 48 for k in pubkeys):
        raise ValueError("pubkeys must be 48 bytes each")
    if len(withdrawal_credentials) != N or len(wc) != 32 * N:
        raise ValueError("need one 32-byte withdrawal credential per deposit")
    if len(signatures) != N or len(sg) != 96 * N or any(len(bytes(s)) != 96 for s in signatures):
        raise ValueError("need one 96-byte signature per deposit")
    if len(amounts) != N or any(not 0 <= int(a) < 1 << 64 for a in amounts):
        raise ValueError("need one uint64 amount per deposit")
    if len(bytes(domain)) != 32:
        raise ValueError("the domain must be 32 bytes")
    amt = np.asarray([int(a) for a in amounts], dtype=np.uint64)
    c = ctx or _native.context()
    out = np.zeros(N, dtype=np.uint8)
    roots = ctypes.create_string_buffer(32 * N) if want_roots and N else None
    c.check(c.lib.bls_deposits_verify(c.h, pk, wc, _ptr(amt), sg, bytes(domain), N, _ptr(out), roots))
    if want_roots:
        raw = roots.raw if roots is not None else b""
        return out.astype(bool), [raw[32 * i: 32 * i + 32] for i in range(N)]
    return out.astype(bool)


class Committees:
    """HBM-resident committee table of one context (bls_committees_load): every committee a list of registry
    indices, fixed for an epoch.  The device keeps each committee's key sum, so that a nearly full aggregate costs
    its absentees instead of its participants (fast_aggregate_verify_batch_bits).  The table belongs to the
    registry it was loaded on: Registry.load / generate make it stale (the bits calls then raise), append keeps
    it."""

    def __init__(self, ctx: _native.Context | None = None):
        self.ctx = ctx or _native.context()
        self.sizes = np.zeros(0, dtype=np.uint64)

    def load(self, index_lists) -> "Committees":
        """index_lists: one sequence of registry indices per committee, or the tuple (flat, offsets) with
        committee c = flat[offsets[c]: offsets[c + 1]].  Replaces any earlier table of the context."""
        if isinstance(index_lists, tuple) and len(index_lists) == 2:
            flat = np.ascontiguousarray(index_lists[0], dtype=np.uint32)
            offs = np.ascontiguousarray(index_lists[1], dtype=np.uint64)
        else:
            lists = [np.asarray(c, dtype=np.uint32).reshape(-1) for c in index_lists]
            flat = np.ascontiguousarray(np.concatenate(lists) if lists else np.zeros(0, np.uint32), dtype=np.uint32)
            offs = offsets_from_lengths([c.size for c in lists])
        if offs.ndim != 1 or offs.size < 1 or np.any(offs[1:] < offs[:-1]) or int(offs[-1]) > flat.size:
            raise ValueError("offsets must be non-decreasing and end inside the index array")
        c = self.ctx
        c.check(c.lib.bls_committees_load(c.h, _ptr(flat), _ptr(offs), offs.size - 1))
        self.sizes = np.diff(offs)
        return self

    def __len__(self):
        return int(self.sizes.size)


def bits_from_bitlist(ssz_bytes, n: int) -> bytes:
    """The ceil(n / 8) participation bytes of a serialized SSZ Bitlist of n bits (aggregation_bits): the
    delimiter bit at position n is checked and stripped."""
    raw = bytes(ssz_bytes)
    if n < 0 or len(raw) != n // 8 + 1 or raw[-1] >> (n % 8) != 1:
        raise ValueError("not a serialized Bitlist of that length")
    body = bytearray(raw[: (n + 7) // 8])
    if n % 8:
        body[-1] &= (1 << (n % 8)) - 1
    return bytes(body)


BITS_MODES = {"auto": 0, "direct": 1, "complement": 2}


def _bits_args(committees: Committees, committee_ids, bits, B: int):
    """(comm_ids u32, comm_offs u64, bit bytes u8, bit_offs u64) of a bits batch of B items, checked on the host
    (ValueError before any device call): every id names a committee of the table, and item b carries exactly
    ceil(n_b / 8) bytes -- or a bool array of n_b entries, packed here -- for the n_b members of its committees."""
    if len(committee_ids) != B or len(bits) != B:
        raise ValueError("need one committee id (or list of ids) and one bitfield per item")
    C = len(committees)
    per_item = []
    for ids in committee_ids:
        a = np.asarray(ids)
        if a.size and a.dtype.kind not in "ui":
            raise ValueError("committee ids must be integers")
        a = a.reshape(-1)
        if a.size and (int(a.min()) < 0 or int(a.max()) >= C):
            raise ValueError("committee id out of range")
        per_item.append(a.astype(np.uint32))
    comm_offs = offsets_from_lengths([a.size for a in per_item])
    comm_ids = np.ascontiguousarray(np.concatenate(per_item) if per_item else np.zeros(0, np.uint32), dtype=np.uint32)
    packed = []
    for a, bf in zip(per_item, bits):
        n = int(committees.sizes[a].sum()) if a.size else 0
        if isinstance(bf, (bytes, bytearray, memoryview)):
            raw = bytes(bf)
        else:
            arr = np.asarray(bf)
            if arr.dtype != np.bool_ or arr.ndim != 1 or arr.size != n:
                raise ValueError("a bit array needs one bool per member of the item's committees")
            raw = np.packbits(arr, bitorder="little").tobytes()
        if len(raw) != (n + 7) // 8:
            raise ValueError("an item needs ceil(n / 8) bytes of bits for the n members of its committees")
        packed.append(raw)
    bit_offs = offsets_from_lengths([len(r) for r in packed])
    return comm_ids, comm_offs, np.frombuffer(b"".join(packed), dtype=np.uint8), bit_offs


def _mode(mode) -> int:
    if mode not in BITS_MODES:
        raise ValueError('mode must be "auto", "direct" or "complement"')
    return BITS_MODES[mode]


def fast_aggregate_verify_batch_bits(committees: Committees, committee_ids, bits, msgs32, sigs96, msg_ids=None,
                                     table=None, mode: str = "auto", ctx=None) -> np.ndarray:
    """B FastAggregateVerify calls whose signers are (committees, participation bits), as an attestation carries
    them: committee_ids[b] is a committee number or a list of them, bits[b] the item's bitfield over their
    concatenated members (bytes in SSZ bit order without the delimiter -- see bits_from_bitlist -- or a bool
    array).  Same verdicts as fast_aggregate_verify_batch on the expanded indices; with msg_ids, as
    fast_aggregate_verify_batch_shared over `table` (default: msgs32 is the table).  mode: "auto" subtracts the
    absentees from the committees' cached sums when that adds fewer points; "direct" / "complement" force a form
    (tests, measurements)."""
    B = len(committee_ids)
    m = _mode(mode)
    comm_ids, comm_offs, raw, bit_offs = _bits_args(committees, committee_ids, bits, B)
    s = _u8(sigs96)
    if s.size != 96 * B:
        raise ValueError("need one 96-byte signature per aggregate")
    if msg_ids is not None:
        t, M, ids = _shared_args(msgs32 if table is None else table, msg_ids, B)
        ids_p = _ptr(ids)
    else:
        t, M, ids_p = _u8(msgs32), 0, None
        if t.size != 32 * B:
            raise ValueError("need one 32-byte message per aggregate")
    c = ctx or committees.ctx
    out = np.zeros(B, dtype=np.uint8)
    c.check(c.lib.bls_fav_batch_committee_bits(c.h, _ptr(comm_ids), _ptr(comm_offs), _ptr(raw), _ptr(bit_offs), B,
                                               t.tobytes(), M, ids_p, s.tobytes(), m, _ptr(out)))
    return out.astype(bool)


def gather_work(ctx=None) -> tuple[int, int]:
    """(points added, complement items) of the last bits batch prepared on the context: the keys its gather
    added plus the committee sums of its complement items, and how many items took the complement form."""
    c = ctx or _native.context()
    pts, cmpl = ctypes.c_uint64(), ctypes.c_uint64()
    c.check(c.lib.bls_last_gather_work(c.h, ctypes.byref(pts), ctypes.byref(cmpl)))
    return int(pts.value), int(cmpl.value)


def _group_args(group_ids, n_groups, include, B: int) -> tuple[np.ndarray, int, np.ndarray | None]:
    """(ids as uint32, G, mask as u8 or None) of a grouped aggregation of B signatures, checked on the host
    (ValueError before any device call): one integer id in [0, G) per signature, one mask byte per signature."""
    raw = np.asarray(group_ids)
    if raw.ndim != 1 or raw.size != B:
        raise ValueError("need one group id per signature")
    if B and raw.dtype.kind not in "ui":
        raise ValueError("group ids must be integers")
    if B and int(raw.min()) < 0:
        raise ValueError("group id out of range")
    if n_groups is None:
        G = int(raw.max()) + 1 if B else 0
    else:
        G = int(n_groups)
        if G < 0 or G != n_groups:
            raise ValueError("n_groups must be a non-negative integer")
    if B and int(raw.max()) >= G:
        raise ValueError("group id out of range")
    mask = None
    if include is not None:
        mask = np.asarray(include)
        if mask.ndim != 1 or mask.size != B:
            raise ValueError("need one mask entry per signature")
        mask = np.ascontiguousarray(mask != 0, dtype=np.uint8)
    return np.ascontiguousarray(raw, dtype=np.uint32), G, mask


def _grouped_result(out: np.ndarray, ok: np.ndarray) -> list:
    raw = out.tobytes()
    return [raw[96 * g: 96 * g + 96] if ok[g] else None for g in range(ok.size)]


def aggregate_grouped(sigs96, group_ids, n_groups=None, include=None, subgroup_check: bool = True, ctx=None) -> list:
    """n_groups Aggregate calls in one (bls_aggregate_grouped): result[g] is the aggregate of the signatures b with
    group_ids[b] == g (and include[b] true, when a mask is given), or None where bls.Aggregate would raise -- a
    group with no included signature, or one whose included signatures do not all decode (and, with
    subgroup_check, lie in G2).  A bad signature spoils only its own group; an excluded one is never judged.
    n_groups defaults to max(id) + 1.  subgroup_check=False is for signatures a batch has already verified
    (include = its verdicts)."""
    s = _u8(sigs96)
    if s.size % 96:
        raise ValueError("signatures must be 96 bytes each")
    B = s.size // 96
    ids, G, mask = _group_args(group_ids, n_groups, include, B)
    c = ctx or _native.context()
    out = np.zeros(96 * max(G, 1), dtype=np.uint8)
    ok = np.zeros(max(G, 1), dtype=np.uint8)
    c.check(c.lib.bls_aggregate_grouped(c.h, _ptr(s), B, _ptr(ids), G, None if mask is None else _ptr(mask),
                                        1 if subgroup_check else 0, _ptr(out), _ptr(ok)))
    return _grouped_result(out[: 96 * G], ok[:G])


def batch_work(ctx=None) -> tuple[int, int]:
    """(messages hashed, Miller pairs) of the last FAV / Verify batch prepared on the context: (B, B + 64)
    unshared, (M, M + 64) shared."""
    c = ctx or _native.context()
    h, p = ctypes.c_uint64(), ctypes.c_uint64()
    c.check(c.lib.bls_last_batch_work(c.h, ctypes.byref(h), ctypes.byref(p)))
    return int(h.value), int(p.value)


def aggregate_verify_batch(pubkeys, messages, signatures, ctx=None) -> np.ndarray:
    """B AggregateVerify calls -> bool array.  pubkeys[b] / messages[b]: item b's lists of 48-byte keys
    and messages (any lengths, equal list lengths); signatures[b]: 96 bytes.  An item whose lists differ
    in length, or with a key other than 48 bytes or a signature other than 96, is False
    (E/utils/bls.py:154-164 returns False on any exception); the rest are checked in one batch
    (bls_aggregate_verify_batch)."""
    c = ctx or _native.context()
    B = len(signatures)
    if len(pubkeys) != B or len(messages) != B:
        raise ValueError("need one pubkey list, one message list and one signature per item")
    good = np.array([len(p) == len(m) and len(bytes(s)) == 96 and all(len(bytes(k)) == 48 for k in p)
                     for p, m, s in zip(pubkeys, messages, signatures)], dtype=bool)
    lens = [len(p) if g else 0 for p, g in zip(pubkeys, good)]
    io = offsets_from_lengths(lens)
    flat_pk = [bytes(k) for p, g in zip(pubkeys, good) if g for k in p]
    flat_m = [bytes(m) for ms, g in zip(messages, good) if g for m in ms]
    mo = offsets_from_lengths([len(m) for m in flat_m])
    sigs = b"".join(bytes(s) if g else bytes(96) for s, g in zip(signatures, good))
    out = np.zeros(B, dtype=np.uint8)
    if B:
        c.check(c.lib.bls_aggregate_verify_batch(c.h, b"".join(flat_pk), b"".join(flat_m), _ptr(mo), _ptr(io), B,
                                                 sigs, _ptr(out)))
    return out.astype(bool) & good


def compute_signing_roots(object_roots, domains, ctx=None) -> list[bytes]:
    """compute_signing_root for many objects on the device (specs/phase0/beacon-chain.md:953-962):
    SHA-256(object_root || domain).  ``domains``: one 32-byte domain for all, or one per root."""
    c = ctx or _native.context()
    roots = [bytes(r) for r in object_roots]
    if any(len(r) != 32 for r in roots):
        raise ValueError("object roots must be 32 bytes")
    if isinstance(domains, (bytes, bytearray)) and len(domains) == 32:
        dom, stride = bytes(domains), 0
    else:
        dl = [bytes(d) for d in domains]
        if len(dl) != len(roots) or any(len(d) != 32 for d in dl):
            raise ValueError("need one 32-byte domain, or one per root")
        dom, stride = b"".join(dl), 32
    n = len(roots)
    out = ctypes.create_string_buffer(32 * n) if n else None
    c.check(c.lib.bls_signing_roots(c.h, b"".join(roots), dom, stride, n, out))
    return [out.raw[32 * i: 32 * i + 32] for i in range(n)]


def merkleize(chunks, limit: int | None = None, ctx=None) -> bytes:
    """SSZ merkleize(chunks, limit) on the device: the tree has next_pow2(limit or len(chunks)) leaves."""
    c = ctx or _native.context()
    ch = [bytes(x) for x in chunks]
    if any(len(x) != 32 for x in ch):
        raise ValueError("chunks must be 32 bytes")
    n = len(ch)
    size = n if limit is None else limit
    if size < n:
        raise ValueError("more chunks than the limit")
    depth = max(size - 1, 0).bit_length()
    out = ctypes.create_string_buffer(32)
    c.check(c.lib.bls_merkleize(c.h, b"".join(ch) if n else None, n, depth, out))
    return out.raw


def mix_in_length(root: bytes, length: int) -> bytes:
    """hash_tree_root of a list: SHA-256(root || uint256 length little-endian) -- one node, host hashlib."""
    import hashlib

    return hashlib.sha256(bytes(root) + int(length).to_bytes(32, "little")).digest()


def pairing_check(pairs, ctx=None) -> bool:
    """KZG pairing_check (E/utils/bls.py; specs/deneb/polynomial-commitments.md:284,407,451):
    prod e(P_i, Q_i) == 1 over compressed (48-byte G1, 96-byte G2) pairs; the identity is allowed,
    an invalid encoding gives False."""
    c = ctx or _native.context()
    g1 = [bytes(p) for p, _ in pairs]
    g2 = [bytes(q) for _, q in pairs]
    if any(len(p) != 48 for p in g1) or any(len(q) != 96 for q in g2):
        raise ValueError("need 48-byte G1 and 96-byte G2 encodings")
    return c.check(c.lib.bls_pairing_check(c.h, b"".join(g1), b"".join(g2), len(g1))) == 1


def g1_multi_exp(points48, scalars, ctx=None, subgroup_check: bool = False) -> bytes:
    """KZG multi_exp / g1_lincomb on compressed points: sum [k_i] P_i (E/utils/bls.py:262-296 -> arkworks
    G1.multiexp_unchecked, i.e. no subgroup check unless asked); scalars are ints (0 <= k < 2^256).  Raises on
    an empty input (E/utils/bls.py:270-271) and on an invalid encoding, like the reference.

    Every call copies and decompresses every point again.  For a point set that is multiplied repeatedly (the KZG
    trusted setup), load it once into a ``G1Table`` and use ``g1_lincomb_indexed`` / ``g1_lincomb_batch``."""
    c = ctx or _native.context()
    pts = [bytes(p) for p in points48]
    ks = [int(k) for k in scalars]
    if not pts or not ks:
        raise ValueError("Cannot call multi_exp with zero points or zero scalars")
    if len(pts) != len(ks):
        raise ValueError("one scalar per point")
    if any(len(p) != 48 for p in pts) or any(not 0 <= k < 1 << 256 for k in ks):
        raise ValueError("need 48-byte points and 256-bit scalars")
    # reduced mod r as curve.Scalar / curve._k32 do (arkworks' Scalar): for a point decoded without the subgroup
    # check, [k]P and [k mod r]P differ, and both entry points must give the same result
    ks = [k % R_ORDER for k in ks]
    out = ctypes.create_string_buffer(48)
    rc = c.check(c.lib.bls_multi_exp(c.h, 1, b"".join(pts), b"".join(k.to_bytes(32, "big") for k in ks), len(pts),
                                     1 if subgroup_check else 0, out))
    if rc != 1:
        raise ValueError("invalid G1 point encoding")
    return out.raw


class G1Table:
    """HBM-resident G1 point table of one context (``bls_g1_table_*``): the points are decoded once and kept with
    their window multiples, so that ``g1_lincomb_indexed`` / ``g1_lincomb_batch`` over them add only.

    The host keeps a point-bytes -> index map for what was loaded or appended through this object, tied to the
    library's table generation as ``Registry``'s map is: after another object replaces the device table, lookups
    return None.  ``checked`` says whether every entry went through the subgroup check; ``usable(i)`` whether
    entry i decoded (an invalid encoding keeps its index and makes an MSM that names it raise)."""

    def __init__(self, ctx: _native.Context | None = None):
        self.ctx = ctx or _native.context()
        self._index: dict[bytes, int] = {}
        self._last: dict[bytes, int] = {}  # the highest index of every point: ``run_of`` past repeated points
        self._ok = np.zeros(0, dtype=np.uint8)
        self._gen = None
        self.checked = False

    def _generation(self) -> int:
        return int(self.ctx.lib.bls_g1_table_generation(self.ctx.h))

    def _current(self) -> bool:
        return self._gen is not None and self._gen == self._generation()

    @staticmethod
    def _points(points48) -> np.ndarray:
        if isinstance(points48, (bytes, bytearray, memoryview, np.ndarray)):
            buf = _u8(points48)
        else:
            buf = _u8(b"".join(bytes(p) for p in points48))
        if buf.size % 48:
            raise ValueError("points must be 48 bytes each")
        return buf

    def _remember(self, buf: np.ndarray, first: int, ok: np.ndarray) -> None:
        raw = buf.tobytes()
        for i in range(len(raw) // 48):
            self._index.setdefault(raw[48 * i: 48 * i + 48], first + i)
            self._last[raw[48 * i: 48 * i + 48]] = first + i
        self._ok = np.concatenate([self._ok[:first], ok])

    def load(self, points48, subgroup_check: bool = False) -> np.ndarray:
        """Replace the table with these compressed points (one bytes object or a sequence of 48-byte encodings);
        returns the per-encoding verdicts (1 = decodes and, with subgroup_check, lies in G1)."""
        buf = self._points(points48)
        n = buf.size // 48
        ok = np.zeros(n, dtype=np.uint8)
        c = self.ctx
        self._index, self._last, self._gen, self._ok = {}, {}, None, np.zeros(0, dtype=np.uint8)
        c.check(c.lib.bls_g1_table_load(c.h, buf.tobytes(), n, 1 if subgroup_check else 0, _ptr(ok)))
        self.checked = bool(subgroup_check)
        self._remember(buf, 0, ok)
        self._gen = self._generation()
        return ok

    def append(self, points48, subgroup_check: bool = False) -> np.ndarray:
        """Add points at indices len(self) ..; existing indices stay."""
        buf = self._points(points48)
        n = buf.size // 48
        first = len(self)
        ok = np.zeros(n, dtype=np.uint8)
        c = self.ctx
        c.check(c.lib.bls_g1_table_append(c.h, buf.tobytes(), n, 1 if subgroup_check else 0, _ptr(ok)))
        if self._current():
            self.checked = self.checked and bool(subgroup_check)
            self._remember(buf, first, ok)
        return ok

    def indices(self, points) -> np.ndarray | None:
        """u32 table indices of every point (bytes-like encodings), or None if any is absent or the map is stale."""
        if not self._current():
            return None
        out = np.empty(len(points), dtype=np.uint32)
        for i, p in enumerate(points):
            k = self._index.get(bytes(p))
            if k is None:
                return None
            out[i] = k
        return out

    def run_of(self, points) -> int | None:
        """the index at which the points lie in the table as one consecutive run, by their first or by their last
        occurrences (a list appended behind a shorter copy of its head is found by the latter); else None"""
        if not self._current() or not len(points):
            return None
        for where in (self._index, self._last):
            idx = [where.get(bytes(p)) for p in points]
            if idx[0] is not None and idx == list(range(idx[0], idx[0] + len(idx))):
                return idx[0]
        return None

    def usable(self, i: int) -> bool:
        return self._current() and 0 <= i < self._ok.size and bool(self._ok[i])

    def all_usable(self, idx: np.ndarray) -> bool:
        """whether every index of an ``indices()`` result names an entry that decoded"""
        return self._current() and bool(self._ok[idx].all())

    def __len__(self):
        return int(self.ctx.lib.bls_g1_table_size(self.ctx.h))


def _lincomb_rows(scalar_rows, n: int) -> bytes:
    rows = []
    for row in scalar_rows:
        ks = [int(k) for k in row]
        if len(ks) != n:
            raise ValueError("one scalar per index in every row")
        if any(not 0 <= k < 1 << 256 for k in ks):
            raise ValueError("need 256-bit scalars")
        rows.append(b"".join(k.to_bytes(32, "big") for k in ks))
    return b"".join(rows)


def g1_lincomb_batch(table: G1Table, idx, scalar_rows) -> list:
    """B linear combinations over one shared index list in one call (``bls_g1_table_msm``): result[v] =
    sum_i [scalar_rows[v][i]] T[idx[i]], 48 compressed bytes each.  Scalars are ints 0 <= k < 2^256 and are taken
    as integer multiples, as the C ABI takes them (no reduction mod r here: reduce first, as ``g1_multi_exp``
    does, where the table holds points outside G1).  Raises ValueError on an empty index list (the reference
    raises on an empty multi_exp), on an index outside the table and when an index names an entry whose encoding
    was invalid at load."""
    a_idx = np.ascontiguousarray(idx, dtype=np.uint32)
    if a_idx.ndim != 1 or a_idx.size == 0:
        raise ValueError("Cannot call multi_exp with zero points or zero scalars")
    n = a_idx.size
    rows = _lincomb_rows(scalar_rows, n)
    B = len(rows) // (32 * n)
    if B == 0:
        return []
    c = table.ctx
    out = ctypes.create_string_buffer(48 * B)
    rc = c.lib.bls_g1_table_msm(c.h, _ptr(a_idx), n, rows, B, out)
    if rc == _native.BLS_E_ARG:
        raise ValueError("index outside the G1 table, or too many scalars for one call")
    if c.check(rc) != 1:
        raise ValueError("an index names an invalid G1 point encoding")
    return [out.raw[48 * v: 48 * v + 48] for v in range(B)]


def g1_lincomb_indexed(table: G1Table, idx, scalars) -> bytes:
    """sum_i [scalars[i]] T[idx[i]] over a resident table: ``g1_lincomb_batch`` with one row."""
    return g1_lincomb_batch(table, idx, [scalars])[0]


def g1_table_stats(ctx=None) -> tuple[int, int, int]:
    """(table MSM calls, bucket entries added, decode hits served from the table) since the context was created:
    the first two from the library, the third counted by ``curve.G1Point`` while ``curve.use_g1_table`` is set."""
    c = ctx or _native.context()
    calls, entries = ctypes.c_uint64(), ctypes.c_uint64()
    c.check(c.lib.bls_g1_table_stats(c.h, ctypes.byref(calls), ctypes.byref(entries)))
    return int(calls.value), int(entries.value), int(getattr(c, "g1_decode_hits", 0))


def g1_msm(points48, scalar_rows, subgroup_check: bool = False, ctx=None) -> list:
    """B linear combinations over the call's own points in one call (``bls_g1_msm``, a bucket MSM without a resident
    table): result[v] = sum_i [scalar_rows[v][i]] P_i, 48 compressed bytes each.  Points are 48-byte encodings,
    decoded without the subgroup check unless asked; scalars are ints 0 <= k < 2^256, one per point in every row.
    They are passed as given and taken as integer multiples, like ``g1_lincomb_batch``'s (no reduction mod r here:
    for the reduced form that the reference's Scalar gives, use ``g1_multi_exp``, or reduce first).  Raises ValueError
    on an empty input (the reference raises on an empty multi_exp) and on an invalid encoding or, with
    ``subgroup_check``, a point outside G1."""
    c = ctx or _native.context()
    pts = [bytes(p) for p in points48]
    if not pts:
        raise ValueError("Cannot call multi_exp with zero points or zero scalars")
    if any(len(p) != 48 for p in pts):
        raise ValueError("need 48-byte points and 256-bit scalars")
    n = len(pts)
    rows = _lincomb_rows(scalar_rows, n)
    B = len(rows) // (32 * n)
    if B == 0:
        raise ValueError("Cannot call multi_exp with zero points or zero scalars")
    out = ctypes.create_string_buffer(48 * B)
    rc = c.lib.bls_g1_msm(c.h, b"".join(pts), n, rows, B, 1 if subgroup_check else 0, out)
    if rc == _native.BLS_E_ARG:
        raise ValueError("too many rows or scalars for one call")
    if c.check(rc) != 1:
        raise ValueError("invalid G1 point encoding")
    return [out.raw[48 * v: 48 * v + 48] for v in range(B)]


def g1_msm_stats(ctx=None) -> tuple[int, int]:
    """(``g1_msm`` calls that ran, bucket entries their sorts placed) since the context was created
    (``bls_g1_msm_stats``): which route ran, and how many non-zero digits of non-identity points it saw."""
    c = ctx or _native.context()
    calls, entries = ctypes.c_uint64(), ctypes.c_uint64()
    c.check(c.lib.bls_g1_msm_stats(c.h, ctypes.byref(calls), ctypes.byref(entries)))
    return int(calls.value), int(entries.value)


def g1_fft(points, inverse: bool = False, ctx=None):
    """The radix-2 transform over G1 on the device (``bls_g1_fft``): out[k] = sum_i [w_n^(i k)] points[i], w_n the
    n-th root of unity of the cell functions' domain, in natural order on both sides; ``inverse`` takes w_n^-1 and
    includes 1 / n.  ``points``: n = 2^k (2 <= n <= 4,096) 48-byte encodings, the identity allowed anywhere -- or a
    list of such lists of one length, transformed in one call, which returns a list of lists.  Raises ValueError on
    a size the call does not take and on an encoding that is invalid or not in G1."""
    c = ctx or _native.context()
    rows = list(points)
    nested = bool(rows) and not isinstance(rows[0], (bytes, bytearray, memoryview))
    vecs = [[bytes(p) for p in v] for v in rows] if nested else [[bytes(p) for p in rows]]
    n = len(vecs[0])
    if any(len(v) != n for v in vecs) or any(len(p) != 48 for v in vecs for p in v):
        raise ValueError("need vectors of one length of 48-byte G1 encodings")
    out = ctypes.create_string_buffer(max(48 * n * len(vecs), 1))
    rc = c.lib.bls_g1_fft(c.h, b"".join(b"".join(v) for v in vecs), n, len(vecs), 1 if inverse else 0, out)
    if rc == _native.BLS_E_ARG:
        raise ValueError("the G1 transform takes n = 2^k points, 2 <= n <= 4096, and at least one vector")
    if c.check(rc) != 1:
        raise ValueError("invalid G1 point encoding")
    raw = out.raw
    res = [[raw[48 * (n * v + i): 48 * (n * v + i + 1)] for i in range(n)] for v in range(len(vecs))]
    return res if nested else res[0]


def fallback_stats(ctx=None) -> tuple[int, int]:
    """(batched final-exponentiation checks, bisection rounds) of the last batch call; (0, 0) if it passed."""
    c = ctx or _native.context()
    checks, rounds = ctypes.c_uint64(), ctypes.c_uint64()
    c.check(c.lib.bls_last_fallback_stats(c.h, ctypes.byref(checks), ctypes.byref(rounds)))
    return int(checks.value), int(rounds.value)


def sign_batch(sks32, msgs32, ctx=None) -> bytes:
    c = ctx or _native.context()
    sk, m = _u8(sks32), _u8(msgs32)
    B = sk.size // 32
    out = ctypes.create_string_buffer(96 * B)
    if c.check(c.lib.bls_sign_batch(c.h, sk.tobytes(), m.tobytes(), B, out)) != 1:
        raise ValueError("invalid secret key in batch")
    return out.raw


def sk_to_pk_batch(sks32, ctx=None) -> bytes:
    c = ctx or _native.context()
    sk = _u8(sks32)
    B = sk.size // 32
    out = ctypes.create_string_buffer(48 * B)
    if c.check(c.lib.bls_sk_to_pk_batch(c.h, sk.tobytes(), B, out)) != 1:
        raise ValueError("invalid secret key in batch")
    return out.raw


class DeviceBuffer:
    """HBM buffer owned by a context (inputs resident before a timed region)."""

    def __init__(self, ctx: _native.Context, data: np.ndarray | bytes | None = None, nbytes: int | None = None):
        self.ctx = ctx
        arr = None if data is None else (np.ascontiguousarray(data) if isinstance(data, np.ndarray) else _u8(data))
        self.nbytes = int(arr.nbytes if arr is not None else nbytes)
        self.ptr = ctx.lib.bls_dev_alloc(ctx.h, max(self.nbytes, 1))
        if not self.ptr:
            raise _native.NativeError("bls_dev_alloc failed")
        if arr is not None and self.nbytes:
            ctx.check(ctx.lib.bls_h2d(ctx.h, self.ptr, _ptr(arr), self.nbytes))

    def to_host(self) -> np.ndarray:
        out = np.empty(self.nbytes, dtype=np.uint8)
        self.ctx.check(self.ctx.lib.bls_d2h(self.ctx.h, _ptr(out), self.ptr, self.nbytes))
        return out

    def free(self):
        if self.ptr:
            self.ctx.lib.bls_dev_free(self.ctx.h, self.ptr)
            self.ptr = None


class ResidentFavBatch:
    """A FastAggregateVerify batch whose inputs live in HBM (bench / multi-GPU).

    ``partial()`` runs this shard's checks and Miller loops and returns the
    576-byte Fp12 partial; partials of all shards are multiplied and
    final-exponentiated by ``check_partials``; ``finish()`` writes verdicts.
    """

    def __init__(self, indices, offsets, msgs32, sigs96, ctx=None, chunks: int = 1, msg_ids=None, committees=None,
                 committee_ids=None, bits=None, mode: str = "auto", keys=None):
        """chunks > 1 splits the batch into that many equal sub-batches (uniform committee size only), each
        submitted as its own FAV job: a pass over the batch is `chunks` jobs (large shards, e.g. the C4 firehose,
        stay within one job's scratch).

        msg_ids (one per item): the items share messages -- msgs32 is then the message table and item b signs
        entry msg_ids[b] (group_messages); the batch runs through the job API (run_pipelined / run), one hash and
        one Miller pair per table entry.  Needs chunks == 1.

        committees / committee_ids / bits (indices and offsets None): the items are (committees, participation
        bits) over a Committees table, as in fast_aggregate_verify_batch_bits; only the bit bytes, messages and
        signatures are resident, and every chunk (B divisible by chunks, any item sizes) is submitted through
        bls_fav_job_submit_bits_dev in the given mode.  The batch runs through the job API.

        keys (a table of 48-byte compressed keys, see key_table): indices name entries of that table instead of
        the registry; the table is resident with the batch and every submit -- each chunk submits the whole table --
        goes through bls_fav_job_submit_keys_dev, which decodes and KeyValidates it into the job's own records.
        Works with msg_ids and with chunks (the uniform-size rule above).  The batch runs through the job API."""
        self.committees = committees
        self.keys, self.K = None, 0
        if keys is not None and committees is not None:
            raise ValueError("a batch takes a key table or a committees table, not both")
        if committees is not None:
            self._init_bits(committees, committee_ids, bits, msgs32, sigs96, ctx, chunks, msg_ids, mode)
            return
        if committee_ids is not None or bits is not None:
            raise ValueError("committee_ids and bits need a committees table")
        offs = np.ascontiguousarray(offsets, dtype=np.uint64)
        self.B = int(offs.size - 1)
        self.chunks = max(1, int(chunks))
        self.msg_ids, self.M = None, 0
        if msg_ids is not None:
            if self.chunks != 1:
                raise ValueError("a shared-message batch needs chunks == 1")
            _, self.M, self.msg_ids = _shared_args(msgs32, msg_ids, self.B)
        self.ctx = ctx or _native.context()
        if self.chunks > 1:
            n = int(offs[1] - offs[0]) if self.B else 0
            if self.B % self.chunks or not np.array_equal(offs, np.arange(self.B + 1, dtype=np.uint64) * n):
                raise ValueError("chunks > 1 needs B divisible by chunks and one committee size")
            self.cb, self.n = self.B // self.chunks, n
            offs = offs[: self.cb + 1]  # every chunk has the same relative offsets
        else:
            self.cb, self.n = self.B, None
        if keys is not None:
            t = _u8(keys)
            if t.size % 48:
                raise ValueError("the key table must be a multiple of 48 bytes")
            self.K = t.size // 48
            self.keys = DeviceBuffer(self.ctx, t)
        self.idx = DeviceBuffer(self.ctx, np.ascontiguousarray(indices, dtype=np.uint32))
        self.offs = DeviceBuffer(self.ctx, offs)
        self.msgs = DeviceBuffer(self.ctx, _u8(msgs32))
        self.sigs = DeviceBuffer(self.ctx, _u8(sigs96))
        self.outs = [DeviceBuffer(self.ctx, nbytes=self.B) for _ in range(FAV_JOBS)]
        self.out = self.outs[0]
        self.last_job = 0
        self._chunk_job = [0] * self.chunks  # job whose buffer holds each chunk's latest verdicts

    def _init_bits(self, committees, committee_ids, bits, msgs32, sigs96, ctx, chunks, msg_ids, mode):
        if committee_ids is None or bits is None:
            raise ValueError("a committees table needs committee_ids and bits")
        self.B = len(committee_ids)
        self.chunks = max(1, int(chunks))
        self.mode = _mode(mode)
        self.comm_ids, self.comm_offs, raw, self.bit_offs = _bits_args(committees, committee_ids, bits, self.B)
        self.msg_ids, self.M = None, 0
        if msg_ids is not None:
            if self.chunks != 1:
                raise ValueError("a shared-message batch needs chunks == 1")
            _, self.M, self.msg_ids = _shared_args(msgs32, msg_ids, self.B)
        elif _u8(msgs32).size != 32 * self.B:
            raise ValueError("need one 32-byte message per aggregate")
        if _u8(sigs96).size != 96 * self.B:
            raise ValueError("need one 96-byte signature per aggregate")
        if self.B % self.chunks:
            raise ValueError("chunks > 1 needs B divisible by chunks")
        self.cb, self.n = self.B // self.chunks, None
        self.ctx = ctx or committees.ctx
        self.idx = self.offs = None
        self.bits = DeviceBuffer(self.ctx, raw)
        self.msgs = DeviceBuffer(self.ctx, _u8(msgs32))
        self.sigs = DeviceBuffer(self.ctx, _u8(sigs96))
        self.outs = [DeviceBuffer(self.ctx, nbytes=self.B) for _ in range(FAV_JOBS)]
        self.out = self.outs[0]
        self.last_job = 0
        self._chunk_job = [0] * self.chunks

    def partial(self, seed32: bytes | None = None) -> bytes:
        if self.chunks > 1 or self.msg_ids is not None or self.committees is not None or self.keys is not None:
            raise ValueError("a chunked, shared-message, bits or keys batch runs through the job API (run_pipelined)")
        seed = seed32 if seed32 is not None else os.urandom(32)
        buf = ctypes.create_string_buffer(576)
        c = self.ctx
        c.check(c.lib.bls_fav_batch_partial_dev(c.h, self.idx.ptr, self.offs.ptr, self.B, self.msgs.ptr,
                                                self.sigs.ptr, seed, buf))
        return buf.raw

    def check_partials(self, partials: bytes) -> bool:
        c = self.ctx
        n = len(partials) // 576
        return c.check(c.lib.bls_partials_check(c.h, partials, n)) == 1

    def finish(self, batch_ok: bool) -> None:
        c = self.ctx
        c.check(c.lib.bls_fav_batch_finish_dev(c.h, 1 if batch_ok else 0, self.out.ptr))
        self.last_job = 0

    # ---- pipelined passes (bls_fav_job_*): up to FAV_JOBS batches in flight --
    def _chunk_ptrs(self, c: int):
        lo = c * self.cb
        nidx = lo * self.n if self.chunks > 1 else 0
        return self.idx.ptr + 4 * nidx, self.msgs.ptr + 32 * lo, self.sigs.ptr + 96 * lo, lo

    def submit(self, job: int, seed32: bytes, chunk: int = 0) -> None:
        c = self.ctx
        if self.committees is not None:
            # the chunk's slices of the host offset tables index the whole comm_ids array and the whole bits buffer
            lo = chunk * self.cb
            co = self.comm_offs[lo: lo + self.cb + 1]
            bo = self.bit_offs[lo: lo + self.cb + 1]
            shared = self.msg_ids is not None
            c.check(c.lib.bls_fav_job_submit_bits_dev(
                c.h, job, _ptr(self.comm_ids), _ptr(co), self.bits.ptr, _ptr(bo), self.cb,
                self.msgs.ptr + (0 if shared else 32 * lo), self.M, _ptr(self.msg_ids) if shared else None,
                self.sigs.ptr + 96 * lo, self.mode, seed32))
            return
        idx, msgs, sigs, _ = self._chunk_ptrs(chunk)
        if self.keys is not None:
            shared = self.msg_ids is not None
            c.check(c.lib.bls_fav_job_submit_keys_dev(c.h, job, self.keys.ptr, self.K, idx, self.offs.ptr, self.cb,
                                                      msgs, self.M, _ptr(self.msg_ids) if shared else None, sigs,
                                                      seed32))
            return
        if self.msg_ids is not None:
            c.check(c.lib.bls_fav_job_submit_shared_dev(c.h, job, idx, self.offs.ptr, self.cb, msgs, self.M,
                                                        _ptr(self.msg_ids), sigs, seed32))
            return
        c.check(c.lib.bls_fav_job_submit_dev(c.h, job, idx, self.offs.ptr, self.cb, msgs, sigs, seed32))

    def job_partial(self, job: int) -> bytes:
        buf = ctypes.create_string_buffer(576)
        c = self.ctx
        c.check(c.lib.bls_fav_job_partial(c.h, job, buf))
        return buf.raw

    def job_check(self, job: int, partials: bytes) -> bool:
        c = self.ctx
        return c.check(c.lib.bls_fav_job_check(c.h, job, partials, len(partials) // 576)) == 1

    def job_check_own(self, job: int) -> bool:
        """The job's own product alone (bls_fav_job_check_own: the check submit enqueued behind it)."""
        c = self.ctx
        return c.check(c.lib.bls_fav_job_check_own(c.h, job)) == 1

    def job_finish(self, job: int, batch_ok: bool, chunk: int = 0) -> None:
        c = self.ctx
        lo = chunk * self.cb
        c.check(c.lib.bls_fav_job_finish_dev(c.h, job, 1 if batch_ok else 0, self.outs[job].ptr + lo))
        self.last_job = job
        self._chunk_job[chunk] = job

    def job_check_comm(self, job: int) -> bool:
        """RCCL all-gather of the job's device-resident partial + the product's final exponentiation
        (bls_fav_job_check_comm; the context's communicator must be initialised: dist.init_comm)."""
        c = self.ctx
        return c.check(c.lib.bls_fav_job_check_comm(c.h, job)) == 1

    def run_pipelined(self, seeds, exchange=None, depth: int = FAV_DEPTH, comm: bool = False) -> list:
        """One pass over the batch per seed (a pass = `chunks` jobs) with up to `depth` jobs in flight:
        job k+1.. are submitted before job k is final-exponentiated (their front kernels overlap job k's
        tail).  Multi-GPU: comm=True exchanges each job's partial inside the library over RCCL
        (bls_fav_job_check_comm); otherwise exchange(partial) -> concatenated partials of all ranks (a
        host-side all-gather, e.g. gloo in the CPU tests).  Every pass is complete (verdicts written) on
        return; returns one bool per pass (all of its chunks' batch checks passed)."""
        seeds = list(seeds)
        depth = max(1, min(depth, FAV_JOBS))
        units = [(k, ch) for k in range(len(seeds)) for ch in range(self.chunks)]
        oks = [True] * len(seeds)
        for u in range(min(depth, len(units))):
            k, ch = units[u]
            self.submit(u % FAV_JOBS, seeds[k], ch)
        for u, (k, ch) in enumerate(units):
            job = u % FAV_JOBS
            if comm:
                ok = self.job_check_comm(job)
            elif exchange is None:  # one shard: its own check, already enqueued behind its product
                ok = self.job_check_own(job)
            else:
                part = self.job_partial(job)
                ok = self.job_check(job, exchange(part))
            self.job_finish(job, ok, ch)
            oks[k] = oks[k] and ok
            if u + depth < len(units):
                k2, ch2 = units[u + depth]
                self.submit((u + depth) % FAV_JOBS, seeds[k2], ch2)
        self.ctx.check(self.ctx.lib.bls_sync(self.ctx.h))  # a failing job's bisection writes its verdicts async
        return oks

    def verdicts(self) -> np.ndarray:
        if self.chunks == 1:
            return self.outs[self.last_job].to_host().astype(bool)
        bufs = {j: self.outs[j].to_host() for j in set(self._chunk_job)}
        return np.concatenate([bufs[j][c * self.cb:(c + 1) * self.cb] for c, j in enumerate(self._chunk_job)]
                              ).astype(bool)

    def run(self) -> np.ndarray:
        if self.msg_ids is not None or self.committees is not None or self.keys is not None:
            self.run_pipelined([os.urandom(32)])
            return self.verdicts()
        ok = self.check_partials(self.partial())
        self.finish(ok)
        return self.verdicts()

    def aggregate_by_message(self, include=None, subgroup_check: bool = False) -> list:
        """The M per-message aggregates of a shared-message batch that has been run: entry m is the sum of the
        signatures of the items that sign table entry m and that the mask includes -- by default the batch's
        last verdicts, read where finish left them in HBM -- or None for a message with no included item (or a
        bad included signature).  bls_aggregate_grouped_dev on the batch's own signature buffer: nothing is
        uploaded again but the mask a caller supplies."""
        if self.msg_ids is None:
            raise ValueError("aggregate_by_message needs a shared-message batch (msg_ids)")
        c = self.ctx
        mask_buf = None
        if include is None:
            d_mask = self.outs[self.last_job].ptr
        else:
            _, _, mask = _group_args(self.msg_ids, self.M, include, self.B)
            mask_buf = DeviceBuffer(c, mask)
            d_mask = mask_buf.ptr
        out = DeviceBuffer(c, nbytes=97 * self.M)
        try:
            c.check(c.lib.bls_aggregate_grouped_dev(c.h, self.sigs.ptr, self.B, _ptr(self.msg_ids), self.M, d_mask,
                                                    1 if subgroup_check else 0, out.ptr, out.ptr + 96 * self.M))
            raw = out.to_host()
        finally:
            out.free()
            if mask_buf is not None:
                mask_buf.free()
        return _grouped_result(raw[: 96 * self.M], raw[96 * self.M:])

    def free(self):
        for b in (self.idx, self.offs, getattr(self, "bits", None), self.keys, self.msgs, self.sigs, *self.outs):
            if b is not None:
                b.free()


class Profiler:
    """hipEvent timing of each kernel of the FAV path (C-ABI bls_profile_*)."""

    def __init__(self, ctx=None):
        self.ctx = ctx or _native.context()

    def start(self):
        self.ctx.check(self.ctx.lib.bls_profile_enable(self.ctx.h, 1))

    def stop(self):
        self.ctx.check(self.ctx.lib.bls_profile_enable(self.ctx.h, 0))

    def read(self) -> dict:
        c = self.ctx
        ms = (ctypes.c_double * 16)()
        cnt = (ctypes.c_uint64 * 16)()
        n = c.check(c.lib.bls_profile_read(c.h, ms, cnt, 16))
        return {c.lib.bls_profile_name(i).decode(): (ms[i], int(cnt[i])) for i in range(n)}
