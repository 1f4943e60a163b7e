"""Host side of the committee-bitfield batches: the item expansion a wave runs and the lane combine base - S of the
gather (csrc/bls_g1_bits.h) in a host build with the digit form's column, value and subtraction checks compiled in
(tests/hostcheck_bits), against a numpy restatement and the Python oracle's G1 arithmetic; the Python argument
checks that precede any device call; and the sigsets routing, with fakes in place of the batch executors."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

from oracle import bls_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "hostcheck_bits")
LIB = os.path.join(DIR, "libhostcheck_bits.so")
INC = os.path.join(os.path.dirname(HERE), "eth-consensus-specs_amd", "csrc")

SIZES = [1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 511, 512, 513]
AUTO, DIRECT, COMPLEMENT = 0, 1, 2
F_COMPLEMENT, F_MALFORMED, F_SOME = 1, 2, 4
FILL = 0xDEADBEEF

P = O.P
MASK = 2 ** 29 - 1
RM = 2 ** 406
LD = 2 ** 29 + 2 ** 4  # the L-form digit bound of the accumulator contract

_lib = None


def lib():
    global _lib
    if _lib is None:
        deps = [os.path.join(DIR, f) for f in ("hostcheck_bits.cpp", "Makefile")]
        deps += [os.path.join(INC, f) for f in os.listdir(INC) if f.endswith(".h")]
        if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(d) for d in deps):
            subprocess.check_call(["make", "-C", DIR], timeout=2400)
        _lib = ctypes.CDLL(LIB)
        vp = ctypes.c_void_p
        _lib.hc_bits_expand.argtypes = [ctypes.c_int, vp, ctypes.c_uint64, vp, vp, vp, vp, ctypes.c_uint64,
                                        ctypes.c_uint64, vp, vp]
        _lib.hc_bits_expand.restype = None
        _lib.hc_bits_combine.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, vp, ctypes.c_uint64, ctypes.c_char_p,
                                         ctypes.c_size_t, ctypes.c_char_p, vp]
        _lib.hc_bits_combine.restype = None
    return _lib


# ---------------------------------------------------------------------------------------------- the expansion --
class Table:
    """one committee per size of SIZES, members = distinct registry indices in a shuffled order; committee 16 has
    a member that was bad at load (cstat 0)"""

    def __init__(self):
        rng = random.Random(0xB175)
        pool = list(range(5000))
        rng.shuffle(pool)
        self.lists, at = [], 0
        for s in SIZES + [40]:
            self.lists.append(pool[at: at + s])
            at += s
        self.idx = np.array([k for c in self.lists for k in c], dtype=np.uint32)
        self.offs = np.zeros(len(self.lists) + 1, dtype=np.uint64)
        np.cumsum([len(c) for c in self.lists], out=self.offs[1:])
        self.cstat = np.array([1] * len(SIZES) + [0], dtype=np.int32)


@pytest.fixture(scope="module")
def table():
    return Table()


def expand(table, comms, bitarr, mode, start=3, raw=None):
    """(len, flags, written list, untouched rest) of the host build for one item"""
    members = [k for c in comms for k in table.lists[c]]
    n = len(members)
    raw = np.packbits(np.asarray(bitarr, dtype=bool), bitorder="little") if raw is None else raw
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    assert raw.size == (n + 7) // 8
    buf = np.concatenate([raw, np.array([0xFF] * 8, dtype=np.uint8)])  # a read past the item's bytes would show
    ids = np.array(comms, dtype=np.uint32)
    out = np.full(start + n + 4, FILL, dtype=np.uint32)
    info = np.zeros(3, dtype=np.uint32)
    lib().hc_bits_expand(mode, ids.ctypes.data, len(comms), table.idx.ctypes.data, table.offs.ctypes.data,
                         table.cstat.ctypes.data, buf.ctypes.data, n, start, out.ctypes.data, info.ctypes.data)
    assert info[2] == 1
    ln = int(info[0])
    assert np.all(out[:start] == FILL) and np.all(out[start + ln:] == FILL)  # nothing outside the item's list
    return ln, int(info[1]), out[start: start + ln].tolist()


def restate(table, comms, bitarr, mode):
    """the numpy restatement: (len, flags, list)"""
    members = np.array([k for c in comms for k in table.lists[c]], dtype=np.uint32)
    bits = np.asarray(bitarr, dtype=bool)
    n, p, nc = members.size, int(bits.sum()), len(comms)
    if p == 0:
        return 0, 0, []
    ok = all(table.cstat[c] for c in comms)
    compl = ok and (mode == COMPLEMENT or (mode == AUTO and (n - p) + nc < p))
    want = members[~bits] if compl else members[bits]
    return want.size, F_SOME | (F_COMPLEMENT if compl else 0), want.tolist()


def patterns(n, rng):
    out = []
    for p in sorted({0, 1, n // 2, n - 1, n}):
        if 0 <= p <= n:
            b = np.zeros(n, dtype=bool)
            b[rng.sample(range(n), p)] = True
            out.append(b)
    return out


@pytest.mark.parametrize("mode", [AUTO, DIRECT, COMPLEMENT])
def test_expansion_single_committee(table, mode):
    rng = random.Random(mode)
    for c, n in enumerate(SIZES):
        for bits in patterns(n, rng):
            assert expand(table, [c], bits, mode) == restate(table, [c], bits, mode), (n, int(bits.sum()))


@pytest.mark.parametrize("mode", [AUTO, DIRECT, COMPLEMENT])
def test_expansion_multi_committee(table, mode):
    rng = random.Random(100 + mode)
    c65, c64, c1, c33 = SIZES.index(65), SIZES.index(64), SIZES.index(1), SIZES.index(33)
    for comms in ([c65, c64, c1], [c33, c33], [c1, c1, c1], [c64, 16], []):
        n = sum(len(table.lists[c]) for c in comms)
        for bits in patterns(n, rng):
            got = expand(table, comms, bits, mode)
            assert got == restate(table, comms, bits, mode), (comms, int(bits.sum()))
            if 16 in comms:  # a committee with a bad member at load: never the complement
                assert not got[1] & F_COMPLEMENT


def test_form_on_both_sides_of_the_rule(table):
    """auto takes the complement iff (n - p) + ncomm < p; direct never; complement always (cstat allowing)"""
    rng = random.Random(7)
    for comms in ([SIZES.index(64)], [SIZES.index(65), SIZES.index(64), SIZES.index(1)]):
        n, nc = sum(len(table.lists[c]) for c in comms), len(comms)
        edge = (n + nc) // 2 + 1  # the smallest p with (n - p) + nc < p
        assert (n - edge) + nc < edge and not (n - (edge - 1)) + nc < edge - 1
        for p, compl in ((edge - 1, False), (edge, True)):
            bits = np.zeros(n, dtype=bool)
            bits[rng.sample(range(n), p)] = True
            ln, flags, _ = expand(table, comms, bits, AUTO)
            assert bool(flags & F_COMPLEMENT) == compl and ln == (n - p if compl else p)
            assert expand(table, comms, bits, DIRECT)[:2] == (p, F_SOME)
            assert expand(table, comms, bits, COMPLEMENT)[:2] == (n - p, F_SOME | F_COMPLEMENT)


def test_padding_bit_is_malformed(table):
    for n in (1, 7, 9, 31, 33, 513):
        c = SIZES.index(n)
        bits = np.ones(n, dtype=bool)
        raw = np.packbits(bits, bitorder="little")
        for extra in range(n % 8, 8):
            bad = raw.copy()
            bad[-1] |= 1 << extra
            for mode in (AUTO, DIRECT, COMPLEMENT):
                assert expand(table, [c], bits, mode, raw=bad) == (0, F_MALFORMED, [])
    # a multiple of 8 has no padding
    c = SIZES.index(64)
    assert expand(table, [c], np.ones(64, dtype=bool), DIRECT)[1] == F_SOME


# --------------------------------------------------------------------------------------------- the lane combine --
def dig(v):
    return [(v >> (29 * i)) & MASK for i in range(13)] + [v >> 377]


def enc(a, k=0):
    """digits of the field element a: its Montgomery representative plus k p"""
    return dig(a * RM % P + k * P)


def val(d):
    return sum(x << (29 * i) for i, x in enumerate(d))


def worst(vbound, digit):
    """digits 0..12 all at `digit`, the top digit as large as a value below vbound p allows"""
    low = [digit] * 13
    d = low + [(vbound * P - 1 - val(low + [0])) >> 377]
    assert (vbound - 1) * P < val(d) < vbound * P
    return d


def poly_add(p, q):
    """the complete addition as polynomials (Renes-Costello-Batina, a = 0, b3 = 12)"""
    X1, Y1, Z1 = p
    X2, Y2, Z2 = q
    xy, yz, xz = X1 * Y2 + X2 * Y1, Y1 * Z2 + Y2 * Z1, X1 * Z2 + X2 * Z1
    m, s = Y1 * Y2 - 12 * Z1 * Z2, Y1 * Y2 + 12 * Z1 * Z2
    return ((xy * m - 12 * yz * xz) % P, (m * s + 36 * X1 * X2 * xz) % P, (s * yz + 3 * X1 * X2 * xy) % P)


def proj(aff, z=1):
    return (0, 1, 0) if aff is None else (aff[0] * z % P, aff[1] * z % P, z % P)


def combine(accs, flags, comm_ids, csum, L):
    """accs: L digit triples; csum: projective integer triples per table entry -> affine point or None"""
    flat = np.array([x for a in accs for c in a for x in c], dtype=np.uint32)
    ids = np.array(comm_ids, dtype=np.uint32)
    raw = b"".join(c.to_bytes(48, "big") for s in csum for c in s)
    out = ctypes.create_string_buffer(96)
    inf = ctypes.c_int(-1)
    lib().hc_bits_combine(flat.ctypes.data, L, flags, ids.ctypes.data, len(comm_ids), raw, len(csum), out,
                          ctypes.byref(inf))
    if inf.value:
        return None
    return int.from_bytes(out.raw[:48], "big"), int.from_bytes(out.raw[48:], "big")


def g1_sum(pts):
    acc = None
    for p in pts:
        acc = O.g1_add(acc, p)
    return acc


def g1_neg(p):
    return None if p is None else (p[0], (-p[1]) % P)


@pytest.fixture(scope="module")
def pool():
    rng = random.Random(0xC0B1)
    base = [O.g1_mul(O.G1_GEN, rng.randrange(1, O.R)) for _ in range(5)]
    pts = list(base)
    while len(pts) < 40:
        pts.append(O.g1_add(rng.choice(pts), rng.choice(base)))
    return pts


@pytest.mark.parametrize("L", [16, 64])
def test_lane_combine_matches_oracle(pool, L):
    """base - S over L lanes and the tree, with one, three and L + 3 committees (some lanes then add two sums, most
    none), against the oracle; and the direct form, which leaves the lanes' sums alone"""
    rng = random.Random(L)
    for ncomm in (1, 3, L + 3):
        lanes = [rng.choice(pool) if rng.random() < 0.7 else None for _ in range(L)]
        accs = [[enc(c) for c in proj(a, rng.randrange(1, P))] for a in lanes]
        sums = [rng.choice(pool) for _ in range(ncomm)]
        csum = [proj(s, rng.randrange(1, P)) for s in sums]
        ids = list(range(ncomm))
        rng.shuffle(ids)
        want = O.g1_add(g1_sum(sums), g1_neg(g1_sum(lanes)))
        assert combine(accs, F_SOME | F_COMPLEMENT, ids, csum, L) == want
        assert combine(accs, F_SOME, ids, csum, L) == g1_sum(lanes)


def test_lane_combine_degenerate(pool):
    L = 16
    ident = [enc(0), enc(1), enc(0)]
    a, b = pool[0], pool[1]
    one = [[enc(c) for c in proj(a, 5)]] + [ident] * (L - 1)
    # S the identity: the base comes back
    assert combine([ident] * L, F_SOME | F_COMPLEMENT, [0], [proj(b, 9)], L) == b
    # base the identity (a committee whose keys cancel, or an empty one): -S
    assert combine(one, F_SOME | F_COMPLEMENT, [0], [(0, 1, 0)], L) == g1_neg(a)
    assert combine(one, F_SOME | F_COMPLEMENT, [], [(0, 1, 0)], L) == g1_neg(a)
    # base == S: the identity
    assert combine(one, F_SOME | F_COMPLEMENT, [0], [proj(a, 3)], L) is None
    # the same committee twice: 2 base - S
    assert combine(one, F_SOME | F_COMPLEMENT, [0, 0], [proj(b, 1)], L) == O.g1_add(O.g1_add(b, b), g1_neg(a))


def test_lane_combine_at_the_top_of_the_contract(pool):
    """Accumulators at the top of the accumulator contract's redundant forms; a failed column, value or
    subtraction check aborts the host build.  On curve points, every lane's value as redundant as the contract
    allows (X + 65p, Y + 3p, Z + 3p) through 16 lanes and the tree; and one lane with every digit at the L-form
    bound 2^29 + 2^4 and the values just under 66p / 4p / 4p -- no curve point has such digits, and none is needed:
    the formulas are polynomial identities, so (X : -Y : Z) + q is checked against the polynomials."""
    L = 16
    rng = random.Random(3)
    lanes = [rng.choice(pool) for _ in range(L)]
    accs = [[enc(c, k) for c, k in zip(proj(a, rng.randrange(1, P)), (65, 3, 3))] for a in lanes]
    sums = [rng.choice(pool) for _ in range(L + 2)]
    csum = [proj(s, rng.randrange(1, P)) for s in sums]
    want = O.g1_add(g1_sum(sums), g1_neg(g1_sum(lanes)))
    assert combine(accs, F_SOME | F_COMPLEMENT, list(range(L + 2)), csum, L) == want
    rinv = pow(RM, -1, P)
    acc = [worst(66, LD), worst(4, LD), worst(4, LD)]
    x, y, z = (val(d) * rinv % P for d in acc)
    for q in ((rng.randrange(P), rng.randrange(P), rng.randrange(P)), (P - 1, P - 1, P - 1), (0, 1, 0)):
        X3, Y3, Z3 = poly_add((x, (-y) % P, z), q)
        zi = pow(Z3, -1, P)
        assert combine([acc], F_SOME | F_COMPLEMENT, [0], [q], 1) == (X3 * zi % P, Y3 * zi % P)


# --------------------------------------------------------------------------------- the Python argument checks --
class _NoDevice:
    """a context whose use fails the test: the argument checks must come first"""

    def __getattr__(self, name):
        raise AssertionError("device call before the argument check")


def _committees(sizes):
    from bls_mi355x import batch

    c = batch.Committees(ctx=_NoDevice())
    c.sizes = np.array(sizes, dtype=np.uint64)
    return c


def test_bad_arguments_rejected_before_any_device_call():
    from bls_mi355x import batch

    com = _committees([8, 9, 64])
    msgs, sigs = bytes(64), bytes(192)
    good = [bytes(1), bytes(2)]
    call = batch.fast_aggregate_verify_batch_bits
    with pytest.raises(ValueError):  # committee id >= C, negative, not an integer
        call(com, [0, 3], [bytes(1), bytes(1)], msgs, sigs)
    with pytest.raises(ValueError):
        call(com, [0, -1], good, msgs, sigs)
    with pytest.raises(ValueError):
        call(com, [0, 1.0], good, msgs, sigs)
    with pytest.raises(ValueError):  # wrong byte count: 9 members need 2 bytes; a list item needs the sum's
        call(com, [0, 1], [bytes(1), bytes(1)], msgs, sigs)
    with pytest.raises(ValueError):
        call(com, [0, [1, 2]], [bytes(1), bytes(9)], msgs, sigs)
    with pytest.raises(ValueError):  # a bool array of the wrong length
        call(com, [0, 1], [np.ones(8, dtype=bool), np.ones(8, dtype=bool)], msgs, sigs)
    with pytest.raises(ValueError):  # one bitfield short
        call(com, [0, 1], [bytes(1)], msgs, sigs)
    with pytest.raises(ValueError):  # bad msg_ids: out of range, one short, an empty table
        call(com, [0, 1], good, msgs, sigs, msg_ids=[0, 2])
    with pytest.raises(ValueError):
        call(com, [0, 1], good, msgs, sigs, msg_ids=[0])
    with pytest.raises(ValueError):
        call(com, [0, 1], good, None, sigs, msg_ids=[0, 0], table=b"")
    with pytest.raises(ValueError):  # messages and signatures, one per item; the mode's name
        call(com, [0, 1], good, bytes(32), sigs)
    with pytest.raises(ValueError):
        call(com, [0, 1], good, msgs, bytes(96))
    with pytest.raises(ValueError):
        call(com, [0, 1], good, msgs, sigs, mode="fast")
    with pytest.raises(ValueError):  # the pipelined form
        batch.ResidentFavBatch(None, None, msgs, sigs, committees=com, committee_ids=[0, 3], bits=good)
    with pytest.raises(ValueError):
        batch.ResidentFavBatch(None, None, msgs, sigs, committees=com, committee_ids=[0, 1], bits=good,
                               msg_ids=[0, 5])
    with pytest.raises(ValueError):
        batch.ResidentFavBatch(None, None, msgs, sigs, committees=com, committee_ids=[0, 1], bits=good, chunks=2,
                               msg_ids=[0, 1])
    with pytest.raises(ValueError):
        batch.ResidentFavBatch(None, None, bytes(96), bytes(288), committees=com, committee_ids=[0, 1, 2],
                               bits=[bytes(1), bytes(2), bytes(8)], chunks=2)
    with pytest.raises(ValueError):
        batch.ResidentFavBatch(None, None, msgs, sigs, committee_ids=[0, 1], bits=good, ctx=_NoDevice())


def test_bool_arrays_are_packed_in_ssz_order():
    from bls_mi355x import batch

    com = _committees([8, 9, 64])
    b9 = np.zeros(9, dtype=bool)
    b9[[0, 3, 8]] = True
    ids, co, raw, bo = batch._bits_args(com, [1, [0, 1]], [b9, bytes([0x81, 0x00, 0x01])], 2)
    assert ids.tolist() == [1, 0, 1] and co.tolist() == [0, 1, 3]
    assert raw.tobytes() == bytes([0x09, 0x01, 0x81, 0x00, 0x01]) and bo.tolist() == [0, 2, 5]


def test_bits_from_bitlist():
    from bls_mi355x import batch

    assert batch.bits_from_bitlist(bytes([0x01]), 0) == b""
    assert batch.bits_from_bitlist(bytes([0x0B]), 3) == bytes([0x03])
    assert batch.bits_from_bitlist(bytes([0xFF, 0x01]), 8) == bytes([0xFF])
    assert batch.bits_from_bitlist(bytes([0x55, 0x03]), 9) == bytes([0x55, 0x01])
    for raw, n in ((bytes([0xFF]), 8), (bytes([0x0B]), 2), (bytes([0x0B]), 4), (bytes([0x03, 0x00]), 9), (b"", 0)):
        with pytest.raises(ValueError):
            batch.bits_from_bitlist(raw, n)


# ---------------------------------------------------------------------------------------------- sigsets routing --
class FakeRegistry:
    def __init__(self, keys):
        self.map = {k: i for i, k in enumerate(keys)}

    def indices(self, pubkeys):
        try:
            return np.array([self.map[bytes(k)] for k in pubkeys], dtype=np.uint32)
        except KeyError:
            return None


def _pk(i):
    return bytes([0x80 | (i & 0x1f)]) + i.to_bytes(47, "big")


@pytest.fixture
def fakes(monkeypatch):
    from bls_mi355x import batch, sigsets

    calls = []

    def fav(idx, offs, msgs, sigs, ctx=None):
        calls.append(("fav", np.asarray(idx).tolist(), np.asarray(offs).tolist(), bytes(msgs), bytes(sigs)))
        return np.ones(len(offs) - 1, dtype=bool)

    def bits(committees, committee_ids, bitfields, msgs, sigs, msg_ids=None, table=None, mode="auto", ctx=None):
        calls.append(("bits", [np.asarray(c).tolist() for c in committee_ids], [bytes(b) for b in bitfields],
                      bytes(msgs), bytes(sigs), None if msg_ids is None else np.asarray(msg_ids).tolist(), mode))
        return np.array([True, False] * len(committee_ids), dtype=bool)[: len(committee_ids)]

    def av(pubkeys, messages, signatures, ctx=None):
        calls.append(("av", len(signatures)))
        return np.ones(len(signatures), dtype=bool)

    monkeypatch.setattr(batch, "fast_aggregate_verify_batch", fav)
    monkeypatch.setattr(batch, "fast_aggregate_verify_batch_bits", bits)
    monkeypatch.setattr(batch, "aggregate_verify_batch", av)
    return sigsets, calls


def test_sigsets_routes_bits_sets_through_the_bits_batch(fakes):
    sigsets, calls = fakes
    keys = [_pk(i) for i in range(4)]
    com = _committees([8, 9, 64])
    a, b = b"\x0a" * 32, b"\x0b" * 32
    s1, s2, s3, s4, s5 = (bytes([j]) * 96 for j in range(1, 6))
    for share in (False, True):
        calls.clear()
        s = sigsets.SignatureSets(FakeRegistry(keys), share_messages=share, committees=com)
        i0 = s.add_fast_aggregate_verify_bits(1, bytes([0xFF, 0x01]), a, s1)
        i1 = s.add_fast_aggregate_verify(keys[:2], b, s2)  # an indexed set keeps its route
        i2 = s.add_fast_aggregate_verify_bits([0, 1], np.ones(17, dtype=bool), b, s3)
        i3 = s.add_aggregate_verify([keys[2]], [b"long message"], s4)
        i4 = s.add_fast_aggregate_verify_bits(2, bytes(8), a, s5)
        bad = [s.add_fast_aggregate_verify_bits(3, bytes(1), a, s1),      # unknown committee
               s.add_fast_aggregate_verify_bits(1, bytes(1), a, s1),      # one byte short
               s.add_fast_aggregate_verify_bits(0, bytes(1), a[:31], s1),  # message, signature
               s.add_fast_aggregate_verify_bits(0, bytes(1), a, s1[:95])]
        out = s.verify()
        want_bits = ("bits", [[1], [0, 1], [2]], [bytes([0xFF, 0x01]), bytes([0xFF, 0xFF, 0x01]), bytes(8)],
                     (a + b) if share else (a + b + a), s1 + s3 + s5, [0, 1, 0] if share else None, "auto")
        assert calls == [("fav", [0, 1], [0, 2], b, s2), want_bits, ("av", 1)]
        # the fake's verdicts (True, False, True) land on the bits sets, in order; refused sets are False
        assert [out[i] for i in (i0, i2, i4)] == [True, False, True]
        assert out[i1] is True and out[i3] is True and all(out[i] is False for i in bad)


def test_sigsets_bits_need_a_table_and_distinct_messages_are_not_shared(fakes):
    sigsets, calls = fakes
    with pytest.raises(ValueError):
        sigsets.SignatureSets(FakeRegistry([])).add_fast_aggregate_verify_bits(0, bytes(1), bytes(32), bytes(96))
    com = _committees([8])
    s = sigsets.SignatureSets(None, share_messages=True, committees=com)
    s.add_fast_aggregate_verify_bits(0, bytes([1]), b"\x01" * 32, bytes(96))
    s.add_fast_aggregate_verify_bits(0, bytes([2]), b"\x02" * 32, bytes(96))
    s.verify()
    assert calls == [("bits", [[0], [0]], [bytes([1]), bytes([2])], b"\x01" * 32 + b"\x02" * 32, bytes(192), None,
                      "auto")]
    with sigsets.deferred(None, committees=com) as col:
        pass
    assert col.committees is com and col.results == []
