"""GPU tests of the committee-bitfield FAV batches (bls_committees_load, bls_fav_batch_committee_bits,
bls_fav_job_submit_bits_dev): items given as (committees, participation bits) over a device-resident
committee table, their aggregate key either the participants' sum or the committees' cached sums minus the
absentees'.  The defining property is checked throughout: the verdicts are those of the index-list entry points on
the expanded index list, in every mode; they are also known by construction.  Requires an MI355X."""
import hashlib

import numpy as np
import pytest

from oracle import bls_oracle as O

pytestmark = pytest.mark.gpu

N_REG = 1 << 14
G1_INF = b"\xc0" + bytes(47)
BAD_PK_0x40 = b"\x40" + bytes(47)
SIZES = [1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 511, 512, 513]
C_INVALID, C_RANGE = len(SIZES), len(SIZES) + 1  # committees holding index 1 (invalid) and index 2^14 (out of range)
MODES = ["auto", "direct", "complement"]


@pytest.fixture(scope="module")
def batch():
    from bls_mi355x import batch as b
    return b


def _lists():
    """one committee per size, distinct valid registry indices in a shuffled order, then the two 16-member
    committees with a bad member at position 5"""
    rng = np.random.default_rng(0xC0DE)
    pool = rng.permutation(np.arange(3, N_REG))
    lists, at = [], 0
    for s in SIZES + [16, 16]:
        lists.append(pool[at: at + s].astype(np.uint32))
        at += s
    lists[C_INVALID][5] = 1
    lists[C_RANGE][5] = N_REG
    return lists


class World:
    def __init__(self, batch):
        self.batch = batch
        self.reg = batch.Registry()
        self.lists = _lists()
        self.com = batch.Committees()
        self.load_registry()
        self.load_committees()

    def load_registry(self):
        """sk_i = i + 1 with G1 infinity at index 1 and a 0x40-flag encoding at index 2"""
        pks = bytearray(self.reg.generate(N_REG, first_sk=1, want_bytes=True))
        pks[48:96] = G1_INF
        pks[96:144] = BAD_PK_0x40
        valid = self.reg.load(bytes(pks))
        assert not valid[1] and not valid[2] and valid.sum() == N_REG - 2
        self.pks = bytes(pks)

    def load_committees(self):
        self.com.load(self.lists)
        assert len(self.com) == len(self.lists) and self.com.sizes.tolist() == [len(c) for c in self.lists]

    def members(self, comms):
        return np.concatenate([self.lists[c] for c in comms]) if len(comms) else np.zeros(0, np.uint32)

    def items(self, specs, seed, msg_ids=None, M=0):
        """specs: (committee list, bool bits) per item.  Each item's signature is sign_batch of its participants'
        summed secret keys (the valid ones: a bad participant has no secret) on its message.  Returns the expanded
        (idx, offs), the messages (per item, or the table) and the signatures."""
        B = len(specs)
        table = [hashlib.sha256(b"bits" + seed.to_bytes(8, "little") + m.to_bytes(8, "little")).digest()
                 for m in range(M if msg_ids is not None else B)]
        exp = [self.members(c)[np.asarray(b, dtype=bool)] for c, b in specs]
        agg = []
        for e in exp:
            good = e[(e >= 3) & (e < N_REG)].astype(np.int64)
            agg.append(int((good + 1).sum()) % O.R or 1)  # no participant: any signature, the verdict is False
        mids = msg_ids if msg_ids is not None else range(B)
        sigs = self.batch.sign_batch(b"".join(a.to_bytes(32, "big") for a in agg), b"".join(table[m] for m in mids))
        idx = np.concatenate(exp).astype(np.uint32) if exp else np.zeros(0, np.uint32)
        offs = self.batch.offsets_from_lengths([e.size for e in exp])
        return idx, offs, b"".join(table), bytearray(sigs)

    def bits_call(self, specs, msgs, sigs, mode="auto", msg_ids=None):
        return self.batch.fast_aggregate_verify_batch_bits(self.com, [c for c, _ in specs], [b for _, b in specs],
                                                           msgs, bytes(sigs), msg_ids=msg_ids, mode=mode)


@pytest.fixture(scope="module")
def world(batch):
    return World(batch)


def _bits(n, p, rng):
    b = np.zeros(n, dtype=bool)
    b[rng.choice(n, size=p, replace=False)] = True
    return b


def test_parity_all_sizes_all_modes(batch, world):
    """Every committee size with p in {0, 1, n/2, n - 1, n} and one random p, in the three modes: the verdicts of
    the indexed call on the expanded indices, which are False exactly at p = 0; without the p = 0 items the batch
    passes whole (no fallback work)."""
    rng = np.random.default_rng(1)
    specs = []
    for c, n in enumerate(SIZES):
        for p in sorted({0, 1, n // 2, n - 1, n}) + [int(rng.integers(0, n + 1))]:
            specs.append(([c], _bits(n, p, rng)))
    idx, offs, msgs, sigs = world.items(specs, 1)
    truth = np.array([b.any() for _, b in specs])
    ref = batch.fast_aggregate_verify_batch(idx, offs, msgs, bytes(sigs))
    assert (ref == truth).all(), np.nonzero(ref != truth)
    for mode in MODES:
        out = world.bits_call(specs, msgs, sigs, mode)
        assert (out == ref).all(), (mode, np.nonzero(out != ref))
    keep = [j for j in range(len(specs)) if truth[j]]
    sub = [specs[j] for j in keep]
    for mode in MODES:
        out = world.bits_call(sub, b"".join(msgs[32 * j: 32 * j + 32] for j in keep),
                              b"".join(bytes(sigs[96 * j: 96 * j + 96]) for j in keep), mode)
        assert out.all() and batch.fallback_stats() == (0, 0), mode


def test_the_complement_form_really_runs(batch, world):
    """64 items of n = 512: with p = 511 auto adds one absentee and one committee sum per item where direct adds
    511 keys; at p = 256 auto stays direct."""
    rng = np.random.default_rng(2)
    c512 = SIZES.index(512)
    specs = [([c512], _bits(512, 511, rng)) for _ in range(64)]
    _, _, msgs, sigs = world.items(specs, 2)
    assert world.bits_call(specs, msgs, sigs, "auto").all()
    assert batch.gather_work() == (64 * 2, 64)
    assert world.bits_call(specs, msgs, sigs, "direct").all()
    assert batch.gather_work() == (64 * 511, 0)
    half = [([c512], _bits(512, 256, rng)) for _ in range(64)]
    _, _, msgs, sigs = world.items(half, 3)
    assert world.bits_call(half, msgs, sigs, "auto").all()
    assert batch.gather_work() == (64 * 256, 0)
    assert world.bits_call(half, msgs, sigs, "complement").all()
    assert batch.gather_work() == (64 * 257, 64)


def test_invalid_and_out_of_range_members(batch, world):
    """A committee with an invalid registry entry, and one with an index past the registry: as a non-participant
    the bad member does not matter (FastAggregateVerify never sees it) and the item never takes the complement;
    as a participant the item is False.  Both as the indexed call says."""
    specs = []
    for c in (C_INVALID, C_RANGE):
        absent = np.ones(16, dtype=bool)
        absent[5] = False
        only = np.zeros(16, dtype=bool)
        only[[5, 6]] = True
        specs += [([c], absent), ([c], np.ones(16, dtype=bool)), ([c], only)]
    idx, offs, msgs, sigs = world.items(specs, 4)
    ref = batch.fast_aggregate_verify_batch(idx, offs, msgs, bytes(sigs))
    assert ref.tolist() == [True, False, False] * 2
    for mode in MODES:
        out = world.bits_call(specs, msgs, sigs, mode)
        assert (out == ref).all(), mode
        pts, compl = batch.gather_work()
        assert compl == 0 and pts == 2 * (15 + 16 + 2), mode


def test_soundness_at_the_bit_level(batch, world):
    """Complement-form items (p >= n - 2): a bit claimed for a key that did not sign, a signer's bit cleared, and
    a wrong-message forgery are each False, isolated by the bisection; every other item stays True."""
    rng = np.random.default_rng(5)
    c64 = SIZES.index(64)
    specs = [([c64], _bits(64, int(rng.integers(62, 65)), rng)) for _ in range(40)]
    for j in (3, 17):
        specs[j] = ([c64], _bits(64, 62, rng))
    idx, offs, msgs, sigs = world.items(specs, 5)
    assert world.bits_call(specs, msgs, sigs, "auto").all()
    assert batch.gather_work()[1] == 40 and batch.fallback_stats() == (0, 0)
    claimed = specs[3][1].copy()
    claimed[np.nonzero(~claimed)[0][0]] = True  # the signature lacks this key
    cleared = specs[17][1].copy()
    cleared[np.nonzero(cleared)[0][0]] = False  # the signature holds this key
    bad = list(specs)
    bad[3], bad[17] = ([c64], claimed), ([c64], cleared)
    wrong = bytearray(sigs)
    wrong[96 * 29: 96 * 30] = sigs[96 * 30: 96 * 31]  # a valid signature, of another item's keys and message
    for mode in ("auto", "complement"):
        out = world.bits_call(bad, msgs, wrong, mode)
        assert np.nonzero(~out)[0].tolist() == [3, 17, 29], mode
        checks, rounds = batch.fallback_stats()
        assert checks > 0 and rounds > 0
    exp = [world.members(c)[b] for c, b in bad]
    ref = batch.fast_aggregate_verify_batch(np.concatenate(exp), batch.offsets_from_lengths([e.size for e in exp]),
                                            msgs, bytes(wrong))
    assert np.nonzero(~ref)[0].tolist() == [3, 17, 29]


def test_multi_committee_items(batch, world):
    """Items over 65 + 64 + 1 members and over one committee listed twice (its keys count twice), against the
    indexed call, in every mode; the nearly full ones take the complement with three (two) committee sums."""
    rng = np.random.default_rng(6)
    three = [SIZES.index(65), SIZES.index(64), SIZES.index(1)]
    twice = [SIZES.index(33), SIZES.index(33)]
    specs = []
    for comms, n in ((three, 130), (twice, 66)):
        for p in (1, n // 2, n - 1, n):
            specs.append((comms, _bits(n, p, rng)))
    idx, offs, msgs, sigs = world.items(specs, 6)
    ref = batch.fast_aggregate_verify_batch(idx, offs, msgs, bytes(sigs))
    assert ref.all()
    for mode in MODES:
        assert world.bits_call(specs, msgs, sigs, mode).all(), mode
    world.bits_call(specs, msgs, sigs, "auto")
    # auto: complement at p = n - 1 and n only -- (n - p) + ncomm additions
    assert batch.gather_work() == ((1 + 65 + 4 + 3) + (1 + 33 + 3 + 2), 4)


def test_padding_bit_fails_its_item_only(batch, world):
    rng = np.random.default_rng(7)
    c9, c33 = SIZES.index(9), SIZES.index(33)
    specs = [([c9], _bits(9, 9, rng)), ([c33], _bits(33, 33, rng)), ([c9], _bits(9, 5, rng)), ([c33], _bits(33, 32, rng))]
    _, _, msgs, sigs = world.items(specs, 7)
    raw = [np.packbits(b, bitorder="little").tobytes() for _, b in specs]
    assert world.bits_call([(c, r) for (c, _), r in zip(specs, raw)], msgs, sigs).all()
    raw[0] = raw[0][:-1] + bytes([raw[0][-1] | 0x80])
    raw[3] = raw[3][:-1] + bytes([raw[3][-1] | 0x02])
    for mode in MODES:
        out = world.bits_call([(c, r) for (c, _), r in zip(specs, raw)], msgs, sigs, mode)
        assert out.tolist() == [False, True, True, False], mode


def test_with_msg_ids(batch, world):
    """200 items on 3 messages: the verdicts of the shared indexed call on the expanded indices, one hash and one
    Miller pair per message."""
    rng = np.random.default_rng(8)
    c32 = SIZES.index(32)
    specs = [([c32], _bits(32, int(rng.integers(1, 33)), rng)) for _ in range(200)]
    ids = rng.integers(0, 3, size=200).astype(np.uint32)
    idx, offs, table, sigs = world.items(specs, 8, msg_ids=ids, M=3)
    sigs[96 * 50: 96 * 51] = sigs[96 * 51: 96 * 52]
    out = world.bits_call(specs, table, sigs, "auto", msg_ids=ids)
    assert batch.batch_work() == (3, 67)
    ref = batch.fast_aggregate_verify_batch_shared(idx, offs, table, ids, bytes(sigs))
    assert (out == ref).all() and np.nonzero(~out)[0].tolist() == [50]


def test_resident_batch_in_chunks_and_aggregate_by_message(batch, world):
    """ResidentFavBatch with bits: two chunks through run_pipelined give the host call's verdicts; with msg_ids,
    aggregate_by_message gives aggregate_grouped's aggregates of the verified signatures."""
    rng = np.random.default_rng(9)
    sizes = [SIZES.index(s) for s in (9, 64, 129)]
    specs = []
    for j in range(24):
        c = sizes[j % 3]
        n = SIZES[c]
        specs.append(([c], _bits(n, n - (j % 2), rng)))
    _, _, msgs, sigs = world.items(specs, 9)
    sigs[96 * 20: 96 * 21] = sigs[96 * 2: 96 * 3]
    want = world.bits_call(specs, msgs, sigs)
    assert np.nonzero(~want)[0].tolist() == [20]
    rb = batch.ResidentFavBatch(None, None, msgs, bytes(sigs), committees=world.com,
                                committee_ids=[c for c, _ in specs], bits=[b for _, b in specs], chunks=2)
    try:
        assert rb.run_pipelined([bytes(range(32))]) == [False]
        assert (rb.verdicts() == want).all()
        assert (rb.run() == want).all()
    finally:
        rb.free()
    ids = (np.arange(24) % 4).astype(np.uint32)
    _, _, table, sigs = world.items(specs, 10, msg_ids=ids, M=4)
    sigs[96 * 5: 96 * 6] = sigs[96 * 9: 96 * 10]  # same message (5 % 4 == 9 % 4), other keys
    rb = batch.ResidentFavBatch(None, None, table, bytes(sigs), committees=world.com,
                                committee_ids=[c for c, _ in specs], bits=[b for _, b in specs], msg_ids=ids)
    try:
        v = rb.run()
        assert np.nonzero(~v)[0].tolist() == [5]
        assert batch.batch_work() == (4, 68)
        assert rb.aggregate_by_message() == batch.aggregate_grouped(bytes(sigs), ids, 4, include=v,
                                                                    subgroup_check=False)
    finally:
        rb.free()


def test_sigsets_mixed_collector(batch, world):
    """bits sets, an indexed set and an AggregateVerify set in one collector with a committees table, with and
    without share_messages: every verdict equals the per-call one."""
    from bls_mi355x import sigsets
    from bls_mi355x.backend import mi355x_bls

    rng = np.random.default_rng(11)
    c9, c64 = SIZES.index(9), SIZES.index(64)
    specs = [([c9], _bits(9, 9, rng)), ([c64], _bits(64, 63, rng)), ([c9, c64], _bits(73, 70, rng)),
             ([c64], _bits(64, 40, rng))]
    ids = np.array([0, 1, 0, 1], dtype=np.uint32)
    idx, offs, table, sigs = world.items(specs, 11, msg_ids=ids, M=2)
    sigs[96 * 3: 96 * 4] = sigs[96: 192]  # set 3 invalid: set 1's signature (same message)
    pk = lambda k: world.pks[48 * int(k): 48 * int(k) + 48]  # noqa: E731
    m2 = [hashlib.sha256(b"av" + bytes([j])).digest() for j in range(2)]
    av_sig = mi355x_bls.Aggregate([batch.sign_batch((11).to_bytes(32, "big"), m2[0]),
                                   batch.sign_batch((12).to_bytes(32, "big"), m2[1])])
    ix = np.array([20, 21, 22], dtype=np.uint32)
    ix_sig = batch.sign_batch((21 + 22 + 23).to_bytes(32, "big"), table[:32])
    percall = [mi355x_bls.FastAggregateVerify([pk(k) for k in idx[int(offs[j]): int(offs[j + 1])]],
                                              table[32 * ids[j]: 32 * ids[j] + 32], bytes(sigs[96 * j: 96 * j + 96]))
               for j in range(4)]
    percall += [mi355x_bls.FastAggregateVerify([pk(k) for k in ix], table[:32], ix_sig),
                mi355x_bls.AggregateVerify([pk(10), pk(11)], m2, av_sig)]
    assert percall == [True, True, True, False, True, True]
    for share in (False, True):
        s = sigsets.SignatureSets(world.reg, share_messages=share, committees=world.com)
        for j, (c, b) in enumerate(specs):
            s.add_fast_aggregate_verify_bits(c, b, table[32 * ids[j]: 32 * ids[j] + 32], bytes(sigs[96 * j: 96 * j + 96]))
        s.add_fast_aggregate_verify_indexed(ix, table[:32], ix_sig)
        s.add_aggregate_verify([pk(10), pk(11)], m2, av_sig)
        assert s.verify() == percall, share


def test_sixteen_lane_forms(batch, world):
    """From 1,024 items (and 1,024 committees at load) the gather runs 16 lanes per item, four items per wave:
    1,027 committees of 1, 5 and 17 members and one item on each -- not a multiple of four -- against the indexed
    call, in every mode."""
    rng = np.random.default_rng(13)
    C = 1027
    saved = world.lists
    world.lists = [rng.choice(np.arange(3, N_REG), size=(1, 5, 17)[c % 3], replace=False).astype(np.uint32)
                   for c in range(C)]
    try:
        world.load_committees()
        specs = []
        for c in range(C):
            n = world.lists[c].size
            specs.append(([c], _bits(n, n if c % 2 else int(rng.integers(1, n + 1)), rng)))
        idx, offs, msgs, sigs = world.items(specs, 13)
        sigs[96 * 1026: 96 * 1027] = sigs[96 * 1025: 96 * 1026]
        ref = batch.fast_aggregate_verify_batch(idx, offs, msgs, bytes(sigs))
        assert np.nonzero(~ref)[0].tolist() == [1026]
        for mode in MODES:
            out = world.bits_call(specs, msgs, sigs, mode)
            assert (out == ref).all(), (mode, np.nonzero(out != ref))
        assert batch.gather_work()[1] == C
    finally:
        world.lists = saved
        world.load_committees()


def test_table_lifetime(batch, world):
    """The table survives registry.append, is refused after registry.generate (its sums belong to the replaced
    keys) and works again once loaded again."""
    from bls_mi355x import _native

    rng = np.random.default_rng(12)
    c65 = SIZES.index(65)
    specs = [([c65], _bits(65, 64, rng)), ([c65], _bits(65, 3, rng)), ([C_RANGE], np.ones(16, dtype=bool))]
    idx, offs, msgs, sigs = world.items(specs, 12)
    assert world.bits_call(specs, msgs, sigs).tolist() == [True, True, False]
    try:
        world.reg.append(O.SkToPk(N_REG + 1))  # index 2^14 now exists: the indexed call sees it, cstat stays 0
        ref = batch.fast_aggregate_verify_batch(idx, offs, msgs, bytes(sigs))
        out = world.bits_call(specs, msgs, sigs, "complement")
        assert (out == ref).all() and batch.gather_work()[1] == 2
        world.reg.generate(64)
        with pytest.raises(_native.NativeError, match="stale"):
            world.bits_call(specs, msgs, sigs)
    finally:
        world.load_registry()
    with pytest.raises(_native.NativeError, match="stale"):  # a reloaded registry is another generation too
        world.bits_call(specs, msgs, sigs)
    world.load_committees()
    assert world.bits_call(specs, msgs, sigs).tolist() == [True, True, False]


def test_identity_sums(batch):
    """Its own registry {pk, -pk, pk'}: the committee {pk, -pk} sums to the identity and is still usable.  All
    bits set is the identity aggregate, False in every mode; one bit set in the complement form is
    identity - (-pk) = pk and verifies pk's signature.  (Last: it replaces the module's registry.)"""
    pk5, pk7 = O.SkToPk(5), O.SkToPk(7)
    neg5 = bytes([pk5[0] ^ 0x20]) + pk5[1:]
    reg = batch.Registry()
    assert reg.load(pk5 + neg5 + pk7).all()
    com = batch.Committees().load([[0, 1], [0, 1, 2], []])
    msgs = [hashlib.sha256(bytes([j])).digest() for j in range(4)]
    sig5 = [batch.sign_batch((5).to_bytes(32, "big"), m) for m in msgs]
    sig7 = batch.sign_batch((7).to_bytes(32, "big"), msgs[2])
    ids = [0, 0, 1, 2]
    bits = [bytes([0x03]), bytes([0x01]), bytes([0x07]), b""]
    sigs = sig5[0] + sig5[1] + sig7 + sig5[3]
    for mode in MODES:
        out = batch.fast_aggregate_verify_batch_bits(com, ids, bits, b"".join(msgs), sigs, mode=mode)
        # {pk, -pk} whole: the identity; pk alone; {pk, -pk, pk'} whole = pk'; the empty committee
        assert out.tolist() == [False, True, True, False], mode
        if mode == "complement":
            assert batch.gather_work() == (1 + 2 + 1, 3)
