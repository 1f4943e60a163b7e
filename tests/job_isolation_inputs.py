"""Inputs and expected values of the job-isolation tests (test_job_isolation_cpu.py, test_gpu_job_isolation.py): the
FAV batches that are left pending on a job between their submit and their finish, and the calls that are made on the
same context meanwhile.  Plain Python: every expected value follows from how the input was built (secret keys
sk_i = i + 1, so sums of keys and of signatures have known discrete logarithms) or comes from the C oracle, and
test_job_isolation_cpu.py checks each against the oracle's own verdict.

The builders do not use test_gpu_parity._synthetic: it signs on the device, and the CPU test needs the same inputs.

  pending(form, variant)   the batch of B = 10 items of 8 keys over a registry of 128 keys in one of the four resident
                           forms ResidentFavBatch takes; variant "bad3" (item 3 carries item 4's signature), "good",
                           or "bad6" (the batches the replacing host-buffer calls bring)
  CALLS                    name -> Call: one small call each, at the smallest size that reaches its kernel route
  REPLACING                the four host-buffer batch forms, which replace job 0's batch
"""
import functools
import hashlib
import random

import numpy as np

import cell_inputs as CI
import g1_table_edge_inputs as E
import kzg_inputs as K
from oracle import bls_oracle as O
from oracle import bls_oracle_c as OC

N_REG, B, N_KEYS, M_SHARED = 128, 10, 8, 4
N_COMM = N_REG // N_KEYS  # the committee table: committee c = keys 8 c .. 8 c + 7
FORMS = ("indexed", "shared", "bits", "keys")
BAD = {"bad3": 3, "bad6": 6, "good": None}
SEED = b"\x09" * 32
GT_ONE = bytes(47) + b"\x01" + bytes(528)  # Fp12 one as bls_multi_pairing writes it (include/blsmi355x.h)


def sk32(k: int) -> bytes:
    return int(k).to_bytes(32, "big")


def _msg(tag: bytes, j: int) -> bytes:
    return hashlib.sha256(b"job-isolation" + tag + j.to_bytes(4, "little")).digest()


@functools.lru_cache(maxsize=None)
def pubkeys() -> tuple:
    """the registry: key i belongs to sk = i + 1"""
    return tuple(OC.SkToPk(i + 1) for i in range(N_REG))


def committee_lists() -> list:
    return [list(range(N_KEYS * c, N_KEYS * c + N_KEYS)) for c in range(N_COMM)]


class Pending:
    """One batch.  members[j]: the registry indices whose keys sign item j; item_msgs[j]: its message; expect[j]: its
    verdict, from how the signatures were built."""

    def __init__(self, form: str, variant: str):
        assert form in FORMS and variant in BAD
        self.form, self.variant = form, variant
        # "good" is "bad3" without the swapped signature; "bad6" has keys and messages of its own
        tag = ("%s/%s" % (form, "replacing" if variant == "bad6" else "pending")).encode()
        rng = random.Random(tag)
        self.committee_ids = self.bits = self.msg_ids = None
        if form == "bits":
            # item 0 is a full committee and item 1 misses one member (complement mode under "auto": fewer
            # absentees than participants), item 2 has a single participant, item 5 spans two committees
            self.committee_ids = [[j] for j in range(B)]
            self.committee_ids[5] = [5, N_COMM - 1]
            self.bits, self.members = [], []
            for j, ids in enumerate(self.committee_ids):
                pool = [k for c in ids for k in committee_lists()[c]]
                n_set = {0: len(pool), 1: len(pool) - 1, 2: 1}.get(j, rng.randrange(3, len(pool) - 1))
                on = set(rng.sample(range(len(pool)), n_set))
                self.bits.append(np.array([i in on for i in range(len(pool))], dtype=bool))
                self.members.append([pool[i] for i in sorted(on)])
        else:
            self.members = [rng.sample(range(N_REG), N_KEYS) for _ in range(B)]
        if form == "shared":
            self.table = [_msg(tag, m) for m in range(M_SHARED)]
            self.msg_ids = [j % M_SHARED for j in range(B)]
            self.item_msgs = [self.table[m] for m in self.msg_ids]
        else:
            self.table = self.item_msgs = [_msg(tag, j) for j in range(B)]
        sigs = [OC.Sign(sum(k + 1 for k in mem) % O.R, m) for mem, m in zip(self.members, self.item_msgs)]
        self.expect = [1] * B
        bad = BAD[variant]
        if bad is not None:
            # the next item's signature: other keys, and another message (ids 3 / 0 and 2 / 3 in the shared form)
            assert self.members[bad] != self.members[bad + 1] and self.item_msgs[bad] != self.item_msgs[bad + 1]
            sigs[bad] = sigs[bad + 1]
            self.expect[bad] = 0
        self.sigs = b"".join(sigs)
        self.idx = np.array([k for mem in self.members for k in mem], dtype=np.uint32)
        self.offs = np.concatenate([[0], np.cumsum([len(mem) for mem in self.members])]).astype(np.uint64)

    def item(self, j: int):
        """(keys, message, signature) of item j, the arguments of the oracle's FastAggregateVerify"""
        return [pubkeys()[k] for k in self.members[j]], self.item_msgs[j], self.sigs[96 * j: 96 * j + 96]

    def key_lists(self) -> list:
        return [[pubkeys()[k] for k in mem] for mem in self.members]

    def resident(self, batch, ctx, committees=None):
        """the batch in HBM (batch.ResidentFavBatch) in its form"""
        msgs = b"".join(self.table)
        if self.form == "bits":
            return batch.ResidentFavBatch(None, None, msgs, self.sigs, ctx=ctx, committees=committees,
                                          committee_ids=self.committee_ids, bits=self.bits)
        if self.form == "keys":
            table, idx, offs = batch.key_table(self.key_lists())
            return batch.ResidentFavBatch(idx, offs, msgs, self.sigs, ctx=ctx, keys=table)
        return batch.ResidentFavBatch(self.idx, self.offs, msgs, self.sigs, ctx=ctx, msg_ids=self.msg_ids)

    def host_call(self, batch, ctx, committees=None) -> list:
        """the same batch through its host-buffer entry point, which prepares it on job 0: its verdicts"""
        msgs = b"".join(self.table)
        if self.form == "indexed":
            v = batch.fast_aggregate_verify_batch(self.idx, self.offs, msgs, self.sigs, ctx=ctx)
        elif self.form == "shared":
            v = batch.fast_aggregate_verify_batch_shared(self.idx, self.offs, msgs, self.msg_ids, self.sigs, ctx=ctx)
        elif self.form == "keys":
            table, idx, offs = batch.key_table(self.key_lists())
            v = batch.fast_aggregate_verify_batch_keys(table, idx, offs, msgs, self.sigs, ctx=ctx)
        else:
            v = batch.fast_aggregate_verify_batch_bits(committees, self.committee_ids, self.bits, msgs, self.sigs,
                                                       ctx=ctx)
        return [int(x) for x in v]


@functools.lru_cache(maxsize=None)
def pending(form: str, variant: str) -> Pending:
    return Pending(form, variant)


# ---- the interleaved calls ------------------------------------------------------------------------------------------
class Call:
    """args(): the call's inputs (built once); want(args): its expected result, by construction; oracle(args): the same
    from the oracle, independently (the CPU test compares the two); run(env, args): the call itself on env.ctx -- env
    carries the modules and the context's resident objects (test_gpu_job_isolation.Env)."""

    def __init__(self, name, args, want, oracle, run):
        self.name, self._want, self._oracle, self._run = name, want, oracle, run
        self._args = functools.lru_cache(maxsize=None)(args)

    def args(self):
        return self._args()

    def want(self):
        return self._want(*self.args())

    def oracle(self):
        return self._oracle(*self.args())

    def __call__(self, env):
        """(the call's result, the expected result)"""
        return self._run(env, *self.args()), self.want()


CALLS = {}


def _call(name, args, want, oracle):
    def deco(run):
        CALLS[name] = Call(name, args, want, oracle, run)
        return run
    return deco


M0 = _msg(b"call", 0)


def _sig(sk: int, m: bytes = M0) -> bytes:
    return OC.Sign(sk, m)


# per-call verification: Verify and FastAggregateVerify keep their Miller values in S_F; AggregateVerify leaves its
# product in S_FPART
@_call("verify", lambda: (OC.SkToPk(7), M0, _sig(7)), lambda *a: True, OC.Verify)
def _(env, pk, m, sig):
    return env.shim.Verify(pk, m, sig)


@_call("verify_failing", lambda: (OC.SkToPk(7), M0, _sig(7, _msg(b"call", 1))), lambda *a: False, OC.Verify)
def _(env, pk, m, sig):
    return env.shim.Verify(pk, m, sig)


@_call("fast_aggregate_verify", lambda: ([OC.SkToPk(5), OC.SkToPk(6)], M0, _sig(11)), lambda *a: True,
       OC.FastAggregateVerify)
def _(env, pks, m, sig):
    return env.shim.FastAggregateVerify(pks, m, sig)


def _av_args():
    sks = (2, 3, 4)
    msgs = [_msg(b"av", k) for k in sks]
    return [OC.SkToPk(k) for k in sks], msgs, OC.Aggregate([_sig(k, m) for k, m in zip(sks, msgs)])


@_call("aggregate_verify", _av_args, lambda *a: True, OC.AggregateVerify)
def _(env, pks, msgs, sig):
    return env.shim.AggregateVerify(pks, msgs, sig)


def _avb_args():
    pks = [[OC.SkToPk(2), OC.SkToPk(3)], [OC.SkToPk(4), OC.SkToPk(5)]]
    msgs = [[_msg(b"avb", 0), _msg(b"avb", 1)], [_msg(b"avb", 2), _msg(b"avb", 3)]]
    good = OC.Aggregate([_sig(2, msgs[0][0]), _sig(3, msgs[0][1])])
    return pks, msgs, [good, good]  # item 1 carries item 0's signature: the batch check fails, the items are re-checked


@_call("aggregate_verify_batch", _avb_args, lambda *a: [True, False],
       lambda pks, msgs, sigs: [OC.AggregateVerify(p, m, s) for p, m, s in zip(pks, msgs, sigs)])
def _(env, pks, msgs, sigs):
    return [bool(v) for v in env.batch.aggregate_verify_batch(pks, msgs, sigs, ctx=env.ctx)]


# pairings: e(P, Q) e(-P, Q) = 1, e(P, Q)^2 != 1
def _cancel():
    p, q = OC.SkToPk(5), _sig(9)
    return [(p, q), (E.neg48(p), q)],


def _twice():
    p, q = OC.SkToPk(5), _sig(9)
    return [(p, q), (p, q)],


@functools.lru_cache(maxsize=None)
def _product_is_one(pairs) -> bool:
    return O.pairing_product_is_one([(O.g1_decompress(p), O.g2_decompress(q)) for p, q in pairs])


def oracle_product_is_one(pairs) -> bool:
    return _product_is_one(tuple(pairs))


@_call("pairing_check", _cancel, lambda pairs: True, oracle_product_is_one)
def _(env, pairs):
    return env.batch.pairing_check(pairs, ctx=env.ctx)


@_call("pairing_check_failing", _twice, lambda pairs: False, oracle_product_is_one)
def _(env, pairs):
    return env.batch.pairing_check(pairs, ctx=env.ctx)


@_call("pairing_check_ex", _twice, lambda pairs: False, oracle_product_is_one)
def _(env, pairs):
    return env.curve.pairing_product_is_one([p for p, _ in pairs], [q for _, q in pairs])


# the last of the calls that leave a product in S_FPART, and a passing one: what a sequence of all calls leaves there
@_call("multi_pairing", _cancel, lambda pairs: GT_ONE, lambda pairs: GT_ONE if oracle_product_is_one(pairs) else None)
def _(env, pairs):
    g1 = [env.curve.G1Point.from_compressed_bytes(p) for p, _ in pairs]
    g2 = [env.curve.G2Point.from_compressed_bytes(q) for _, q in pairs]
    return env.curve.GT.multi_pairing(g1, g2).to_bytes()


# key and signature calls: sums of keys sk G1 and of signatures sk H(m) are the key and the signature of the sum
def _g1(k: int):
    return O.g1_mul(O.G1_GEN, k)


@_call("g1_multi_exp", lambda: ([OC.SkToPk(1), OC.SkToPk(2)], [3, 5]), lambda pts, ks: OC.SkToPk(13),
       lambda pts, ks: O.g1_compress(O.g1_add(O.g1_mul(O.g1_decompress(pts[0]), ks[0]),
                                              O.g1_mul(O.g1_decompress(pts[1]), ks[1]))))
def _(env, pts, ks):
    return env.batch.g1_multi_exp(pts, ks, ctx=env.ctx)


@_call("aggregate_pks", lambda: ([OC.SkToPk(5), OC.SkToPk(6)],), lambda pks: OC.SkToPk(11), OC.AggregatePKs)
def _(env, pks):
    return bytes(env.shim.AggregatePKs(pks))


@_call("aggregate", lambda: ([_sig(5), _sig(6)],), lambda sigs: _sig(11), OC.Aggregate)
def _(env, sigs):
    return bytes(env.shim.Aggregate(sigs))


@_call("key_validate", lambda: (OC.SkToPk(9),), lambda pk: True, OC.KeyValidate)
def _(env, pk):
    return env.shim.KeyValidate(pk)


@_call("sign_batch", lambda: ([3, 4], [_msg(b"sign", 0), _msg(b"sign", 1)]),
       lambda sks, msgs: [OC.Sign(k, m) for k, m in zip(sks, msgs)],
       lambda sks, msgs: [O.Sign(k, m) for k, m in zip(sks, msgs)])
def _(env, sks, msgs):
    raw = env.batch.sign_batch(b"".join(sk32(k) for k in sks), b"".join(msgs), ctx=env.ctx)
    return [raw[96 * i: 96 * i + 96] for i in range(len(sks))]


@_call("sk_to_pk_batch", lambda: ([21, 22],), lambda sks: [OC.SkToPk(k) for k in sks],
       lambda sks: [O.g1_compress(_g1(k)) for k in sks])
def _(env, sks):
    raw = env.batch.sk_to_pk_batch(b"".join(sk32(k) for k in sks), ctx=env.ctx)
    return [raw[48 * i: 48 * i + 48] for i in range(len(sks))]


# grouped aggregation, the shape of test_grouped_between_job_partial_and_finish: the pending batch's ten signatures in
# two groups (group g signs with the sum of its items' keys' sums -- but over different messages, so the expected
# aggregates are the oracle's)
def _grouped_args():
    p = pending("indexed", "bad3")
    return [p.sigs[96 * j: 96 * j + 96] for j in range(B)], [j % 2 for j in range(B)]


def _grouped(agg):
    return lambda sigs, ids: [agg([s for s, g in zip(sigs, ids) if g == grp]) for grp in (0, 1)]


@_call("aggregate_grouped", _grouped_args, _grouped(OC.Aggregate), _grouped(O.Aggregate))
def _(env, sigs, ids):
    return env.batch.aggregate_grouped(b"".join(sigs), ids, ctx=env.ctx)


# signing roots and merkleization: SHA-256 by their definitions
def _sha(a: bytes, b: bytes) -> bytes:
    return hashlib.sha256(a + b).digest()


@_call("compute_signing_roots", lambda: ([_msg(b"root", j) for j in range(3)], _msg(b"domain", 0)),
       lambda roots, dom: [_sha(r, dom) for r in roots], lambda roots, dom: [_sha(r, dom) for r in roots])
def _(env, roots, dom):
    return env.batch.compute_signing_roots(roots, dom, ctx=env.ctx)


def _merkle3(chunks, limit):
    assert len(chunks) == 3 and limit == 4
    return _sha(_sha(chunks[0], chunks[1]), _sha(chunks[2], bytes(32)))


@_call("merkleize", lambda: ([_msg(b"chunk", j) for j in range(3)], 4), _merkle3, _merkle3)
def _(env, chunks, limit):
    return env.batch.merkleize(chunks, limit, ctx=env.ctx)


# the resident G1 table: eight points [1] G .. [8] G replace the context's table, then two rows over three of them
def _table_args():
    return [OC.SkToPk(k) for k in range(1, 9)], [0, 1, 2], [[1, 1, 1], [2, 0, 3]]


def _table_oracle(pts, idx, rows):
    dec = [O.g1_decompress(pts[i]) for i in idx]
    out = []
    for row in rows:
        acc = None
        for k, p in zip(row, dec):
            if k:
                acc = O.g1_add(acc, O.g1_mul(p, k))
        out.append(O.g1_compress(acc))
    return [1] * len(pts), out


@_call("g1_table", _table_args, lambda pts, idx, rows: ([1] * 8, [OC.SkToPk(6), OC.SkToPk(11)]), _table_oracle)
def _(env, pts, idx, rows):
    table = env.batch.G1Table(env.ctx)
    ok = table.load(pts)
    return [int(v) for v in ok], env.batch.g1_lincomb_batch(table, idx, rows)


# blob KZG: two openings of linear polynomials p = a0 + a1 X (commitment a0 M[0] + a1 M[1], proof a1 M[0] at any z,
# y = a0 + a1 z), the second with y + 1: the batch check fails and each item is checked on its own (k_kzg_item_pairs)
def _kzg_args():
    items, a1s = [], []
    for i, (a0, a1, c, proof) in enumerate(K.linear_answers()[:2]):
        z = 0x1234567 + i
        items.append((c, z, (a0 + a1 * z + i) % K.R, proof))
        a1s.append(a1)
    return items, a1s


def _kzg_oracle(items, a1s):
    """e(C - [y] G1, G2) = e(proof, [tau - z] G2) with proof = [a1] G1 is C - [y] M[0] = [a1] (M[1] - [z] M[0]): the
    oracle's G1 arithmetic on the setup's points, no pairing"""
    m0, m1 = K.monomial_points()[:2]
    out = []
    for (c, z, y, proof), a1 in zip(items, a1s):
        assert proof == O.g1_compress(O.g1_mul(m0, a1))
        lhs = O.g1_add(O.g1_decompress(c), O.g1_neg(O.g1_mul(m0, y))) if y else O.g1_decompress(c)
        rhs = O.g1_mul(O.g1_add(m1, O.g1_neg(O.g1_mul(m0, z))), a1)
        out.append(lhs == rhs)
    return out


@_call("verify_kzg_proof_batch_failing", _kzg_args, lambda items, a1s: [True, False], _kzg_oracle)
def _(env, items, a1s):
    c, z, y, proof = zip(*items)
    return env.kzg.verify_kzg_proof_items(list(c), list(z), list(y), list(proof))


# cell KZG: polynomials of degree below 64 are their own interpolants on every cell and have the identity as proof, so
# an item holds iff its commitment commits to its cell's polynomial.  The second item pairs the first polynomial's
# commitment with another polynomial's cell: the batch check fails and each item is checked alone (k_cells_item_pairs)
def _cell_polys():
    rng = random.Random(0xCE1150)
    return CI.CellAnswer([rng.randrange(K.R)]), CI.CellAnswer([rng.randrange(K.R), rng.randrange(K.R)])


def _cell_args():
    a, b = _cell_polys()
    return [a.item(0), (a.commitment,) + b.item(1)[1:]],


def _cell_oracle(items):
    a, b = _cell_polys()
    out = []
    for (c, k, cell, proof), poly in zip(items, (a, b)):
        assert cell == poly.cell(k) and proof == K.IDENTITY48
        out.append(K.commit_monomial(poly.interpolant(k)) == c)
    return out


@_call("verify_cells_failing", _cell_args, lambda items: [True, False], _cell_oracle)
def _(env, items):
    c, k, cell, proof = zip(*items)
    return env.cells().verify_cell_kzg_proof_items(list(c), list(k), list(cell), list(proof))


# the registry grows by two keys (indices at its end: no pending batch names them)
@_call("registry_append", lambda: ([OC.SkToPk(200), OC.SkToPk(201)],), lambda pks: [True, True],
       lambda pks: [OC.KeyValidate(k) for k in pks])
def _(env, pks):
    return [bool(v) for v in env.registry.append(b"".join(pks))]


# calls that replace job 0's batch: the four host-buffer batch forms, each with its own bad item (6)
REPLACING = FORMS


def replacing(form: str) -> Pending:
    return pending(form, "bad6")
