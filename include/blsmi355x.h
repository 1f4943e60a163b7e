/*
 * libblsmi355x -- MI355X (gfx950) BLS12-381 signature-verification backend.
 *
 * C ABI: plain pointers and sizes, caller-owned contiguous buffers, no torch
 * or HIP types.  It replaces the arithmetic the reference reaches through
 * ``eth2spec.utils.bls`` (reference ``tests/core/pyspec/eth2spec/utils/bls.py``,
 * written ``E/utils/bls.py`` below), i.e. the milagro_bls_binding /
 * py_ecc entry points bound at E/utils/bls.py:1-32,57-68.
 *
 * Return convention:
 *    1  valid / success
 *    0  invalid input (decode, subgroup, infinity, empty-list rejection,
 *       failed verification)
 *   <0  internal or device error (BLS_E_*); bls_last_error() describes it.
 * The Python shim maps a negative code to an exception everywhere, and 0 to
 * an exception exactly where the reference raises (Aggregate, AggregatePKs,
 * Sign, SkToPk), to False elsewhere.
 *
 * Threading: one context per process/device; calls on a context are
 * serialised by an internal mutex.  All device memory and streams are owned
 * by the context.  Every compute entry point runs on the GPU; there is no
 * CPU fallback (a missing/failed device is an error).
 */
#ifndef BLSMI355X_H
#define BLSMI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BLS_E_DEVICE (-1)  /* HIP runtime / kernel failure */
#define BLS_E_ARG (-2)     /* bad argument (NULL pointer, size overflow) */
#define BLS_E_NOREG (-3)   /* indexed call without a loaded registry */

typedef struct bls_ctx bls_ctx;

/* FAV batch slots of one context (bls_fav_job_*): the first BLS_FAV_JOBS_INIT (env, default 10) get streams
 * (BLS_JOB_STREAMS per job, default 2). */
#define BLS_FAV_JOBS 16

/* Context on HIP device `device` (ordinal).  Returns 0 or BLS_E_*. */
int bls_ctx_create(int device, bls_ctx** out);
void bls_ctx_destroy(bls_ctx* ctx);
const char* bls_last_error(bls_ctx* ctx);
/* Device name / CU count for reports; returns 0 or BLS_E_*. */
int bls_device_info(bls_ctx* ctx, char* name, size_t name_len, int* cu_count);

/* ---- drop-in per-call API (one call = one reference wrapper call) ---- */

/* Verify  <- E/utils/bls.py:141-151 (milagro Verify / py_ecc Verify). */
int bls_verify(bls_ctx* ctx, const uint8_t* pk48, const uint8_t* msg, size_t msg_len, const uint8_t* sig96);

/* FastAggregateVerify  <- E/utils/bls.py:167-177.  n == 0 -> 0. */
int bls_fast_aggregate_verify(bls_ctx* ctx, const uint8_t* pks48, size_t n, const uint8_t* msg, size_t msg_len,
                              const uint8_t* sig96);

/* AggregateVerify  <- E/utils/bls.py:154-164.  msgs is the concatenation of
 * the n messages, msg_lens[i] their lengths.  n == 0 -> 0. */
int bls_aggregate_verify(bls_ctx* ctx, const uint8_t* pks48, size_t n, const uint8_t* msgs, const size_t* msg_lens,
                         const uint8_t* sig96);

/* Aggregate  <- E/utils/bls.py:180-184.  1 and out96 on success; 0 on empty
 * list or an undecodable / non-G2 signature (the reference raises). */
int bls_aggregate(bls_ctx* ctx, const uint8_t* sigs96, size_t n, uint8_t* out96);

/* G Aggregate calls in one: group g is the items i with group_id[i] == g and
 * (include == NULL || include[i] != 0), in any order.  Returns 1 or BLS_E_*.
 *
 * out_ok[g] = 1 and out96[96 g ..] = the compressed sum when group g has at
 * least one included item and every included signature decodes and, with
 * subgroup_check != 0, lies in G2; otherwise out_ok[g] = 0 and the 96 bytes
 * are zero.  With subgroup_check = 1 that is, group by group, what
 * bls_aggregate returns on the group's included signatures (code and bytes):
 *   - the infinity encoding is a valid member and contributes the identity;
 *   - a sum that is the identity (sigma and -sigma, or only infinity members)
 *     is ok = 1 with bytes c0 00..;
 *   - a bad member spoils only its own group;
 *   - an excluded item's bytes are never judged and affect no output.
 * subgroup_check = 0 decodes without the subgroup check, as bls_point_decode
 * does -- for signatures a batch has already verified; the sum is still the
 * correct sum of curve points (the additions are complete on E2(Fp2)).
 *
 * An id >= G, or G == 0 with B > 0, is BLS_E_ARG, refused before any device
 * call.  B == 0 returns 1 with every out_ok 0.  The call uses scratch of its
 * own: it may run between a FAV job's partial and finish without changing
 * that job's verdicts. */
int bls_aggregate_grouped(bls_ctx* ctx, const uint8_t* sigs96, size_t B, const uint32_t* group_id, size_t G,
                          const uint8_t* include, int subgroup_check, uint8_t* out96, uint8_t* out_ok);
/* The same on device pointers: d_sigs96 (96 B), d_include (B bytes, nullable;
 * typically the verdict buffer bls_fav_job_finish_dev wrote), d_out96 (96 G)
 * and d_ok (G) are device resident, group_id is a HOST array (free on return).
 * It first waits for every job stream of the context, as bls_d2h does (a
 * failing job's verdicts are written asynchronously); nothing passes through
 * the host, and the results are complete after bls_d2h / bls_sync. */
int bls_aggregate_grouped_dev(bls_ctx* ctx, const uint8_t* d_sigs96, size_t B, const uint32_t* group_id, size_t G,
                              const uint8_t* d_include, int subgroup_check, uint8_t* d_out96, uint8_t* d_ok);

/* _AggregatePKs  <- E/utils/bls.py:202-213 (eth_aggregate_pubkeys,
 * specs/altair/bls.md:36-52).  0 on empty list or any key failing
 * KeyValidate (the reference raises). */
int bls_aggregate_pks(bls_ctx* ctx, const uint8_t* pks48, size_t n, uint8_t* out48);

/* KeyValidate  <- E/utils/bls.py:395-397. */
int bls_key_validate(bls_ctx* ctx, const uint8_t* pk48);

/* Sign / SkToPk  <- E/utils/bls.py:187-194,216-221; sk is 32 bytes
 * big-endian, 0 < sk < r (else 0). */
int bls_sign(bls_ctx* ctx, const uint8_t* sk32, const uint8_t* msg, size_t msg_len, uint8_t* out96);
int bls_sk_to_pk(bls_ctx* ctx, const uint8_t* sk32, uint8_t* out48);

/* hash_to_G2 (RFC 9380 BLS12381G2_XMD:SHA-256_SSWU_RO_) with caller DST,
 * compressed output.  The POP DST is the spec's (beacon-chain.md:692). */
int bls_hash_to_g2(bls_ctx* ctx, const uint8_t* msg, size_t msg_len, const uint8_t* dst, size_t dst_len,
                   uint8_t* out96);

/* ---- batch API (throughput path) -------------------- */

/* Decode + KeyValidate n compressed pubkeys into the HBM-resident affine
 * registry (replacing any previous one).  out_valid[i] = 1/0 (may be NULL).
 * Returns 1 or BLS_E_*. */
int bls_registry_load(bls_ctx* ctx, const uint8_t* pks48, size_t n, uint8_t* out_valid);
size_t bls_registry_size(bls_ctx* ctx);
/* Generation of the registry table: bumped whenever bls_registry_load or
 * bls_registry_generate replaces it (appends keep it).  A host-side
 * pubkey -> index map is valid only for the generation it was built on. */
uint64_t bls_registry_generation(bls_ctx* ctx);

/* B FastAggregateVerify calls over registry indices: item b uses
 * idx[offsets[b] .. offsets[b+1]) (offsets has B+1 entries), message
 * msgs32[32 b ..], signature sigs96[96 b ..].  out[b] = 1/0.  One random-
 * linear-combination pairing check for the whole batch; on failure a
 * bisection (16-ary product tree, batched final exponentiations) isolates the
 * invalid items.  Returns 1 or BLS_E_*. */
int bls_fav_batch_indexed(bls_ctx* ctx, const uint32_t* idx, const uint64_t* offsets, size_t B, const uint8_t* msgs32,
                          const uint8_t* sigs96, uint8_t* out);

/* B independent Verify calls with registry indices (gossip firehose): the
 * same RLC batch check + bisection as bls_fav_batch_indexed with one key per
 * item.  Returns 1 or BLS_E_*. */
int bls_verify_batch_indexed(bls_ctx* ctx, const uint32_t* idx, size_t B, const uint8_t* msgs32,
                             const uint8_t* sigs96, uint8_t* out);

/* Shared-message batches: as bls_fav_batch_indexed / bls_verify_batch_indexed,
 * but item b's message is msgs32[32 * msg_id[b] ..], one of M table entries
 * (msg_id[b] < M, else BLS_E_ARG; M == 0 with B > 0 is BLS_E_ARG; both are
 * refused before any device call).  Table entries need not be distinct or
 * used.  out[b] equals what the unshared call returns for the expanded
 * messages.  The batch equation takes one hash_to_G2 and one Miller pair per
 * table entry instead of per item: prod_{i: m_i = m} e(r_i apk_i, H(m)) =
 * e(sum_i r_i apk_i, H(m)), the sum by a levelled fold on the device
 * (csrc/bls_g1_segsum.h).  The r_i stay per item (seed, b, message,
 * signature), so the soundness bound is the unshared batch's; a failing batch
 * bisects down to single items as ever.  Sharing pays when M < B; with
 * M == B nothing collapses and the fold is extra work, though at 125,000
 * items it measured no slower than the unshared call. */
int bls_fav_batch_indexed_shared(bls_ctx* ctx, const uint32_t* idx, const uint64_t* offsets, size_t B,
                                 const uint8_t* msgs32, size_t M, const uint32_t* msg_id, const uint8_t* sigs96,
                                 uint8_t* out);
int bls_verify_batch_indexed_shared(bls_ctx* ctx, const uint32_t* idx, size_t B, const uint8_t* msgs32, size_t M,
                                    const uint32_t* msg_id, const uint8_t* sigs96, uint8_t* out);

/* Work of the last FAV batch prepared on this context: messages hashed and
 * Miller pairs in its product (host counters, no device read).  An unshared
 * batch reports B and B + 64, a shared one M and M + 64.  Returns 0. */
int bls_last_batch_work(bls_ctx* ctx, uint64_t* hashes, uint64_t* miller_pairs);

/* Committee table: C committees as registry index lists, committee c =
 * idx[offsets[c] .. offsets[c+1]) (offsets has C+1 entries).  The lists stay
 * in HBM, replacing any earlier table, and one launch computes each
 * committee's projective key sum csum[c] and cstat[c] = 1 iff every member
 * index is below the registry size and marked valid.  An empty committee and
 * one whose sum is the identity are allowed (cstat 1).  The table belongs to
 * the registry generation it was loaded on: after bls_registry_load or
 * bls_registry_generate it is stale and the bits calls below return
 * BLS_E_ARG; bls_registry_append keeps it (a member that was out of range at
 * load time keeps cstat 0).  Returns 1 or BLS_E_*. */
int bls_committees_load(bls_ctx* ctx, const uint32_t* idx, const uint64_t* offsets, size_t C);
size_t bls_committees_count(bls_ctx* ctx);

/* B FastAggregateVerify calls whose signers are given as an attestation gives
 * them (get_attesting_indices): item b names the committees
 * comm_ids[comm_offs[b] .. comm_offs[b+1]) of the table and carries one bit
 * per member of their concatenation, in the bytes
 * bits[bit_offs[b] .. bit_offs[b+1]); bit k = (byte[k/8] >> (k%8)) & 1, the
 * SSZ bit order without the Bitlist delimiter.  With n_b the member count of
 * the item's committees, out[b] is what bls_fav_batch_indexed (msg_id NULL:
 * one message per item, M ignored) or bls_fav_batch_indexed_shared (msg_id:
 * a table of M messages) returns for the expanded index list -- the members
 * whose bit is 1, in order -- for every table, whatever it holds.
 * BLS_E_ARG before any device call: a committee id >= C, a byte count other
 * than ceil(n_b / 8), a bad msg_id, no or a stale table.  Verdict 0, decided
 * on the device: a padding bit set in the last byte; n_b == 0 or no bit set.
 * mode 0 (auto): an item's key is the committees' sums minus the
 * non-participants' keys iff every committee of the item has cstat 1 and
 * that adds fewer points, (n_b - p) + ncomm < p with p the bits set;
 * mode 1: always the participants' sum; mode 2: the complement wherever
 * cstat allows it (an item with no bit set has no work in any mode).  Modes
 * 1 and 2 are for tests and measurements.  Returns 1 or BLS_E_*. */
int bls_fav_batch_committee_bits(bls_ctx* ctx, const uint32_t* comm_ids, const uint64_t* comm_offs,
                                 const uint8_t* bits, const uint64_t* bit_offs, size_t B, const uint8_t* msgs32,
                                 size_t M, const uint32_t* msg_id, const uint8_t* sigs96, int mode, uint8_t* out);

/* The last bits batch prepared on this context (either entry point): points
 * its gather added -- keys, plus committee sums of complement items -- and
 * the number of complement items.  Waits for that batch's gather.  Returns 0. */
int bls_last_gather_work(bls_ctx* ctx, uint64_t* points_added, uint64_t* complement_items);

/* Key-table batches: B FastAggregateVerify calls on keys given as bytes.
 * keys48: a table of K compressed keys (duplicates allowed); item b uses table
 * entries idx[offsets[b] .. offsets[b+1]).  Messages: one per item (msg_id
 * NULL, M ignored) or a table of M with msg_id[b] < M, as in
 * bls_fav_batch_indexed_shared.  out[b] is what bls_fav_batch_indexed(_shared)
 * returns for the same idx / offsets on a registry loaded with keys48 -- i.e.
 * bls_fast_aggregate_verify on the item's keys:
 *   - a member that fails KeyValidate -> 0;
 *   - an index >= K -> 0;
 *   - an empty item -> 0;
 *   - the same key twice in an item counts twice.
 * out_key_valid (nullable, K bytes): the KeyValidate verdict per table entry
 * (with B == 0 the table is still judged when this is given).
 * The batch decodes and KeyValidates the table itself, into records of its
 * own, and then runs the indexed batch's pipeline on them: the RLC check, the
 * MSM and split Miller loop, the bisection on failure.  It needs no registry
 * and touches none: size, generation, committee table and any batch in flight
 * on another job are unaffected.  The price is K KeyValidates per batch, which
 * the registry pays once per key: keys that are used across batches -- the
 * validator set -- belong in the registry (bls_registry_load / _append); this
 * form is for keys that are not there (deposits, withdrawal keys, a run that
 * has loaded no registry).
 * K == 0 is allowed (every verdict 0).  K or B > 2^32 - 1, a bad msg_id,
 * M == 0 with msg_id: BLS_E_ARG before any device call.  Returns 1 or BLS_E_*. */
int bls_fav_batch_keys(bls_ctx* ctx, const uint8_t* keys48, size_t K, const uint32_t* idx, const uint64_t* offsets,
                       size_t B, const uint8_t* msgs32, size_t M, const uint32_t* msg_id, const uint8_t* sigs96,
                       uint8_t* out, uint8_t* out_key_valid);
/* One key per item: item b's key is table entry b (K == B) -- B Verify calls
 * on raw keys. */
int bls_verify_batch_keys(bls_ctx* ctx, const uint8_t* keys48, size_t B, const uint8_t* msgs32, size_t M,
                          const uint32_t* msg_id, const uint8_t* sigs96, uint8_t* out);

/* B AggregateVerify calls <- E/utils/bls.py:154-164 (one call per item).
 * Item b owns the pairs item_offs[b] .. item_offs[b+1] (item_offs has B+1
 * entries, total = item_offs[B]): pubkeys pks48[48 t ..], messages
 * msgs[msg_offs[t] .. msg_offs[t+1]) (msg_offs has total+1 entries, any
 * lengths), and signature sigs96[96 b ..].  out[b] = 1/0 with the per-call
 * semantics of bls_aggregate_verify (empty item, invalid key or signature ->
 * 0).  One random-linear-combination pairing check over all items; when it
 * fails every item is checked on its own (batched final exponentiations).
 * Returns 1 or BLS_E_*. */
int bls_aggregate_verify_batch(bls_ctx* ctx, const uint8_t* pks48, const uint8_t* msgs, const uint64_t* msg_offs,
                               const uint64_t* item_offs, size_t B, const uint8_t* sigs96, uint8_t* out);

/* Append n compressed keys to the HBM registry (deposits: new validator
 * indices reg_n .. reg_n + n), decoding + KeyValidate on the device like
 * bls_registry_load; out_valid as there.  Existing entries keep their
 * indices.  <- specs/phase0/beacon-chain.md:2037-2062 (add_validator_to_registry),
 * specs/electra/beacon-chain.md:1577-1588.  Returns 1 or BLS_E_*. */
int bls_registry_append(bls_ctx* ctx, const uint8_t* pks48, size_t n, uint8_t* out_valid);

/* ---- signing roots and SSZ merkleization ------ */
/* out32[i] = SHA-256(object_roots32[32 i ..] || domains32[domain_stride i ..]):
 * compute_signing_root  <- specs/phase0/beacon-chain.md:953-962 (SigningData
 * :317-320).  domain_stride 0 = one domain for all, 32 = one per item.
 * Returns 1 or BLS_E_*. */
int bls_signing_roots(bls_ctx* ctx, const uint8_t* object_roots32, const uint8_t* domains32, size_t domain_stride,
                      size_t n, uint8_t* out32);
/* SSZ merkleize(chunks, limit): n 32-byte chunks, tree of 2^depth leaves
 * (depth >= ceil(log2 n); missing leaves are zero chunks).  n = 0 gives the
 * zero-subtree root of that depth.  Returns 1 or BLS_E_*. */
int bls_merkleize(bls_ctx* ctx, const uint8_t* chunks32, size_t n, int depth, uint8_t* root32);
/* N deposit signature checks (is_valid_deposit_signature,
 * specs/electra/beacon-chain.md:1577-1588): message i is
 * compute_signing_root(DepositMessage(pubkey_i, wc_i, amount_i), domain32),
 * computed on the device (five SHA-256 nodes per deposit).
 * out[i] = bls_verify(pubkey_i, that root, sig_i), through
 * bls_verify_batch_keys's path (table = the N keys).  out_roots32 (nullable):
 * the N signing roots.  Appending the accepted new keys to the registry is
 * the caller's (bls_registry_append: which deposits are top-ups is its
 * knowledge).  Returns 1 or BLS_E_*. */
int bls_deposits_verify(bls_ctx* ctx, const uint8_t* pubkeys48, const uint8_t* wc32, const uint64_t* amounts,
                        const uint8_t* sigs96, const uint8_t* domain32, size_t N, uint8_t* out, uint8_t* out_roots32);

/* ---- KZG pieces ---------------------------------- */
/* pairing_check  <- E/utils/bls.py pairing_check (used by
 * specs/deneb/polynomial-commitments.md:284,407,451): 1 iff
 * prod_i e(P_i, Q_i) == 1 for compressed P_i (48 B, identity allowed) and
 * Q_i (96 B, identity allowed); both subgroup-checked.  0 if the product is
 * not 1 or any encoding is invalid.  Returns 1 / 0 / BLS_E_*. */
int bls_pairing_check(bls_ctx* ctx, const uint8_t* g1s48, const uint8_t* g2s96, size_t n);
/* multi_exp / g1_lincomb  <- E/utils/bls.py multi_exp
 * (specs/deneb/polynomial-commitments.md g1_lincomb): out48 = compressed
 * sum_i [k_i] P_i, scalars as 32-byte big-endian integers.  1 on success, 0
 * if a point encoding is invalid (the reference raises).  Returns 1 / 0 /
 * BLS_E_*. */
int bls_g1_multi_exp(bls_ctx* ctx, const uint8_t* g1s48, const uint8_t* scalars32, size_t n, uint8_t* out48);

/* ---- curve objects  <- E/utils/bls.py:224-392 ---------------------------
 * The arkworks G1Point / G2Point / GT operations of the reference's
 * fastest_bls helpers: add (:239-246), multiply (:249-259), multi_exp
 * (:262-296), neg (:299-306), bytes48_to_G1 / bytes96_to_G2 (unchecked decode,
 * :367-392), G1_to_bytes48 / G2_to_bytes96 (:345-364), pairing_check
 * (:224-236).  group: 1 = G1 (48-byte compressed), 2 = G2 (96-byte).  The
 * identity encoding is a valid point.  Return 1 on success, 0 if an encoding
 * is invalid (the reference raises), BLS_E_* on errors. */
/* out_ok[i] (may be NULL) = 1 iff in[i] decodes (and, with subgroup_check, lies
 * in G1 / G2); returns 1 iff all do. */
int bls_point_decode(bls_ctx* ctx, int group, const uint8_t* in, size_t n, int subgroup_check, uint8_t* out_ok);
int bls_point_add(bls_ctx* ctx, int group, const uint8_t* a, const uint8_t* b, uint8_t* out);
/* [k] P, k a 32-byte big-endian integer (the reference reduces scalars mod r first) */
int bls_point_mul(bls_ctx* ctx, int group, const uint8_t* p, const uint8_t* k32, uint8_t* out);
int bls_point_neg(bls_ctx* ctx, int group, const uint8_t* p, uint8_t* out);
/* sum_i [k_i] P_i.  n == 0 -> 0 (the reference raises, E/utils/bls.py:270-271).
 * subgroup_check 0 = multiexp_unchecked (:280-282). */
int bls_multi_exp(bls_ctx* ctx, int group, const uint8_t* pts, const uint8_t* scalars32, size_t n, int subgroup_check,
                  uint8_t* out);
/* ---- resident G1 point table and its batched MSM (KZG g1_lincomb) ------- */
/* The points a spec run multiplies again and again (KZG_SETUP_G1_LAGRANGE,
 * KZG_SETUP_G1_MONOMIAL; specs/deneb/polynomial-commitments.md:266-286) are
 * decoded once and kept in HBM, one table per context, with the window
 * multiples 2^(8w) P (w = 0..31) of every entry as 128-byte affine records
 * (4 KiB per entry), so that an MSM over them is additions only.
 *
 * bls_g1_table_load replaces the table with the n points of pts48 (decoded as
 * bls_point_decode does, with or without the subgroup check); out_ok[i]
 * (may be NULL) = 1 iff pts48[i] is a valid encoding (and, with
 * subgroup_check, in G1).  An invalid entry keeps its index and is unusable:
 * an MSM that names it returns 0.  The identity encoding is valid and
 * contributes nothing.  bls_g1_table_append adds n entries at indices
 * size .. size + n; existing indices stay.  At most 2^26 entries.
 * bls_g1_table_generation is bumped whenever the table is replaced (appends
 * keep it): a host-side bytes -> index map is valid only for the generation
 * it was built on.  Return 1 or BLS_E_*. */
int bls_g1_table_load(bls_ctx* ctx, const uint8_t* pts48, size_t n, int subgroup_check, uint8_t* out_ok);
int bls_g1_table_append(bls_ctx* ctx, const uint8_t* pts48, size_t n, int subgroup_check, uint8_t* out_ok);
size_t bls_g1_table_size(bls_ctx* ctx);
uint64_t bls_g1_table_generation(bls_ctx* ctx);
/* out48[v] = sum_i [k_{v,i}] T[idx[i]] for v < B: one shared list of n table
 * indices and a B x n matrix of 32-byte big-endian scalars (row v at
 * scalars32 + 32 n v), any 0 <= k < 2^256 taken as an integer multiple, as
 * bls_multi_exp takes them.  An index may repeat.  Returns 1; 0 if an index
 * names an invalid entry (the reference raises); BLS_E_NOREG without a table;
 * BLS_E_ARG if n == 0 (the reference raises on an empty input), B == 0,
 * B > 65,536, 32 B n >= 2^31 or an index is not below the table size. */
int bls_g1_table_msm(bls_ctx* ctx, const uint32_t* idx, size_t n, const uint8_t* scalars32, size_t B, uint8_t* out48);
/* Totals since the context was created: bls_g1_table_msm calls that ran and
 * the bucket entries (non-zero digits of non-identity entries) they added.
 * Returns 0. */
int bls_g1_table_stats(bls_ctx* ctx, uint64_t* msm_calls, uint64_t* bucket_entries);
/* ---- bucket MSM over a call's own G1 points (variable base) --------------- */
/* out48[v] = sum_i [k_{v,i}] P_i for v < B: n compressed points, decoded as
 * bls_multi_exp decodes them (identity accepted, subgroup check on request),
 * and a B x n matrix of 32-byte big-endian scalars (row v at
 * scalars32 + 32 n v), any 0 <= k < 2^256 taken as an integer multiple and not
 * reduced mod r: for a point decoded without the subgroup check the result is
 * the bytes bls_multi_exp gives.  Always the bucket path (digit sort per (row,
 * window), bucket folds, one doubling chain per row), from n = 1: callers
 * choose between this and bls_multi_exp.  Returns 1; 0 for an invalid
 * encoding, a point outside G1 under subgroup_check, or n == 0 (the reference
 * raises on an empty input); BLS_E_ARG for null pointers, B == 0, B > 256 or
 * 32 B n >= 2^31. */
int bls_g1_msm(bls_ctx* ctx, const uint8_t* pts48, size_t n, const uint8_t* scalars32, size_t B, int subgroup_check,
               uint8_t* out48);
/* Totals since the context was created: bucket MSMs over a call's own points
 * that ran and the bucket entries (non-zero digits of non-identity points)
 * their sorts placed.  Returns 0. */
int bls_g1_msm_stats(bls_ctx* ctx, uint64_t* calls, uint64_t* bucket_entries);
/* ---- Deneb blob KZG on the device (specs/deneb/polynomial-commitments.md) -- */
/* A blob is 4,096 field elements of 32 big-endian bytes (131,072 bytes), the
 * evaluations of a polynomial p over the bit-reversed 4,096th roots of unity;
 * z, y are 32-byte big-endian elements of F_r; commitments and proofs are
 * 48-byte compressed G1 points.  The scalar-field arithmetic (range checks,
 * barycentric evaluation, quotients, the batch's random linear combination)
 * and the group side all run on the device.  Return 1 on success, 0 where the
 * spec asserts (an element, z or y >= r; an invalid or non-G1 encoding) or a
 * verification fails, BLS_E_* otherwise.
 *
 * The Fiat-Shamir challenge of the blob functions is an input (z32): it is
 * one SHA-256 over a sequential transcript of 131,152 bytes -- the 16 bytes
 * "FSBLOBVERIFY_V1_", the number 4,096 as 16 big-endian bytes, the blob, the
 * 48-byte commitment -- taken as a big-endian integer mod r
 * (compute_challenge, :247-264).  The host's SHA-256 does that in about
 * 0.1 ms; bls_mi355x/kzg.py computes it.
 *
 * bls_kzg_setup: g2_tau96 = KZG_SETUP_G2_MONOMIAL[1] (subgroup-checked; kept
 * negated).  lagrange_n = 0 sets up verification only; lagrange_n = 4096
 * names entries lagrange_first .. lagrange_first + 4096 of the resident G1
 * table (bls_g1_table_load / _append) as the bit-reversal-permuted
 * KZG_SETUP_G1_LAGRANGE.  Returns 0 if tau's encoding or a named entry is
 * invalid, BLS_E_NOREG without a table, BLS_E_ARG if the entries are out of
 * range.  The setup remembers bls_g1_table_generation: after the table has
 * been replaced, commitment and proof calls return BLS_E_ARG until
 * bls_kzg_setup is called again (verification is unaffected).  A call that
 * needs a setup (or its Lagrange entries) and finds none: BLS_E_NOREG. */
int bls_kzg_setup(bls_ctx* ctx, const uint8_t* g2_tau96, uint32_t lagrange_first, uint32_t lagrange_n);
/* y32[b] = p_b(z32[b]) (evaluate_polynomial_in_evaluation_form, :319-351) for
 * B <= 1,024 blobs.  A z >= r returns 0.  out_ok[b] (may be NULL) = 1 iff
 * every element of blob b is < r; otherwise y32[b] is zero.  Returns 1 iff
 * every blob is ok.  Needs no setup. */
int bls_kzg_eval_blobs(bls_ctx* ctx, const uint8_t* blobs, size_t B, const uint8_t* z32, uint8_t* y32,
                       uint8_t* out_ok);
/* out48[b] = blob_to_kzg_commitment(blob b): one row of the table MSM per
 * blob, B <= 511.  out_ok as above; a bad blob's 48 bytes are zero. */
int bls_kzg_blob_commitments(bls_ctx* ctx, const uint8_t* blobs, size_t B, uint8_t* out48, uint8_t* out_ok);
/* compute_kzg_proof_impl (:508-541) for B <= 511 blobs: y32[b] = p_b(z_b) and
 * proofs48[b] = the commitment to (p_b(X) - y_b) / (X - z_b), for z_b inside
 * or outside the domain.  out_ok and the return value as above. */
int bls_kzg_compute_proofs(bls_ctx* ctx, const uint8_t* blobs, size_t B, const uint8_t* z32, uint8_t* proofs48,
                           uint8_t* y32, uint8_t* out_ok);
/* verify_kzg_proof_batch (:412-463) as one check
 *   e(sum r_i pi_i, -[tau] G2) e(sum r_i C_i + sum r_i z_i pi_i - (sum r_i y_i) G1, G2) == 1
 * with independent 128-bit r_i derived from bls_host_seed (BLS_E_DEVICE when
 * the entropy source fails): a batch with a false item passes with
 * probability at most 2^-128.  n <= 65,536; n == 0 returns 1.  Returns 1 iff
 * every item verifies.  An invalid encoding (the identity c0 00.. is valid)
 * or a z or y >= r returns 0 without a pairing; out_item (may be NULL) then
 * holds 0 for exactly the invalid items.  Otherwise out_item[i] = item i's
 * own verdict: all ones after a passing batch, and after a failing one each
 * item's own two-pair check. */
int bls_kzg_verify_batch(bls_ctx* ctx, const uint8_t* commitments48, const uint8_t* z32, const uint8_t* y32,
                         const uint8_t* proofs48, size_t n, uint8_t* out_item);
/* verify_blob_kzg_proof_batch (:589-614) given the challenges: y_b = p_b(z_b)
 * on the device, then the batch check above on (C_b, z_b, y_b, pi_b).  A blob
 * with an element >= r is an invalid item.  B <= 1,024. */
int bls_kzg_verify_blob_batch(bls_ctx* ctx, const uint8_t* blobs, const uint8_t* commitments48,
                              const uint8_t* proofs48, const uint8_t* z32, size_t B, uint8_t* out_item);
/* ---- Fulu cell KZG on the device (specs/fulu/polynomial-commitments-sampling.md) -- */
/* A cell is 64 field elements of 32 big-endian bytes (2,048 bytes); a blob
 * extends to 128 cells: the evaluations of its polynomial over the
 * bit-reversed 8,192nd roots of unity, so cells 0 .. 63 are the blob itself.
 * The transforms are number-theoretic transforms over F_r on the device.
 * Cell computation and recovery need no setup.
 *
 * bls_kzg_cells_setup: g2_tau64_96 = KZG_SETUP_G2_MONOMIAL[64] (subgroup-
 * checked; kept negated); monomial_n = 64 names entries monomial_first ..
 * monomial_first + 64 of the resident G1 table as KZG_SETUP_G1_MONOMIAL[0..64).
 * Returns 0 if the encoding or a named entry is invalid, BLS_E_NOREG without a
 * table, BLS_E_ARG if the entries are out of range or monomial_n is not 64.
 * The setup remembers bls_g1_table_generation: after the table has been
 * replaced, bls_kzg_verify_cells returns BLS_E_ARG until the setup is made
 * again; without a setup it returns BLS_E_NOREG. */
int bls_kzg_cells_setup(bls_ctx* ctx, const uint8_t* g2_tau64_96, uint32_t monomial_first, uint32_t monomial_n);
/* verify_cell_kzg_proof_batch's check on n <= 8,192 items (n == 0 returns 1):
 * item k is the cell cells + 2048 k with index cell_index[k] < 128, the proof
 * proofs48 + 48 k and the commitment commitments48 + 48 commitment_index[k] of
 * n_commitments <= 8,192 distinct ones (an index not below n_commitments:
 * BLS_E_ARG).  One check of the universal verification equation
 *   e(sum r_k pi_k, [tau^64] G2) ==
 *   e(sum_i w_i C_i - sum_m s_m [tau^m] G1 + sum r_k h_k^64 pi_k, G2)
 * with w_i the sum of the r_k of commitment i's items, s_m = sum r_k c_{k,m}
 * over the coefficients c_k of cell k's interpolation polynomial (an inverse
 * 64-point transform per cell) and h_k the cell's coset shift.  The r_k are
 * independent 128-bit values derived from bls_host_seed as in
 * bls_kzg_verify_batch, not powers of the spec's challenge: a batch with a
 * false item passes with probability at most 2^-128.  Returns 1 iff every
 * item verifies.  An invalid encoding (the identity is valid), a field
 * element >= r or a cell index >= 128 returns 0 without a pairing; out_item
 * (may be NULL) then holds 0 for exactly the invalid items.  Otherwise
 * out_item[k] = item k's own verdict: all ones after a passing batch, and
 * after a failing one each item's own two-pair check. */
int bls_kzg_verify_cells(bls_ctx* ctx, const uint8_t* commitments48, size_t n_commitments,
                         const uint32_t* commitment_index, const uint32_t* cell_index, const uint8_t* cells,
                         const uint8_t* proofs48, size_t n, uint8_t* out_item);
/*
 * bls_kzg_compute_cells: cells[b] = compute_cells(blob b), 128 x 2,048 bytes
 * per blob, for B <= 128 blobs: the inverse 4,096-point transform of the blob
 * and the 8,192-point transform of its zero-padded coefficients.  out_ok[b]
 * (may be NULL) = 1 iff every element of blob b is < r; otherwise blob b's
 * cells are zero.  Returns 1 iff every blob is ok. */
int bls_kzg_compute_cells(bls_ctx* ctx, const uint8_t* blobs, size_t B, uint8_t* cells, uint8_t* out_ok);
/* The cells of recover_cells_and_kzg_proofs (recover_polynomialcoeff, then the
 * extension above; the cell proofs are not computed) for B <= 128 blobs that
 * share one list of present cells: cell_index, 64 <= n_present <= 128 strictly
 * ascending indices below 128 (anything else: BLS_E_ARG); cells holds blob b's
 * cell p (index cell_index[p]) at cells + 2048 (b n_present + p).  out_cells,
 * out_ok and the return value as above, with every element of the given cells
 * checked.  Given cells that lie on no polynomial of degree < 4,096 yield what
 * the spec's algorithm yields on them. */
int bls_kzg_recover_cells(bls_ctx* ctx, const uint32_t* cell_index, size_t n_present, const uint8_t* cells, size_t B,
                          uint8_t* out_cells, uint8_t* out_ok);
/* The radix-2 transform over G1, out[k] = sum_i [w_n^(i k)] in[i] with w_n the
 * n-th root of unity of the cell functions' domain (w_n = w^(8192 / n), w =
 * 7^((r - 1) / 8192)), for B >= 1 independent vectors of n = 2^k points, 2 <= n
 * <= 4,096: vector v is the n compressed points at in48 + 48 n v, and its
 * transform goes to out48 + 48 n v.  Input and output are in natural order.
 * inverse != 0 takes w_n^-1 and includes the factor 1 / n.  The identity
 * (c0 00...) is a valid point anywhere.  Returns 1 on success; 0 if an
 * encoding is invalid or not in G1 (out48 is not written); BLS_E_ARG if n is
 * not a power of two in 2 .. 4,096, B == 0 or n B > 2^20.  One kernel launch
 * per stage, one lane per butterfly over all B vectors. */
int bls_g1_fft(bls_ctx* ctx, const uint8_t* in48, size_t n, size_t B, int inverse, uint8_t* out48);
/* ---- Fulu cell proofs (compute_cells_and_kzg_proofs, recover_cells_and_kzg_proofs) -- */
/* bls_kzg_cell_proofs_setup: monomial_n = 4,096 names entries monomial_first ..
 * monomial_first + 4,096 of the resident G1 table as KZG_SETUP_G1_MONOMIAL
 * ([tau^i] G1).  Returns 1; 0 if a named entry is invalid; BLS_E_NOREG without
 * a table; BLS_E_ARG if the entries are out of range or monomial_n is not
 * 4,096.  It remembers bls_g1_table_generation as bls_kzg_cells_setup does: the
 * two calls below return BLS_E_NOREG without this setup and BLS_E_ARG after the
 * table has been replaced, until the setup is made again.  It is independent
 * of bls_kzg_cells_setup (proofs need no G2 point), and bls_g1_table_append
 * keeps both valid.
 *
 * bls_kzg_compute_cells_and_proofs: bls_kzg_compute_cells (same arguments,
 * checks, cell bytes, out_ok and return value; cells may be NULL here) and the
 * 128 proofs of every blob, 48 bytes each in cell order at proofs48 + 6144 b.
 * With p = sum f_i X^i the blob's polynomial, the proof of cell k is
 *   pi_k = sum_{m < 64} [a_k^m] h_m,  a_k = w_128^brp7(k),
 *   h_m = sum_{i < 4096 - 64 (m + 1)} f_{i + 64 (m + 1)} [tau^i] G1
 * the h_m being 63 rows per blob of the table MSM (bls_g1_table_msm's kernels;
 * zero scalars cost nothing there) and the pi_k one 128-point bls_g1_fft over
 * all blobs.  A blob that is not ok gets 128 x 48 zero bytes.
 *
 * bls_kzg_recover_cells_and_proofs: bls_kzg_recover_cells (same arguments,
 * checks, cell bytes, out_ok and return value) and the proofs of the recovered
 * polynomial as above. */
int bls_kzg_cell_proofs_setup(bls_ctx* ctx, uint32_t monomial_first, uint32_t monomial_n);
int bls_kzg_compute_cells_and_proofs(bls_ctx* ctx, const uint8_t* blobs, size_t B, uint8_t* cells, uint8_t* proofs48,
                                     uint8_t* out_ok);
int bls_kzg_recover_cells_and_proofs(bls_ctx* ctx, const uint32_t* cell_index, size_t n_present, const uint8_t* cells,
                                     size_t B, uint8_t* out_cells, uint8_t* out_proofs48, uint8_t* out_ok);
/* GT.multi_pairing: prod_i e(P_i, Q_i) after the final exponentiation, as 576
 * bytes (six Fp2 coefficients c0..c5 of the w-basis, each c0||c1 big-endian;
 * GT one = byte 47 set).  n == 0 gives one. */
int bls_multi_pairing(bls_ctx* ctx, const uint8_t* g1s48, const uint8_t* g2s96, size_t n, int subgroup_check,
                      uint8_t* out576);
int bls_gt_mul(bls_ctx* ctx, const uint8_t* a576, const uint8_t* b576, uint8_t* out576);
/* pairing_check over curve objects (arkworks GT.multi_pairing(...) == GT.one(),
 * :229): subgroup_check 0 skips the subgroup checks of bls_pairing_check. */
int bls_pairing_check_ex(bls_ctx* ctx, const uint8_t* g1s48, const uint8_t* g2s96, size_t n, int subgroup_check);

/* Fallback statistics of the last batch finished on this context: the number
 * of final-exponentiation checks and bisection rounds (tree levels) it ran
 * (both 0 when the whole-batch check passed; waits for that batch's
 * verdicts).  Returns 0 or BLS_E_*. */
int bls_last_fallback_stats(bls_ctx* ctx, uint64_t* fe_checks, uint64_t* rounds);

/* Synthetic registry for benchmarks: pk_i = (first_sk + i) * G1 written
 * straight into the HBM registry (all valid); compressed keys are copied
 * to out_pks48 when non-NULL.  Returns 1 or BLS_E_*. */
int bls_registry_generate(bls_ctx* ctx, uint64_t first_sk, size_t n, uint8_t* out_pks48);

/* Synthetic-data helpers (used by bench.py and tests to make inputs). */
int bls_sign_batch(bls_ctx* ctx, const uint8_t* sks32, const uint8_t* msgs32, size_t B, uint8_t* out96);
int bls_sk_to_pk_batch(bls_ctx* ctx, const uint8_t* sks32, size_t B, uint8_t* out48);

/* ---- device-resident variants (inputs already in HBM) ----------------- */
void* bls_dev_alloc(bls_ctx* ctx, size_t bytes);
int bls_dev_free(bls_ctx* ctx, void* dptr);
int bls_h2d(bls_ctx* ctx, void* dst, const void* src, size_t bytes);
/* bls_d2h and bls_sync first wait for every job stream of the context (verdicts
 * of pipelined jobs are written asynchronously, see bls_fav_job_finish_dev). */
int bls_d2h(bls_ctx* ctx, void* dst, const void* src, size_t bytes);
int bls_sync(bls_ctx* ctx);

/* Phase 1 of a (possibly multi-GPU) FAV batch on device pointers: per-item
 * checks and this shard's Miller-loop product, written to partial576 (host,
 * 576 bytes: the 6 w-basis Fp2 coefficients, each c0||c1 big-endian).
 * seed32 keys the RLC scalars.  Per-item state stays in the context. */
int bls_fav_batch_partial_dev(bls_ctx* ctx, const uint32_t* d_idx, const uint64_t* d_offsets, size_t B,
                              const uint8_t* d_msgs32, const uint8_t* d_sigs96, const uint8_t* seed32,
                              uint8_t* partial576);
/* Final exponentiation of the product of n partials == 1 ?  1 / 0. */
int bls_partials_check(bls_ctx* ctx, const uint8_t* partials576, size_t n);
/* Phase 2: write verdicts for the batch prepared by the last
 * bls_fav_batch_partial_dev call on this context.  batch_ok = result of
 * bls_partials_check; when 0 this shard is bisected (its own product is
 * re-checked first, so a bad shard elsewhere leaves these verdicts intact). */
int bls_fav_batch_finish_dev(bls_ctx* ctx, int batch_ok, uint8_t* d_out);

/* ---- pipelined FAV batches (device-resident inputs) --------------------
 * The three phases above, split per job so that up to BLS_FAV_JOBS batches
 * are in flight on one context: while job k's Miller product is gathered
 * (RCCL) and final-exponentiated, job k+1's kernels already run on the job's
 * own streams.  A job must be finished before it is submitted again; each
 * job keeps its own per-item state for its finish/bisection.  Same meaning,
 * return codes and verdicts as bls_fav_batch_partial_dev / bls_partials_check
 * / bls_fav_batch_finish_dev (those are job 0, submitted and waited at once).
 *   submit:  enqueue the batch, return at once (1 or BLS_E_*)
 *   partial: wait for the job's 576-byte Miller product
 *   check:   final exponentiation of the product of n partials: 1 / 0
 *   finish:  verdicts into d_out, enqueued on the job's stream without a host
 *            wait -- a failing batch's bisection runs there on the device (no
 *            host round trip per round) while the host checks the next job;
 *            bls_d2h / bls_sync wait for it
 * Other calls on the context between a job's submit and its finish -- the
 * per-call verifications, aggregation, the pairing and curve calls, the G1
 * table, signing roots, the KZG calls, bls_registry_append -- run on job 0
 * and leave a submitted batch's verdicts unchanged, on job 0 as on every
 * other job, with or without a communicator.  The exceptions replace what the
 * slot holds:
 *   - the host-buffer batch calls (bls_fav_batch_indexed, _indexed_shared,
 *     _keys, _committee_bits, bls_verify_batch_*, bls_deposits_verify)
 *     prepare their batch on job 0: a batch submitted there before is
 *     replaced.  bls_fav_job_check_own(ctx, 0) is then BLS_E_ARG, and
 *     bls_fav_job_finish_dev(ctx, 0, 0, d_out) bisects the replacing batch
 *     from its root and writes that batch's verdicts.
 *   - bls_committees_load and the registry calls wait for the device before
 *     they replace (or grow) a table, so the pending batch's verdicts are
 *     unchanged: a submitted batch has read the tables it was submitted on. */
int bls_fav_job_submit_dev(bls_ctx* ctx, int job, const uint32_t* d_idx, const uint64_t* d_offsets, size_t B,
                           const uint8_t* d_msgs32, const uint8_t* d_sigs96, const uint8_t* seed32);
/* The shared-message form of submit (bls_fav_batch_indexed_shared): d_idx,
 * d_offsets, the message table d_msgs32 (M entries) and d_sigs96 are device
 * resident; msg_id is a HOST array of B entries (the library builds its
 * tables from it and uploads them on the job's stream from a job-owned host
 * copy that lives until the job is finished, so the caller's array is free
 * on return).  partial / check / check_own / check_comm / finish are the
 * calls above, unchanged. */
int bls_fav_job_submit_shared_dev(bls_ctx* ctx, int job, const uint32_t* d_idx, const uint64_t* d_offsets, size_t B,
                                  const uint8_t* d_msgs32, size_t M, const uint32_t* msg_id,
                                  const uint8_t* d_sigs96, const uint8_t* seed32);
/* The committee-bitfield form of submit (bls_fav_batch_committee_bits): the
 * bit bytes d_bits, the messages (B of them, or with msg_id a table of M) and
 * d_sigs96 are device resident; comm_ids, comm_offs, bit_offs and msg_id are
 * HOST arrays, checked before any device call and uploaded from job-owned
 * copies that live until the job is finished.  The calls around it are
 * unchanged. */
int bls_fav_job_submit_bits_dev(bls_ctx* ctx, int job, const uint32_t* comm_ids, const uint64_t* comm_offs,
                                const uint8_t* d_bits, const uint64_t* bit_offs, size_t B, const uint8_t* d_msgs32,
                                size_t M, const uint32_t* msg_id, const uint8_t* d_sigs96, int mode,
                                const uint8_t* seed32);
/* The key-table form of submit (bls_fav_batch_keys): d_keys48 (K keys),
 * d_idx, d_offsets, d_msgs32 (B messages, or with msg_id a table of M) and
 * d_sigs96 are device resident, msg_id is a HOST array (nullable) as in the
 * shared form.  d_keys48 must be 4-byte aligned (the kernels read the key
 * bytes as 32-bit words; any bls_dev_alloc / hipMalloc base is, and so is any
 * offset of whole keys from one).  The decoded table is the job's own, so
 * jobs in flight together each keep theirs.  partial / check / check_own / check_comm /
 * finish are the calls below, unchanged. */
int bls_fav_job_submit_keys_dev(bls_ctx* ctx, int job, const uint8_t* d_keys48, size_t K, const uint32_t* d_idx,
                                const uint64_t* d_offsets, size_t B, const uint8_t* d_msgs32, size_t M,
                                const uint32_t* msg_id, const uint8_t* d_sigs96, const uint8_t* seed32);
int bls_fav_job_partial(bls_ctx* ctx, int job, uint8_t* partial576);
int bls_fav_job_check(bls_ctx* ctx, int job, const uint8_t* partials576, size_t n);
/* check_own: the final exponentiation of the job's own product alone, which
 * submit already enqueued on the job's stream (the single-GPU check: no host
 * round trip of the partial; with a communicator it runs on demand): 1 / 0.
 * A finish after a failed multi-shard check uses the same verdict -- a job
 * whose own product passes keeps every per-item status, one whose own product
 * fails bisects below its root.  Another batch prepared on the job since its
 * submit (the host-buffer calls use job 0) voids that verdict: check_own is
 * then BLS_E_ARG and a failing finish bisects from the root. */
int bls_fav_job_check_own(bls_ctx* ctx, int job);
int bls_fav_job_finish_dev(bls_ctx* ctx, int job, int batch_ok, uint8_t* d_out);

/* ---- multi-GPU exchange over RCCL ----------------------
 * One communicator per context.  bls_comm_unique_id runs on one rank; its 128
 * bytes reach the other ranks out of band (bench.py: the torchrun TCP store).
 * With a communicator on the context, bls_fav_job_submit_dev itself enqueues
 * the exchange behind the job's Miller product: the 576-byte partial is
 * all-gathered on the device (ncclAllGather over xGMI, on the context's one
 * comm stream, so the collectives run in submission order -- every rank
 * submits the same jobs in the same order) and the job's stream multiplies
 * the world partials inside the final-exponentiation kernel.  No host step
 * sits between a job's product and its verdict; bls_fav_job_check_comm only
 * waits for that verdict (1 / 0).  The job's own check is then not enqueued:
 * a failing verdict is localised by bls_fav_job_finish_dev(..., 0, ...) on
 * every rank, which checks its own partial first, so only the bad shard
 * bisects.  A rank with an empty shard submits B = 0 (its partial is the
 * identity) and still joins every all-gather; B = 0 without a communicator is
 * BLS_E_ARG.  A submit that fails after the communicator exists aborts it
 * (below), so peers never wait for this rank's collective. */
int bls_comm_unique_id(uint8_t* out128);
int bls_comm_init(bls_ctx* ctx, const uint8_t* uid128, int rank, int world);
int bls_comm_destroy(bls_ctx* ctx);
int bls_fav_job_check_comm(bls_ctx* ctx, int job);
/* Abort the communicator (ncclCommAbort): peers blocked in a collective with
 * this rank fail instead of hanging.  The library calls it itself when
 * bls_fav_job_submit_dev or bls_fav_job_check_comm fails after the communicator exists; a host that
 * leaves the exchange on its own error (bench.py, dist.py) calls it before
 * exiting.  No-op without a communicator. */
int bls_comm_abort(bls_ctx* ctx);

/* ---- tracing: hipEvent time per kernel of the FAV path ------------------ */
int bls_profile_enable(bls_ctx* ctx, int on);  /* also resets the totals */
/* Fills up to max entries of total_ms / counts; returns the entry count. */
int bls_profile_read(bls_ctx* ctx, double* total_ms, uint64_t* counts, int max);
const char* bls_profile_name(int i);

/* ---- RLC seed entropy (host only, no device needed) ----------------------
 * bls_host_seed fills 32 bytes from the entropy source (/dev/urandom) and
 * returns 0, or BLS_E_DEVICE (seed zeroed) when fewer than 32 bytes can be
 * read: every batch call that draws an RLC seed then fails closed with
 * BLS_E_DEVICE instead of using a predictable seed.  bls_set_entropy_source
 * redirects the source (process-wide) and exists for tests. */
int bls_host_seed(uint8_t* seed32);
int bls_set_entropy_source(const char* path);

/* ---- test hooks (tests/ only; no reference counterpart) -------------------
 * bls_test_force_h2c_fallback: items i < n with mask[i] != 0 of every later
 * hash_to_G2 (batch, per-call, AggregateVerify) take the reference-path
 * fallback kernel as if the lane kernels had flagged them; n = 0 clears.
 * Refused (BLS_E_ARG) unless the environment has BLSMI355X_TEST_HOOKS=1, so a
 * production process cannot reroute its hashes by accident.
 * bls_test_hash_to_g2_batch: hash_to_G2 (DST POP) of n 32-byte messages through
 * the FAV batch's kernels and fallback routing, compressed into out96. */
int bls_test_force_h2c_fallback(bls_ctx* ctx, const uint8_t* mask, size_t n);
int bls_test_hash_to_g2_batch(bls_ctx* ctx, const uint8_t* msgs32, size_t n, uint8_t* out96);
/* bls_test_miller_forms: the product of n pairings (48-B G1 / 96-B G2 encodings, no subgroup checks) through each
 * Miller-loop form of the batch path, final-exponentiated: out576 holds 8 x 576 bytes -- split lines +
 * accumulation (G = 2), fused (G = 2), fused (G = 1), split (G = 4), the wave-program kernel, split (G = 8),
 * split (G = 4, each step's lines multiplied together first), split (G = 1 on eight lanes per f).
 * 1, or 0 on an invalid encoding. */
int bls_test_miller_forms(bls_ctx* ctx, const uint8_t* g1s48, const uint8_t* g2s96, size_t n, uint8_t* out576);
/* the same through the one-wave-per-message kernel of the per-call path */
int bls_test_hash_to_g2_wide(bls_ctx* ctx, const uint8_t* msgs32, size_t n, uint8_t* out96);
/* intermediate stages of the one-wave hash of one 32-byte message (debugging) */
int bls_test_h2c_wide_stages(bls_ctx* ctx, const uint8_t* msg32, uint8_t* out);
/* bls_test_final_check: the final-exponentiation check (FE(f_0 .. f_{n-1}) == 1) of n <= 64 raw Fp12 values
 * (576 bytes each: 12 little-endian Montgomery Fp in tower order) on the six-wave kernel (wide != 0) or the
 * one-wave lane kernel; *out = 1 / 0.  wide == 2: also the six-wave kernel's stage clocks (wall_clock64, 100 MHz)
 * as 8 uint64 at out + 2 (out then needs room for 18 int32). */
int bls_test_final_check(bls_ctx* ctx, const uint8_t* f576, size_t n, int wide, int32_t* out);

/* bls_test_wide_selftest: nw waves compare the wavefront-cooperative products
 * (bls_wide.h) with the lane form on four inputs each (48-byte big-endian
 * integers < p); bad[w] = bitmask of differing forms, 0 when all agree. */
int bls_test_wide_selftest(bls_ctx* ctx, const uint8_t* in48, size_t nw, int32_t* bad);

/* bls_test_rlc_msm: the RLC batch check's signature MSM on n 96-byte signatures (decoded without subgroup checks;
 * none may be the identity) and n 64-bit scalars, exactly as a FAV batch runs it (sort, bucket folds, bit sums, the
 * affine conversion of the pairs): out holds the 64 bit sums U_b compressed (64 x 96 bytes, c0 00 .. for the
 * identity), U_b = the sum of the sigma_i whose scalar has bit b.  The batch pairs them with -w_b G1, w_b = 2^b
 * below bit 32 and 2^(b - 32) lambda above, so S = sum_b w_b U_b is left to the caller.  run_len: entries per bucket
 * run, 0 = the batch's own choice for n items.  Uses the FAV batch's scratch: not between a batch's partial and
 * finish calls.  1, or 0 on an invalid encoding. */
int bls_test_rlc_msm(bls_ctx* ctx, const uint8_t* sigs96, const uint64_t* scalars, size_t n, uint32_t run_len,
                     uint8_t* out);

#ifdef __cplusplus
}
#endif
#endif /* BLSMI355X_H */
