// Host-side launchers for the gfx950 kernels in bls_kernels.hip.
#pragma once
#include "bls_ops.h"

namespace bls {

hipError_t launch_key_validate(hipStream_t st, const uint8_t* pks, size_t n, G1A* out, int* ok);
// the same kernel writing RegKey records (verdict in REG_VALID, a failed key zeroed) straight from the key bytes:
// the key table of a keys batch; valid (nullable): the verdicts as bytes (bls_key_out.h)
hipError_t launch_key_records(hipStream_t st, const uint8_t* pks, size_t n, RegKey* rec, uint8_t* valid);
// SSZ signing roots of n deposits (bls_ssz.hip): five 64-byte SHA-256 nodes per lane
hipError_t launch_deposit_roots(hipStream_t st, const uint8_t* pks48, const uint8_t* wc32, const uint64_t* amounts,
                                const uint8_t* domain32, size_t n, uint8_t* out32);
hipError_t launch_sig_validate(hipStream_t st, const uint8_t* sigs, size_t n, G2A* out, int* ok);
hipError_t launch_g1_sum_aff(hipStream_t st, const G1A* in, const int* ok, size_t n, G1J* tmp, G1J* out);
hipError_t launch_g2_sum_aff(hipStream_t st, const G2A* in, const int* ok, size_t n, G2J* tmp, G2J* out);
hipError_t launch_g1_compress(hipStream_t st, const G1J* in, uint8_t* out48, int* is_inf);
hipError_t launch_g2_compress(hipStream_t st, const G2J* in, uint8_t* out96);
hipError_t launch_percall_pairs(hipStream_t st, const G1A* keys, const int* key_ok, size_t n, const G1J* apk_sum,
                                const int* sig_ok, G1A* P, int* live, Fp* pz = nullptr);
hipError_t launch_hash_many(hipStream_t st, const uint8_t* msgs, const uint64_t* offs, size_t n, const uint8_t* dst, uint32_t dst_len, G2A* out);
hipError_t launch_sign_many(hipStream_t st, const uint8_t* sks, const uint8_t* msgs, const uint64_t* offs, size_t n, uint8_t* out, int* ok);
hipError_t launch_sk_to_pk_many(hipStream_t st, const uint8_t* sks, size_t n, uint8_t* out, int* ok);
// the registry gather (k_fav_gather_q: two keys per step, the pair summed first): 4 lanes per aggregate from 4,096
// aggregates up, 16 from 1,024 up, else 64
hipError_t launch_fav_gather(hipStream_t st, const uint32_t* idx, const uint64_t* offs, size_t B, const RegKey* reg, uint32_t reg_n, G1P* apk, int* status);
// the affine gather (bls_gather_aff.hip) for batches of >= 4,096 aggregates: scratch of fav_gather_aff_words(B) u32,
// redo[B] (1 = recompute with launch_fav_gather_redo, the complete-formula kernel on the flagged aggregates only)
size_t fav_gather_aff_words(size_t B);
hipError_t launch_fav_gather_aff(hipStream_t st, const uint32_t* idx, const uint64_t* offs, size_t B,
                                 const RegKey* reg, uint32_t reg_n, G1P* apk, int* status, uint32_t* scr, int* redo);
hipError_t launch_fav_gather_redo(hipStream_t st, const uint32_t* idx, const uint64_t* offs, size_t B,
                                  const RegKey* reg, uint32_t reg_n, G1P* apk, int* status, const int* redo);
// committee-bitfield batches (bls_gather_bits.hip, bls_g1_bits.h): one wave per item expands (committees, bits) into
// the list of registry indices the gather adds -- the participants, or for a complement item the non-participants --
// at list[slot_offs[b] ..), with the item's record (length, form, malformed);
// the gather variant then sums each list and, for complement items, subtracts it from the committees' sums csum.
// members_ok (nullable): 1 iff every listed key was in range and valid (the committee table's cstat)
struct BitsItem;
hipError_t launch_bits_expand(hipStream_t st, size_t B, int mode, const uint32_t* comm_ids, const uint64_t* comm_offs,
                              const uint8_t* bits, const uint64_t* bit_offs, const uint64_t* slot_offs,
                              const uint32_t* tab_idx, const uint64_t* tab_offs, const int* cstat, uint32_t* list,
                              BitsItem* items);
hipError_t launch_fav_gather_bits(hipStream_t st, const uint32_t* list, const BitsItem* items, size_t B,
                                  const RegKey* reg, uint32_t reg_n, const uint32_t* comm_ids,
                                  const uint64_t* comm_offs, const G1P* csum, G1P* apk, int* status,
                                  int* members_ok);
// registry entries from k_key_validate output (+ the host validity mask)
hipError_t launch_reg_pack(hipStream_t st, const G1A* a, const int* ok, size_t n, RegKey* reg, uint8_t* valid);
hipError_t launch_av_items(hipStream_t st, size_t B, const uint64_t* io, const int* pk_ok, const int* sig_ok, const G2A* sig, const uint64_t* rsc, int* status, G1A* P2, G2A* Q2);
hipError_t launch_av_pairs(hipStream_t st, size_t total, const uint32_t* pair_item, const int* status, const uint64_t* rsc, const G1A* pk, const G2A* H, G1A* P2, G2A* Q2);
// out[b] = product of in[io[b] + b .. io[b + 1] + b] (the AggregateVerify batch's per-item segments)
hipError_t launch_fp12_seg_prod(hipStream_t st, const Fp12* in, const uint64_t* io, size_t B, Fp12* out);
// SHA-256 of 64-byte nodes (bls_ssz.hip): signing roots and SSZ merkleization
hipError_t launch_sha256_pairs(hipStream_t st, const uint8_t* left, const uint8_t* right, size_t rstride, size_t n,
                               uint8_t* out);
hipError_t launch_merkleize(hipStream_t st, uint8_t* a, uint8_t* b, size_t n, int depth, uint8_t* zero, uint8_t** root);
// KZG: checked G1 decode (identity allowed), per-point scalar products for multi_exp
hipError_t launch_g1_decode_checked(hipStream_t st, const uint8_t* in48, size_t n, G1A* out, int* ok);
hipError_t launch_g1_scale(hipStream_t st, const G1A* P, const uint8_t* k32, size_t n, G1A* out, int* live);
hipError_t launch_verdicts(hipStream_t st, const int* status, const uint8_t* bad, size_t B, uint8_t* out);
hipError_t launch_status_to_u8(hipStream_t st, const int* status, size_t B, uint8_t* out);
hipError_t launch_fp12_to_bytes(hipStream_t st, const Fp12* f, uint8_t* out);
hipError_t launch_fp12_from_bytes(hipStream_t st, const uint8_t* in, size_t n, Fp12* f);
hipError_t launch_g2_compress_aff(hipStream_t st, const G2A* in, uint8_t* out96);
hipError_t launch_registry_generate(hipStream_t st, uint64_t first, size_t n, G1J* tmpJ, RegKey* reg, uint8_t* out48);
hipError_t launch_miller_wave(hipStream_t st, const G1A* P, const G2A* Q, const int* ok, size_t n, Fp12* f);
constexpr int HCF = 24;  // hash_to_G2 staging: Fd slots per item (bls_fav_kernels.hip, bls_chain_lane.hip)
// one lane per item (bls_chain_lane.hip)
// gstat: gather status (read-only: the MSM reads it concurrently on another stream); status: written
hipError_t launch_sig_lane(hipStream_t st, size_t B, const int* gstat, int* status, const int* dstat, const G1P* apk,
                           const G2A* sig, const uint64_t* rsc, G1P* rPj);
// hf: h2c_scratch_fd(B) Fd slots of staging between the hash_to_G2 phases
size_t h2c_scratch_fd(size_t B);
hipError_t launch_h2c(hipStream_t st, size_t B, const uint8_t* msgs32, const int* status, Fd* hf, G2A* H, int* flag);
// hash_to_G2 (POP DST) of B messages of any length, msgs[offs[i] .. offs[i+1]); same phases as launch_h2c
hipError_t launch_h2c_msgs(hipStream_t st, size_t B, const uint8_t* msgs, const uint64_t* offs, Fd* hf, G2A* H,
                           int* flag);
// exceptional h2c items (flag set: an isogeny denominator vanished) recomputed by one workgroup; offs == nullptr
// for 32-byte messages.  Not part of launch_h2c / launch_h2c_msgs: the caller picks its stream (bls_capi_ctx.hip).
hipError_t launch_h2c_fallback(hipStream_t st, size_t B, const uint8_t* msgs, const uint64_t* offs, const int* flag,
                               G2A* H);
hipError_t launch_sig_decode(hipStream_t st, size_t B, const uint8_t* msgs32, const uint8_t* sigs96, const uint8_t* seed32, G2A* sig, uint64_t* rsc, int* dstat);
// the same with item i's message at msgs32 + 32 msg_id[i] (a shared-message batch: r_i still hashes the item's own
// number, message and signature)
hipError_t launch_sig_decode_idx(hipStream_t st, size_t B, const uint8_t* msgs32, const uint32_t* msg_id,
                                 const uint8_t* sigs96, const uint8_t* seed32, G2A* sig, uint64_t* rsc, int* dstat);
// rPj: B projective scratch points (r_i apk_i before the affine conversion)
hipError_t launch_sig_vm(hipStream_t st, size_t B, const int* gstat, int* status, const int* dstat, const G1P* apk_aff,
                         const G2A* sig, const uint64_t* rsc, G1P* rPj, G1A* rP);
size_t msm_scratch_u32(size_t B);
size_t msm_scratch_fd(size_t B, uint32_t run_len = 0);
// the 64 bit-sums U_b of S = sum_i r_i sigma_i = sum_b 2^b U_b as Miller pairs (-2^b G1, U_b) at P[0 .. 64),
// Q[0 .. 64), ok[0 .. 64) = 1; comb: the bisection's -G1 comb (neg_g1_comb_entries() entries); scr / pts:
// msm_scratch_u32(B) words / msm_scratch_fd(B, run_len) slots.  run_len: entries per bucket run, 0 = chosen from B
// (every batch; the test hook sets it to reach the run boundaries with few points)
constexpr int MSM_UPAIRS = 64;
hipError_t launch_msm_upairs(hipStream_t st, size_t B, const int* status, const int* status2, const uint64_t* rsc,
                             const G2A* sig, uint32_t* scr, Fd* pts, const G1A* comb, G1A* P, G2A* Q, int* ok,
                             uint32_t run_len = 0);
// the same Miller values in two kernels (G2 lines, then f); L: miller_lines_u32(n) words of scratch
constexpr int MILLER_NLINES = 68;  // 63 doublings + 5 additions (|x| = 0xd201000000010000)
// Miller line records (k_miller_lines2 -> k_miller_acc4q): three Fp2 (l0, l2, l3), the line l0 + l2 (-x_P) v
// + l3 y_P v w up to an Fp2 factor -- (B - E, 3 J, H) for a doubling, (theta x_Q - lambda y_Q, theta, lambda) for an
// addition, bls_miller_lines.h -- as 14-digit bound-typed values (bls_fqb.h FqB<ML_LV, ML_LD>: value < ML_LV p, digits <=
// ML_LD), word w of line k of pair i at L[(k * ML_WORDS + w) * n + i]
constexpr int ML_WORDS = 84;
constexpr uint64_t ML_LV = 4096, ML_LD = 0x20000000ull + 64;
size_t miller_lines_ld(size_t n);  // the records' leading dimension (>= n, a multiple of 32 pairs)
size_t miller_lines_u32(size_t n);
hipError_t launch_miller_lines(hipStream_t st, const G2A* Q, size_t n, uint32_t* L);
// four lanes per f, G = 1 or 2 pairs per f (bls_miller_pair.hip); writes ceil(n / G) values; ld >= n: the
// line records' leading dimension (the n of the launch_miller_lines that wrote them)
hipError_t launch_miller_acc4(hipStream_t st, const G1A* P, const G2A* Q, const int* ok, size_t n, const uint32_t* L,
                              size_t ld, Fp12* f, int G);
// the same with four pairs per f and each round's four lines multiplied together before they meet f
// (k_miller_acc4l); writes ceil(n / 4) values
hipError_t launch_miller_acc4l(hipStream_t st, const G1A* P, const G2A* Q, const int* ok, size_t n, const uint32_t* L,
                               size_t ld, Fp12* f);
// one pair per f on eight lanes (k_miller_acc8, the latency form for small batches); writes n values
hipError_t launch_miller_acc8(hipStream_t st, const G1A* P, const G2A* Q, const int* ok, size_t n, const uint32_t* L,
                              size_t ld, Fp12* f);
// the whole Miller loop of n pairs in one kernel (k_miller_fused: the G2 side and the f accumulation in the same
// workgroup, line records in LDS); G = 1 or 2 pairs per f; writes ceil(n / G) values (conjugated, x < 0)
hipError_t launch_miller_fused(hipStream_t st, const G1A* P, const G2A* Q, const int* ok, size_t n, Fp12* f, int G);
hipError_t launch_final_check_wave(hipStream_t st, const Fp12* f, int n, int* out);
// one bisection-tree level: node b is checked (res[b] = FE(node[b]) == 1, ++*nchecks) when parent is null or
// parent[b / pdiv] == 0, else res[b] = 1 (bls_fe.hip k_fe_check_gated)
hipError_t launch_final_check_gated(hipStream_t st, const Fp12* node, size_t n, const int* parent, uint32_t pdiv,
                                    int* res, uint32_t* nchecks);
// the same on the six-wave kernel (k_fe_wide)
hipError_t launch_fe_wide_gated(hipStream_t st, const Fp12* node, size_t n, const int* parent, uint32_t pdiv, int* res,
                                uint32_t* nchecks);
// out[b] = prod_{i in [b chunk, (b + 1) chunk) and < n} a[i] b[i]
hipError_t launch_fp12_chunk_prod2(hipStream_t st, const Fp12* a, const Fp12* b, size_t n, int chunk, Fp12* out);
// bisection fallback (bls_bisect.hip): the -G1 comb table (neg_g1_comb_entries() G1A), -r_i G1 in affine (tmp: B
// projective scratch points), verdicts from the leaf results
size_t neg_g1_comb_entries();
hipError_t launch_neg_g1_comb_table(hipStream_t st, G1A* tab);
hipError_t launch_neg_rg1(hipStream_t st, size_t B, const int* status, const uint64_t* rsc, const G1A* tab, G1P* tmp,
                          G1A* out);
hipError_t launch_verdicts_res(hipStream_t st, const int* status, const int* res, size_t B, uint8_t* out);
// projective -> affine with one inversion per 8 items (k_g1_affine_b); status-0 items -> identity
hipError_t launch_g1_affine(hipStream_t st, size_t B, const int* status, const G1P* Pj, G1A* out);
// shared-message batches (bls_segsum.hip): one level of the segmented G1 sum (bls_g1_segsum.h; level 0 reads the
// items' affine rP through `items`, the levels above the partials `prev` of the level below; non-final runs write
// `tmp`, final runs gsum[group] and ok[group] = sum != identity), and the bisection's H_item[i] = H[msg_id[i]]
struct SegRun;
hipError_t launch_g1_seg_fold(hipStream_t st, int level, const SegRun* runs, uint32_t nruns, const uint32_t* items,
                              const int* status, const G1A* rP, const G1P* prev, G1P* tmp, G1P* gsum, int* ok);
hipError_t launch_g2a_gather(hipStream_t st, size_t B, const G2A* H, const uint32_t* msg_id, G2A* out);
// grouped signature aggregation (bls_segsum.hip): one level of the segmented G2 sum (bls_g2_segsum.h; level 0 reads
// the decoded members a / ok through `items`, skipping those outside the nullable mask `include`; the levels above
// read the partials `prev`; non-final runs write `tmp`, final runs gsum[group]), and the finish: G sums to
// compressed bytes and ok (one inversion per 4 groups).  Partials are g2_seg_partial_bytes() each.
struct G2SP;
size_t g2_seg_partial_bytes();
hipError_t launch_g2_seg_fold(hipStream_t st, int level, const SegRun* runs, uint32_t nruns, const uint32_t* items,
                              const int* ok, const uint8_t* include, const G2A* a, const G2SP* prev, G2SP* tmp,
                              G2SP* gsum);
hipError_t launch_g2_seg_finish(hipStream_t st, size_t G, const G2SP* gsum, uint8_t* out96, uint8_t* out_ok);
// nsel independent checks: out[b] = (FE(f[sel[b]]) == 1)
hipError_t launch_final_check_sel(hipStream_t st, const Fp12* f, const uint32_t* sel, size_t nsel, int* out);
hipError_t launch_fp12_chunk_prod(hipStream_t st, const Fp12* in, size_t n, int chunk, Fp12* out);
hipError_t launch_fp12_prod_vm(hipStream_t st, const Fp12* in, size_t n, Fp12* tmp, Fp12* out);
// out[b] = prod in[b chunk .. (b + 1) chunk) with the final exponentiation's lane-parallel product (bls_fe.hip)
hipError_t launch_fp12_chunk_prod_fe(hipStream_t st, const Fp12* in, size_t n, int chunk, Fp12* out);
hipError_t launch_fp12_chunk_prod2_fe(hipStream_t st, const Fp12* a, const Fp12* b, size_t n, int chunk, Fp12* out);
hipError_t launch_fp12_seg_prod_fe(hipStream_t st, const Fp12* in, const uint64_t* io, size_t B, Fp12* out);

// curve objects (bls_points.hip): group 1 = G1 (48-B encodings, G1A), 2 = G2 (96-B, G2A)
hipError_t launch_pt_decode(hipStream_t st, int group, const uint8_t* in, size_t n, int subgroup, void* out, int* ok);
// op 0: a + b, op 1: [k32] a; *ok = 0 if an encoding is invalid
hipError_t launch_pt_binop(hipStream_t st, int group, const uint8_t* a, const uint8_t* b, const uint8_t* k32, int op,
                           uint8_t* out, int* ok);
size_t pt_msm_scratch_bytes(int group, size_t n);
hipError_t launch_pt_msm(hipStream_t st, int group, const void* P, const uint8_t* k32, size_t n, void* tmp,
                         uint8_t* out);
hipError_t launch_gt_final_exp(hipStream_t st, const Fp12* f, uint8_t* out576);
hipError_t launch_gt_mul(hipStream_t st, const uint8_t* a, const uint8_t* b, uint8_t* out);

// resident G1 table and its batched bucket MSM (bls_g1_table.hip, bls_g1_msm.h).  The table holds 32 window-major
// RegKey records per entry (record w * cap + i = 2^(8w) T[i], REG_VALID on usable non-identity points) and a state
// byte per entry (0 invalid, 1 point, 2 identity).
// launch_g1_table_fill: entries first .. first + n from decoded points a / ok; cur (n G1P), live (n), aff (n G1A):
// scratch; out_ok[i] = the encoding's verdict.
hipError_t launch_g1_table_fill(hipStream_t st, const G1A* a, const int* ok, size_t n, RegKey* tab, size_t cap,
                                size_t first, uint8_t* stat, G1P* cur, int* live, G1A* aff, uint8_t* out_ok);
// what an MSM of B vectors over n items needs: bucket slots, the most entries, the fold's levels with the most runs
// of each (its grids), the two partial arrays (G1P each) and the u32 scratch
struct G1MsmPlan {
  uint32_t slots;
  size_t entries, u32_words, part[2], level_runs[8];
  int levels;
};
G1MsmPlan g1_msm_plan(size_t n, size_t B);
// out48[v] = sum_i [k32[v n + i]] T[idx[i]] (compressed), v < B; every idx names a valid entry; k32 16-byte aligned;
// U: 8 B, res: B G1P, live: B, aff: B G1A; *d_entries: where the device leaves the number of bucket entries
hipError_t launch_g1_table_msm(hipStream_t st, const G1MsmPlan& p, const RegKey* tab, uint32_t cap,
                               const uint8_t* stat, const uint32_t* idx, uint32_t n, uint32_t B, const uint8_t* k32,
                               uint32_t* scr, G1P* partA, G1P* partB, G1P* U, G1P* res, int* live, G1A* aff,
                               uint8_t* out48, const uint32_t** d_entries);
// The bucket MSM over a call's own points (bls_g1_var_msm.h): res / aff / out48[v] = sum_i [k32[v n + i]] pts[i],
// v < B, integer multiples.  pts / ok: n decoded points and their usability flags (a point with ok = 0 is dropped like
// the identity: the caller refuses invalid encodings first); k32 16-byte aligned.  The plan has 8,192 B slots and a
// fullest bucket of n entries.  rec: n records, plive: n; scr / partA / partB as the plan says; U: 256 B, W: 32 B G1P,
// wlive: 32 B; res: B G1P (canonical projective), live: B (0 for the identity), aff: B G1A; out48 (nullable): the
// compressed bytes; d_entries (nullable) as above.  Everything stays on the device and on st.
G1MsmPlan g1_var_msm_plan(size_t n, size_t B);
hipError_t launch_g1_var_msm(hipStream_t st, const G1MsmPlan& p, const G1A* pts, const int* ok, uint32_t n,
                             uint32_t B, const uint8_t* k32, RegKey* rec, int* plive, uint32_t* scr, G1P* partA,
                             G1P* partB, G1P* U, G1P* W, int* wlive, G1P* res, int* live, G1A* aff, uint8_t* out48,
                             const uint32_t** d_entries);

// Deneb blob KZG on F_r (bls_kzg.hip; lane pieces bls_kzg_blob.h, field bls_fr.h).  Fr: 32 B, Montgomery form.
// dom: the 4,096 domain entries omega^brp(i) (kzg_domain_bytes()); f: 4,096 elements per blob; ok[b] = every element
// of blob b is < r (a failing element is stored as 0)
struct Fr;
size_t kzg_domain_bytes();
hipError_t launch_fr_domain(hipStream_t st, Fr* dom);
hipError_t launch_blob_decode(hipStream_t st, const uint8_t* blobs, size_t B, Fr* f, int* ok);
// n 32-byte big-endian scalars: out[i] in Montgomery form and ok[i] = (scalar < r)
hipError_t launch_fr_decode(hipStream_t st, const uint8_t* in32, size_t n, Fr* out, int* ok);
// y[b] = p_b(z[b]) (also as 32 big-endian bytes), hit[b] = the domain index z[b] equals, or -1; ok nullable: a blob
// with ok[b] = 0 gives y = 0; pre: 4,096 B elements of scratch (the lanes' prefix products)
hipError_t launch_blob_eval(hipStream_t st, const Fr* dom, const Fr* f, const Fr* z, const int* ok, size_t B, Fr* pre,
                            Fr* y, uint8_t* y32, int* hit);
// q32: B rows of 4,096 32-byte scalars, the evaluation form of (p_b(X) - y[b]) / (X - z[b]); hit: launch_blob_eval's
hipError_t launch_blob_quotient(hipStream_t st, const Fr* dom, const Fr* f, const Fr* z, const Fr* y, const int* hit,
                                size_t B, Fr* pre, uint8_t* q32);
// a verification batch's scalars and points: P holds the n decoded commitments, then the n proofs; the kernel adds
// G1 at P[2 n] and the proofs again at P[2 n + 1 ..), and writes the 3 n + 1 scalar rows r_i | r_i z_i |
// -sum r_i y_i | r_i (r_i: 128 bits from seed32 and i)
hipError_t launch_kzg_rlc(hipStream_t st, const uint8_t* seed32, size_t n, const Fr* z, const Fr* y, G1A* P,
                          uint8_t* k32);
// P / Q[0 .. 2): (sums[1], negtau), (sums[0], G2)
hipError_t launch_kzg_pairs(hipStream_t st, const G1J* sums, const G2A* negtau, G1A* P, G2A* Q);
// P / Q[2 i], [2 i + 1]: (pi_i, negtau), (C_i + [z_i] pi_i - [y_i] G1, G2); CP: commitments, then proofs
hipError_t launch_kzg_item_pairs(hipStream_t st, size_t n, const G1A* CP, const Fr* z, const Fr* y,
                                 const G2A* negtau, G1A* P, G2A* Q);
hipError_t launch_kzg_g2_neg(hipStream_t st, G2A* q);  // *q = -*q

// Fulu cell KZG on F_r (bls_kzg_cells.hip; the transform's pieces: bls_fr_ntt.h).  tab: w^i | 7^i | 7^-i, 8,192
// entries each (ntt_tables_bytes()), w = 7^((r - 1) / 8192)
size_t ntt_tables_bytes();
hipError_t launch_ntt_tables(hipStream_t st, Fr* tab);
// B transforms of 2^logn points (logn 12 or 13): blob b reads src + b src_stride and writes dst + b dst_stride (dst
// may be src); tmp: B 2^logn entries.  flags: NTT_INV | NTT_SRC_BRP | NTT_DST_BRP; inputs from index `limit` on read
// as zero (bls_fr_ntt.h)
hipError_t launch_ntt(hipStream_t st, const Fr* W, uint32_t logn, uint32_t flags, uint32_t limit, size_t B,
                      const Fr* src, size_t src_stride, Fr* tmp, Fr* dst, size_t dst_stride);
// cells: B x n_present x 2,048 bytes, cell p of every blob at index idx[p] < 128; ext (B x 8,192, zeroed before) gets
// the elements at 64 idx[p] + j, bad[b] (zeroed before) = 1 if an element of blob b is not below r
hipError_t launch_cells_scatter(hipStream_t st, const uint8_t* cells, const uint32_t* idx, uint32_t n_present, size_t B,
                                Fr* ext, int* bad);
// present: 128 flags; zd[m] = Z(w^m) and zci[m] = 1 / Z(7 w^m), m < 128, Z the vanishing polynomial of the missing
// cells' cosets
hipError_t launch_cells_vanish(hipStream_t st, const uint8_t* present, const Fr* W, Fr* zd, Fr* zci);
// dst[b][i] = src[b][brp ? brp13(i) : i] mul[i & mask], i < dst_n <= 8,192 (src: 8,192 per blob, dst: dst_n; dst may
// be src when dst_n = 8,192 and brp is false)
hipError_t launch_cells_pointwise(hipStream_t st, const Fr* src, Fr* dst, uint32_t dst_n, size_t B, bool brp,
                                  const Fr* mul, uint32_t mask);
hipError_t launch_fr_encode(hipStream_t st, const Fr* in, size_t n, uint8_t* out32);
// n cells (2,048 bytes each) with cell indices kidx: coef[k] = the 64 coefficients of cell k's interpolation polynomial;
// cok[k] = every element < r and kidx[k] < 128
hipError_t launch_cells_interp(hipStream_t st, const uint8_t* cells, const uint32_t* kidx, size_t n, const Fr* W,
                               Fr* coef, int* cok);
// A cell batch's scalars and points.  P holds the nc decoded commitments, then the n proofs; the kernels add the
// identity at P[nc + n] and the proofs again behind it, and write the nc + 2 n + 1 scalar rows: commitment i's sum of
// the r_k of its items (cidx) | r_k h_k^64 | 0 | r_k (r_k: 128 bits from seed32 and k), and rli32, the 64 rows
// -sum_k r_k c_{k,m}.  rfr: n elements; part: 64 cells_colsum_groups(n) elements
size_t cells_colsum_groups(size_t n);
hipError_t launch_cells_rlc(hipStream_t st, const uint8_t* seed32, size_t nc, size_t n, const uint32_t* cidx,
                            const uint32_t* kidx, const Fr* W, const Fr* coef, Fr* rfr, Fr* part, G1A* P, uint8_t* k32,
                            uint8_t* rli32);
hipError_t launch_cells_put(hipStream_t st, const G1A* aff, const int* aff_live, G1A* S, int* live);  // *S, *live = ...
// P / Q[2 k], [2 k + 1]: (pi_k, negtau64), (C_k - I_k + [h_k^64] pi_k, G2); CP: nc commitments, then n proofs
hipError_t launch_cells_item_pairs(hipStream_t st, size_t nc, size_t n, const G1A* CP, const uint32_t* cidx,
                                   const uint32_t* kidx, const G1A* I, const Fr* W, const G2A* negtau64, G1A* P,
                                   G2A* Q);

// The transform over G1 and the cell proofs' rows (bls_g1_fft.hip; pieces and derivation: bls_g1_fft.h).  buf: B
// vectors of 2^logn canonical projective points (1 <= logn <= 12), W: launch_ntt_tables' table.
// launch_g1fft_load: vector v's entries 0 .. have are src[v have ..] (the identity where live, nullable, is 0), the
// rest the identity.  launch_g1fft: logn stages in place, natural order in, bit-reversed order out; the inverse
// includes 1 / n.  launch_g1fft_finish: out = buf in bit-reversed (as it stands) or natural order, live, aff and
// out48 its B 2^logn live flags, affine forms and encodings
hipError_t launch_g1fft_load(hipStream_t st, const G1A* src, const int* live, uint32_t have, uint32_t logn, size_t B,
                             G1P* buf);
hipError_t launch_g1fft(hipStream_t st, const Fr* W, uint32_t logn, bool inverse, size_t B, G1P* buf);
hipError_t launch_g1fft_finish(hipStream_t st, const G1P* buf, uint32_t logn, size_t B, bool natural, G1P* out,
                               int* live, G1A* aff, uint8_t* out48);
// rows32: per blob 63 rows of 4,032 32-byte big-endian scalars, row m = coef[64 (m + 1) + i], zero from 4,096 on
// (coef: 4,096 Montgomery elements per blob)
size_t cellproof_rows_per_blob();
size_t cellproof_row_entries();
hipError_t launch_cellproof_rows(hipStream_t st, const Fr* coef, size_t B, uint8_t* rows32);

// wavefront-cooperative arithmetic (bls_wide.hip)
hipError_t launch_wide_selftest(hipStream_t st, size_t nw, const uint8_t* be48, int* bad);
// hash_to_G2 with one wave per message (msgs 32 B apart when offs is null); flag[i] = 1: recompute on the fallback;
// Hz: H in Jacobian coordinates (Z in Hz, 1 for flagged items) instead of affine
hipError_t launch_h2c_wide(hipStream_t st, size_t B, const uint8_t* msgs, const uint64_t* offs, G2A* H, int* flag,
                           Fp2* Hz = nullptr);
hipError_t launch_h2c_wide_dbg(hipStream_t st, const uint8_t* msg32, Fp* out);
// signature decode + subgroup check with one wave per signature (k_sig_validate semantics)
hipError_t launch_sig_validate_wide(hipStream_t st, const uint8_t* sigs, size_t n, G2A* out, int* ok);
// the whole Miller loop of npairs <= 2 pairs on one workgroup (line waves + six f waves): out = f (tower Fp12);
// ok0 / ok1 (nullable): pair 0 / 1 runs with constant lines unless *okp; qz (nullable): the pairs' Q are Jacobian
// (X, Y in Q, Z in qz; the f differs from the affine Q's by an Fp2 factor: the same final exponentiation)
// pz (nullable): the pairs' P are Jacobian (X, Y in P, Z in pz; the lines scaled by Z^3, an Fp factor)
hipError_t launch_miller_wide(hipStream_t st, const G1A* P, const G2A* Q, const int* ok0, const int* ok1, int npairs,
                              Fp12* out, const Fp2* qz = nullptr, const Fp* pz = nullptr);
// n pairs on miller_wide_nf(n) = ceil(n / 2) workgroups of the per-call kernel: out[0 .. miller_wide_nf(n)) (ok per
// pair, or nullptr)
size_t miller_wide_nf(size_t n);
hipError_t launch_miller_wide_n(hipStream_t st, const G1A* P, const G2A* Q, const int* ok, size_t n, Fp12* out,
                                const Fp2* qz = nullptr);
// final-exponentiation check of the product of f[0 .. n): easy part lane-parallel, hard part on six waves (F2)
hipError_t launch_fe_wide(hipStream_t st, const Fp12* f, int n, int* out, uint64_t* ts = nullptr);  // ts: stage clocks (tests)
// KeyValidate with two keys per wave (k_key_validate semantics)
hipError_t launch_key_validate_wide(hipStream_t st, const uint8_t* pks, size_t n, G1A* out, int* ok);
// ... writing RegKey records (launch_key_records on the wide kernel)
hipError_t launch_key_records_wide(hipStream_t st, const uint8_t* pks, size_t n, RegKey* rec, uint8_t* valid);
// the checked G1 decode (identity accepted, k_pt_decode semantics) on the wide KeyValidate kernel
hipError_t launch_g1_decode_checked_wide(hipStream_t st, const uint8_t* in48, size_t n, G1A* out, int* ok);

}  // namespace bls
