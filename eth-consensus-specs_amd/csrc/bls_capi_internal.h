// What the pieces of the C ABI (csrc/bls_capi*.hip; declared in include/blsmi355x.h) share: the context and its
// jobs, the scratch arena, the error / profile / entry macros, and the helpers more than one piece calls.  Host
// code: argument checks, H2D/D2H copies into a per-context scratch arena, kernel launches on the context's
// streams.  No compute happens on the host.
#pragma once
#include <mutex>
#include <new>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include <rccl/rccl.h>

#include "../../include/blsmi355x.h"
#include "bls_kernels.h"
#define BLS_SEGSUM_PLAN_ONLY  // the host plan of the segmented G1 sum; its kernels are in bls_segsum.hip
#include "bls_g1_segsum.h"
#include "bls_g1_bits.h"

using namespace bls;

enum Slot {
  S_IN0, S_IN1, S_IN2, S_IN3, S_OFFS, S_G1A, S_G2A, S_G2A_B, S_OK, S_G1J, S_G1J_T, S_G2J, S_G2J_T, S_F, S_F_T, S_INT,
  S_PC_PZ,
  // FAV batch state (kept between partial and finish)
  S_FAV_F, S_FAV_FT, S_APK, S_STATUS, S_GSTAT, S_APKA, S_SIG, S_RP, S_RS, S_H, S_FPART, S_SEED, S_BYTES, S_FCHK, S_FLAG, S_RSC, S_MSMU, S_MSMF, S_MSTAT, S_HCF, S_RPJ, S_MLINES,
  // bisection fallback (fav_bisect)
  S_BP, S_BQ, S_BS, S_BT, S_BSEL, S_BRES, S_BBAD, S_BSIG, S_BRSC,
  // AggregateVerify batches (own slots: a FAV batch may be between its partial and finish calls)
  S_AV_IO, S_AV_RSC, S_AV_PITEM, S_AV_SIG, S_AV_SOK, S_AV_H, S_AV_ST, S_AV_P, S_AV_Q, S_AV_F, S_AV_FT, S_AV_SEL,
  S_AV_FI, S_AV_RES, S_AV_HCF, S_AV_FLAG,
  // signing roots / merkleization
  S_SZ_A, S_SZ_B, S_SZ_C, S_SZ_Z,
  // KZG pieces
  S_KZ_IN, S_KZ_P, S_KZ_Q, S_KZ_OK, S_KZ_OK2, S_KZ_F, S_KZ_FT, S_KZ_S, S_KZ_J, S_KZ_OUT,
  // curve objects (bls_g1_* / bls_g2_* / bls_multi_exp / bls_multi_pairing / bls_gt_mul)
  S_PT_IN, S_PT_A, S_PT_OK, S_PT_TMP, S_PT_OUT,
  // per-call Verify / FastAggregateVerify pair points (not S_RP: a FAV batch's r_i apk_i live there between its
  // partial and finish calls, and fav_bisect reads them back)
  S_PC_P,
  S_OWN,  // the job's own final check (enqueue_own_check)
  // the job's product again, for an own check that runs on demand (job_submit with the device exchange, read_own):
  // S_FPART is every per-call product's slot too, and such calls may come between the submit and the finish
  S_OWN_F,
  S_GAFF, S_GREDO,  // the affine gather's level lists and redo flags (bls_gather_aff.hip)
  S_COMM, S_CV,  // the all-gathered partials of all ranks and their check's verdict (enqueue_comm_check)
  // shared-message batches (FavItems::msg_id): the pair arrays' status and G1 side (M + MSM_UPAIRS; the
  // G2 side is S_H), the group sums before the affine conversion, the fold's two partial arrays, its runs and sorted
  // item list, the items' message ids, and the bisection's per-item H
  S_PSTAT, S_GP, S_GSUM, S_SEGA, S_SEGB, S_SEGRUN, S_SEGIT, S_MSGID, S_BHIT,
  // grouped signature aggregation (bls_aggregate_grouped; own slots: a FAV batch may be between its partial and
  // finish calls): staged signatures, mask and outputs of the host-buffer call, the decoded members and their ok,
  // the fold's runs, sorted item list, two partial arrays and the group sums
  S_AGG_IN, S_AGG_INC, S_AGG_OUT, S_AGG_A, S_AGG_OK, S_AGG_RUN, S_AGG_IT, S_AGG_PA, S_AGG_PB, S_AGG_SUM,
  // committee-bitfield batches (FavItems::bits): the job's host tables in one piece (the three offset tables
  // -- committees | bit bytes | list slots, B + 1 each -- then the items' committee ids), the expanded index lists
  // and the item records
  S_BTAB, S_BLIST, S_BITEM,
  // key-table batches (FavItems::keys): the job's own table of RegKey records, decoded and KeyValidated from the
  // batch's key bytes (at least one record: the gather's unconditional load of record 0), and for the host-buffer
  // entry points the uploaded key bytes and the verdict bytes that go back
  S_KTAB, S_KEYS_IN, S_KVALID,
  // resident G1 table (bls_capi_msm.hip).  A load: the uploaded encodings, the decoded points and verdicts, the
  // running projective points, their live flags and affine forms, the verdict bytes.  An MSM: the scalars and
  // indices, the sort's counters, offsets and lists, the fold's two partial arrays, the bit sums, the results
  // (projective, live, affine) and the output bytes
  S_G1T_IN, S_G1T_A, S_G1T_OK, S_G1T_CUR, S_G1T_LIVE, S_G1T_AFF, S_G1T_VERD,
  S_G1M_IN, S_G1M_U32, S_G1M_PA, S_G1M_PB, S_G1M_U, S_G1M_RES, S_G1M_LIVE, S_G1M_AFF, S_G1M_OUT,
  // blob KZG (bls_capi_kzg.hip).  Blobs: the uploaded bytes, the elements, the lanes' prefix products, the per-blob
  // verdicts, the z / y bytes, their elements and verdicts, the in-domain indices, the quotient rows.
  // Verification: the encodings, the
  // 3 n + 1 points, their verdicts, scalar rows, products and live flags, the sums' scratch and the two sums, the
  // seed, the pairs, their Miller values, the per-item checks' selection and results
  S_KB_BLOB, S_KB_F, S_KB_PRE, S_KB_OK, S_KB_Z32, S_KB_Y32, S_KB_ZF, S_KB_YF, S_KB_ZOK, S_KB_YOK, S_KB_HIT, S_KB_Q,
  S_KB_ENC, S_KB_P, S_KB_POK, S_KB_K, S_KB_S, S_KB_LIVE, S_KB_J, S_KB_SUM, S_KB_SEED, S_KB_PP, S_KB_PQ, S_KB_FV,
  S_KB_SEL, S_KB_RES,
  // cell KZG (bls_capi_kzg_cells.hip).  Cells: the uploaded bytes, the index list and presence flags, the extended
  // blobs (two buffers the recovery alternates between), the transform's intermediate, the coefficient form (kept
  // after a call), the vanishing polynomial's values and inverses, the per-blob verdicts, the output bytes
  S_KC_IN, S_KC_IDX, S_KC_PRES, S_KC_X, S_KC_Y, S_KC_T, S_KC_COEF, S_KC_ZD, S_KC_ZCI, S_KC_BAD, S_KC_OUT,
  // ... verification: the encodings, the commitment and cell indices, the nc + 2 n + 1 points, their verdicts, the
  // cells' verdicts and interpolation coefficients, the r_k, the column sums' partials and rows, the scalar rows,
  // products and live flags, the sums' scratch and the two sums, the seed, the pairs, their Miller values, the
  // per-item checks' selection and results, the interpolants' scalar rows and commitments
  S_KC_ENC, S_KC_CIDX, S_KC_KIDX, S_KC_P, S_KC_POK, S_KC_COK, S_KC_CF, S_KC_RFR, S_KC_PART, S_KC_RLI, S_KC_K, S_KC_S,
  S_KC_LIVE, S_KC_J, S_KC_SUM, S_KC_SEED, S_KC_PP, S_KC_PQ, S_KC_FV, S_KC_SEL, S_KC_RES, S_KC_ROWS, S_KC_I,
  // cell proofs and the G1 transform (bls_capi_kzg_cells.hip): the uploaded encodings, the decoded points and their
  // verdicts, the scalar rows of one table MSM, the transform's buffer (the h_m of every blob: an MSM's results are
  // copied out of the S_G1M_* slots before the next one), the buffer in output order, its live flags, affine forms
  // and encodings
  S_KP_IN, S_KP_A, S_KP_OK, S_KP_ROWS, S_KP_BUF, S_KP_PERM, S_KP_LIVE, S_KP_AFF, S_KP_OUT,
  // bucket MSM over a call's own points (bls_g1_msm, bls_capi_msm.hip): the scalars and encodings, the decoded points
  // and verdicts, their records and live flags, the sort's counters, offsets and lists, the fold's two partial
  // arrays, the bit sums, the window sums and their flags, the results (projective, live, affine), the output bytes
  S_GV_IN, S_GV_A, S_GV_OK, S_GV_REC, S_GV_PLIVE, S_GV_U32, S_GV_PA, S_GV_PB, S_GV_U, S_GV_W, S_GV_WLIVE, S_GV_RES,
  S_GV_LIVE, S_GV_AFF, S_GV_OUT,
  NSLOT
};

struct Buf {
  void* p = nullptr;
  size_t cap = 0;
};

// A job's events, all hipEventDisableTiming, created with its streams before any kernel runs.
enum JobEvent {
  EV_FORK, EV_JOIN, EV_SIG, EV_MSM, EV_GATHER,
  EV_PARTIAL,  // the batch's 576-byte partial is in h_partial
  EV_H2C, EV_FB, EV_FE,  // hand-offs to the context-wide aux streams
  // a bisection has copied what it reads of the batch state that stream2 / stream3 overwrite: the job's next batch
  // starts its hash and signature branches from here instead of after the whole bisection (fav_prepare)
  EV_BIS,
  EV_OWN,  // h_own[0] is written
  EV_COMM, EV_CV,  // the partials are all-gathered; h_own[1] is written
  EV_BITS,  // the last upload of bits_tab has been read
  EV_N
};

// Per-batch device state, streams and events.  A context owns
// BLS_FAV_JOBS of them so that consecutive FAV batches can be in flight
// together (bls_fav_job_*): batch k+1's front kernels fill the GPU while
// batch k's Miller product is final-exponentiated.  The per-call API and the
// registry use job 0.
struct Job {
  hipStream_t stream = nullptr;
  hipStream_t stream2 = nullptr;  // concurrent branch of the FAV batch (hash_to_G2)
  hipStream_t stream3 = nullptr;  // concurrent branch: sum r_i sigma_i (MSM) + its Miller loop
  hipEvent_t ev[EV_N] = {};
  bool bis_pending = false;  // a bisection has recorded ev[EV_BIS] that no batch has forked from yet
  uint8_t* h_partial = nullptr;     // pinned host copy of the partial
  Buf buf[NSLOT];
  // last prepared FAV batch
  size_t fav_B = 0;
  bool fav_ready = false;
  bool partial_pending = false;
  // the final-exponentiation check of the job's own product, enqueued by job_submit right behind it:
  // h_own[0] = its verdict once ev[EV_OWN] has passed; own_state -1 not read yet, 0 failed, 1 passed
  int* h_own = nullptr;
  bool own_pending = false;
  int own_state = -1;
  // multi-GPU (a communicator on the context): job_submit enqueues the all-gather of the partial on the context's
  // comm stream (ev[EV_COMM]: gathered) and the product's check on the job's stream; h_own[1] = that verdict once
  // ev[EV_CV] has passed.  The own check then runs only when the combined check fails (read_own).
  bool comm_pending = false;
  int fav_mg = 1;  // pairs per f of the prepared batch's Miller accumulation
  // the prepared batch shares messages (FavItems::msg_id): its pair arrays are per message, and the
  // bisection takes its per-item H through S_MSGID; seg / seg_ids: the host plan and ids its uploads read
  bool fav_shared = false;
  SegPlan seg;
  std::vector<uint32_t> seg_ids;
  // the prepared batch's items are (committees, bits) (FavItems::bits): the host tables its upload reads, in
  // pinned memory so that the copy never holds the submitting thread -- comm_offs | bit_offs | slot_offs (B + 1
  // u64 each), then the items' committee ids (u32) -- refilled only after the last upload has passed ev[EV_BITS];
  // bits_B / bits_items: the batch bls_last_gather_work reads back
  uint64_t* bits_tab = nullptr;
  size_t bits_tab_cap = 0, bits_tab_bytes = 0, bits_B = 0;
  bool bits_up_pending = false;
  const BitsItem* bits_items = nullptr;
  std::vector<uint64_t> bits_n;  // bits_plan's member counts
  // last bisection fallback: final-exponentiation checks and rounds (levels); the checks of a FAV bisection are
  // counted on the device (bis_dev_checks, read after the job's stream by bls_last_fallback_stats)
  uint64_t bis_checks = 0, bis_rounds = 0;
  uint32_t* bis_dev_checks = nullptr;
};

// Profile ids (bls_profile_*), in the order of PROF_NAMES (bls_capi_ctx.hip); PROF_CAP bounds the context's
// tables and what bls_profile_read copies out (batch.Profiler passes arrays of 16)
enum ProfId {
  P_FAV_GATHER, P_SIG_DECODE, P_FAV_HASH, P_G2_SUM, P_SIG_PAIR, P_MILLER, P_FP12_PROD, P_FINAL_EXP, P_FAV_FINISH,
  P_PARTIALS_PROD, P_SIG_VM, P_MSM, P_MILLER_LINES, P_KEY_VALIDATE, P_BITS_EXPAND, PROF_N
};
constexpr int PROF_CAP = 16;
static_assert(PROF_CAP >= PROF_N, "the profile tables hold every id");

struct bls_ctx {
  int device = 0;
  int njobs = 10;  // job slots with streams: BLS_FAV_JOBS_INIT (default 10, at most BLS_FAV_JOBS)
  Job jobs[BLS_FAV_JOBS];
  Job* j = &jobs[0];  // the job the current call works on
  std::mutex mu;
  std::string err;
  G1A* comb = nullptr;  // -G1 comb of the bisection fallback (bls_bisect.hip), built on first use
  Job* stats_job = &jobs[0];  // the job whose fallback statistics bls_last_fallback_stats reports
  uint64_t last_hashes = 0, last_pairs = 0;  // work of the last prepared FAV batch (bls_last_batch_work)
  // Context-wide streams for the kernels with large private segments (the h2c
  // fallback, 6,000 B/lane; final-exponentiation checks, 3,296 B/lane): the
  // runtime gives every hardware queue that runs such a kernel a scratch
  // reservation of (private segment x device wave slots), so they run on two
  // queues instead of on every job's (see k_h2c_fallback).
  hipStream_t fb_stream = nullptr, fe_stream = nullptr;
  // the per-call API's signature branch (verify_percall, AggregateVerify) beside the hash on stream2 and the keys
  // on stream1 when job 0 has two streams: one more stream, used by no batch
  hipStream_t pc_stream = nullptr;
  // the FAV jobs' all-gathers (multi-GPU): ONE stream, so the collectives run in the order the jobs were submitted
  // -- the same order on every rank -- whichever job's product is ready first
  hipStream_t comm_stream = nullptr;
  // registry (HBM resident): RegKey records of 96 B of affine (x, y) padded to 128 B and 128-B aligned (one
  // cache line per random read), validity in x's top bit; 128 MiB per 2^20 keys, 256 MiB for 2^21
  RegKey* reg = nullptr;
  size_t reg_n = 0;
  size_t reg_cap = 0;  // entries allocated (bls_registry_append grows it)
  uint64_t reg_gen = 0;  // bumped whenever the table is replaced (load / generate)
  // committee table (bls_committees_load, HBM resident): member lists ctab_idx[ctab_offs[c] .. ctab_offs[c + 1]),
  // csum[c] their keys' projective sum and cstat[c] = 1 iff every member was in range and valid at load; the
  // offsets' host copy sizes the items of a bits batch; ctab_gen: the registry generation the sums belong to
  uint32_t* ctab_idx = nullptr;
  uint64_t* ctab_offs = nullptr;
  G1P* ctab_sum = nullptr;
  int* ctab_stat = nullptr;
  std::vector<uint64_t> ctab_offs_h;
  bool ctab_loaded = false;
  uint64_t ctab_gen = 0;
  // G1 point table (bls_g1_table_load, HBM resident): 32 window-major RegKey records per entry -- record
  // w * g1t_cap + i is 2^(8w) T[i], REG_VALID on usable non-identity points -- and a state byte per entry (0 invalid,
  // 1 point, 2 identity; the host copy checks an MSM's indices); g1t_checked: every load and append so far asked
  // for the subgroup check; g1t_gen: bumped whenever the table is replaced; the MSM counters of bls_g1_table_stats
  RegKey* g1t = nullptr;
  uint8_t* g1t_stat = nullptr;
  std::vector<uint8_t> g1t_stat_h;
  size_t g1t_n = 0, g1t_cap = 0;
  bool g1t_checked = false;
  uint64_t g1t_gen = 0, g1t_msm_calls = 0, g1t_msm_entries = 0;
  uint64_t g1v_msm_calls = 0, g1v_msm_entries = 0;  // bls_g1_msm_stats: the bucket MSMs over a call's own points
  // blob KZG (bls_capi_kzg.hip): the domain table omega^brp(i), filled on first use; the setup's -[tau] G2 and, with
  // a Lagrange setup, the device list of its 4,096 table indices kzg_first + i and the G1 table generation it was
  // made on (a commitment call after the table was replaced is refused, the committee table's rule)
  Fr* kzg_dom = nullptr;
  G2A* kzg_negtau = nullptr;
  uint32_t* kzg_idx = nullptr;
  bool kzg_set = false;
  uint32_t kzg_first = 0, kzg_n = 0;
  uint64_t kzg_gen = 0;
  // cell KZG (bls_capi_kzg_cells.hip): the transform's tables w^i | 7^i | 7^-i, filled on first use
  Fr* kzc_tab = nullptr;
  // ... the cell setup's -[tau^64] G2, the device list of the 64 table indices of [tau^k] G1 and the G1 table
  // generation it was made on (a verification after the table was replaced is refused, as for kzg_gen)
  G2A* kzc_negtau64 = nullptr;
  uint32_t* kzc_idx = nullptr;
  bool kzc_set = false;
  uint64_t kzc_gen = 0;
  // ... the cell proof setup: the device list of the 4,096 table indices of [tau^i] G1 and the table generation
  uint32_t* kp_idx = nullptr;
  bool kp_set = false;
  uint64_t kp_gen = 0;
  Job* work_job = nullptr;  // the job whose bits batch bls_last_gather_work reports
  // test hook (bls_test_force_h2c_fallback): items whose hash_to_G2 is routed to k_h2c_fallback regardless of
  // the lane kernels' flags; null in every product use
  int* force_fb = nullptr;
  size_t force_fb_n = 0;
  SegPlan agg_plan;  // the host plan the last grouped aggregation's uploads read (bls_aggregate_grouped)
  uint8_t* pc_stage = nullptr;  // pinned staging of a per-call's inputs: one DMA instead of four pageable copies
  size_t pc_stage_cap = 0;
  // multi-GPU exchange of FAV partials (bls_comm_*): one RCCL communicator
  ncclComm_t comm = nullptr;
  int comm_rank = 0, comm_world = 1;
  std::string comm_abort_cause;  // why the library aborted the communicator (reported by later calls)
  // per-kernel hipEvent timing of the FAV path (bls_profile_*)
  bool prof_on = false;
  std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> prof_pending;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_pool;
  double prof_ms[PROF_CAP] = {0};
  uint64_t prof_cnt[PROF_CAP] = {0};
};

namespace capi {

// Every environment knob of the C ABI pieces but three: BLS_GATHER is read per batch (gather_stage), and
// BLS_FAV_JOBS_INIT / BLS_JOB_STREAMS / BLS_FE_STREAM shape the context at bls_ctx_create.  Names, defaults and the
// evidence for each are in one table, knobs() in bls_capi_ctx.hip, read once on first use.
struct Knobs {
  size_t wide_h2c_max, wide_miller_max, acc_shared_min, acc8_max, fe_wide_max;
  int acc_g;
  bool miller_fused, acc_ll, bisect_fe_wide;
};
const Knobs& knobs();

int fail(bls_ctx* c, hipError_t e, const char* where);
int h2d(bls_ctx* ctx, void* d, const void* h, size_t n);  // async, on the job's stream
int d2h(bls_ctx* ctx, void* h, const void* d, size_t n);  // ... and synchronises it
int all_ok(bls_ctx* ctx, const int* d_ok, size_t n);  // the n verdict words back: 1, 0 if any is 0, or BLS_E_*
int sync_jobs(bls_ctx* ctx);
int run_final_check(bls_ctx* ctx, const Fp12* f, int n, bool wide);
int run_final_checks_sel(bls_ctx* ctx, const Fp12* f, const uint32_t* sel, size_t nsel, uint32_t* d_sel, int* d_res,
                         int* res);
int h2c_fallback(bls_ctx* ctx, hipStream_t st, size_t B, const uint8_t* msgs, const uint64_t* offs, int* flag, G2A* H);
int validate_pks(bls_ctx* ctx, const uint8_t* pks, size_t n, G1A** outA, int** outOk);
hipError_t launch_keys(hipStream_t st, const uint8_t* pks, size_t n, G1A* out, int* ok);
hipError_t launch_key_table(hipStream_t st, const uint8_t* pks, size_t n, RegKey* rec, uint8_t* valid);
hipError_t launch_pairs_decode(hipStream_t st, const uint8_t* d_in, size_t n, bool subgroup, G1A* P, G2A* Q, int* ok1,
                               int* ok2);
hipError_t launch_miller_call(hipStream_t st, const G1A* P, const G2A* Q, size_t n, Fp12* f, size_t* nf,
                              const Fp2* qz);
int stage_pairs(bls_ctx* ctx, const uint8_t* g1s48, const uint8_t* g2s96, size_t n, bool subgroup, G1A** P, G2A** Q);
// The bucket MSM over device-resident points (bls_capi_msm.hip; launch_g1_var_msm on the job's stream with the
// S_GV_* scratch): aff / live[v] = sum_i [k32[v n + i]] pts[i] for v < B, in the caller's arrays; out48 (nullable,
// device): the compressed bytes; *d_entries (nullable): where the device leaves the bucket entries.  No host round
// trip; counted by bls_g1_msm_stats as one call (the entries only where the caller reads them back).
int g1_var_msm_dev(bls_ctx* ctx, const G1A* pts, const int* ok, size_t n, size_t B, const uint8_t* k32, G1A* aff,
                   int* live, uint8_t* out48, const uint32_t** d_entries);
int ensure_comb(bls_ctx* ctx, hipStream_t st);  // ctx->comb, the -G1 comb (bls_bisect.hip), built on first use
int host_seed(bls_ctx* ctx, uint8_t seed[32]);
int nccl_fail(bls_ctx* c, ncclResult_t r, const char* where);
void comm_fail_abort(bls_ctx* ctx);
int enqueue_comm_check(bls_ctx* ctx);

}  // namespace capi
using namespace capi;

#define HIPCK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(ctx, e_, #x); } while (0)
#define CK(x) do { int r_ = (x); if (r_) return r_; } while (0)

// Device scratch pointer for slot s with at least `bytes` bytes.
template <class T>
int scratch(bls_ctx* ctx, int s, size_t count, T** out) {
  size_t bytes = count * sizeof(T);
  if (bytes == 0) bytes = 16;
  Buf& b = ctx->j->buf[s];
  if (b.cap < bytes) {
    if (b.p) {
      HIPCK(hipStreamSynchronize(ctx->j->stream));
      HIPCK(hipFree(b.p));
      b.p = nullptr;
      b.cap = 0;
    }
    size_t cap = bytes + bytes / 4;
    HIPCK(hipMalloc(&b.p, cap));
    b.cap = cap;
  }
  *out = (T*)b.p;
  return 0;
}
#define SCR(slot, n, ptr) CK(scratch(ctx, slot, (n), &(ptr)))

// Event pair around one launch when profiling is on.
struct ProfScope {
  bls_ctx* c;
  int id;
  hipStream_t st;
  std::pair<hipEvent_t, hipEvent_t> ev{nullptr, nullptr};
  ProfScope(bls_ctx* c_, ProfId id_, hipStream_t st_) : c(c_), id(id_), st(st_ ? st_ : c_->j->stream) {
    if (!c->prof_on) return;
    if (c->prof_pool.empty()) {
      hipEvent_t a, b;
      if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
      c->prof_pool.push_back({a, b});
    }
    ev = c->prof_pool.back();
    c->prof_pool.pop_back();
    (void)hipEventRecord(ev.first, st);
  }
  ~ProfScope() {
    if (!ev.first) return;
    (void)hipEventRecord(ev.second, st);
    c->prof_pending.push_back({id, ev});
  }
};
#define PROF2(id, st, expr) do { ProfScope ps_(ctx, id, st); HIPCK(expr); } while (0)
#define PROF(id, expr) PROF2(id, nullptr, expr)  // on the job's stream

#define API_ENTER(ctx)                         \
  if (!ctx) return BLS_E_ARG;                  \
  std::lock_guard<std::mutex> lock_(ctx->mu);  \
  if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, hipGetLastError(), "hipSetDevice")

// Points the call at job k (after API_ENTER); job 0 again on return.
struct JobScope {
  bls_ctx* c;
  JobScope(bls_ctx* c_, int k) : c(c_) { c->j = &c->jobs[k]; }
  ~JobScope() { c->j = &c->jobs[0]; }
};
#define JOB_ENTER(ctx, job)                                  \
  API_ENTER(ctx);                                            \
  if ((job) < 0 || (job) >= ctx->njobs) return BLS_E_ARG;     \
  JobScope job_scope_(ctx, job)
