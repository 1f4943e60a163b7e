// C ABI of libblsmi355x.so (declared in include/blsmi355x.h).  Host code:
// argument checks, H2D/D2H copies into a per-context scratch arena, kernel
// launches on the context's stream.  No compute happens on the host.
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

namespace {

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
  S_OWN,  // the job's own final check (job_submit)
  S_GAFF, S_GREDO,  // the affine gather's level lists and redo flags (bls_gather_aff.hip)
  S_COMM, S_CV,  // the all-gathered partials of all ranks and their check's verdict (enqueue_comm_check)
  // shared-message batches (fav_prepare with a grouping): the pair arrays' status and G1 side (M + MSM_UPAIRS; the
  // G2 side is S_H), the group sums before the affine conversion, the fold's two partial arrays, its runs and sorted
  // item list, the items' message ids, and the bisection's per-item H
  S_PSTAT, S_GP, S_GSUM, S_SEGA, S_SEGB, S_SEGRUN, S_SEGIT, S_MSGID, S_BHIT,
  // grouped signature aggregation (bls_aggregate_grouped; own slots: a FAV batch may be between its partial and
  // finish calls): staged signatures, mask and outputs of the host-buffer call, the decoded members and their ok,
  // the fold's runs, sorted item list, two partial arrays and the group sums
  S_AGG_IN, S_AGG_INC, S_AGG_OUT, S_AGG_A, S_AGG_OK, S_AGG_RUN, S_AGG_IT, S_AGG_PA, S_AGG_PB, S_AGG_SUM,
  // committee-bitfield batches (fav_prepare with bits): the job's host tables in one piece (the three offset tables
  // -- committees | bit bytes | list slots, B + 1 each -- then the items' committee ids), the expanded index lists
  // and the item records
  S_BTAB, S_BLIST, S_BITEM,
  NSLOT
};

struct Buf {
  void* p = nullptr;
  size_t cap = 0;
};

}  // namespace

// Per-batch device state, streams and events.  A context owns
// BLS_FAV_JOBS of them so that consecutive FAV batches can be in flight
// together (bls_fav_job_*): batch k+1's front kernels fill the GPU while
// batch k's Miller product is final-exponentiated.  The per-call API and the
// registry use job 0.
struct Job {
  hipStream_t stream = nullptr;
  hipStream_t stream2 = nullptr;  // concurrent branch of the FAV batch (hash_to_G2)
  hipStream_t stream3 = nullptr;  // concurrent branch: sum r_i sigma_i (MSM) + its Miller loop
  hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_sig = nullptr, ev_msm = nullptr, ev_gather = nullptr;
  hipEvent_t ev_partial = nullptr;  // the batch's 576-byte partial is in h_partial
  hipEvent_t ev_h2c = nullptr, ev_fb = nullptr, ev_fe = nullptr;  // hand-offs to the context-wide aux streams
  // a bisection has copied what it reads of the batch state that stream2 / stream3 overwrite: the job's next batch
  // starts its hash and signature branches from here instead of after the whole bisection (fav_prepare)
  hipEvent_t ev_bis = nullptr;
  bool bis_pending = false;
  uint8_t* h_partial = nullptr;     // pinned host copy of the partial
  Buf buf[NSLOT];
  // last prepared FAV batch
  size_t fav_B = 0;
  bool fav_ready = false;
  bool partial_pending = false;
  // the final-exponentiation check of the job's own product, enqueued by job_submit right behind it:
  // h_own[0] = its verdict once ev_own has passed; own_state -1 not read yet, 0 failed, 1 passed
  int* h_own = nullptr;
  hipEvent_t ev_own = nullptr;
  bool own_pending = false;
  int own_state = -1;
  // multi-GPU (a communicator on the context): job_submit enqueues the all-gather of the partial on the context's
  // comm stream (ev_comm: gathered) and the product's check on the job's stream; h_own[1] = that verdict once
  // ev_cv has passed.  The own check then runs only when the combined check fails (read_own).
  bool comm_pending = false;
  hipEvent_t ev_comm = nullptr, ev_cv = nullptr;
  int fav_mg = 1;  // pairs per f of the prepared batch's Miller accumulation
  // the prepared batch shares messages (fav_prepare with a grouping): its pair arrays are per message, and the
  // bisection takes its per-item H through S_MSGID; seg / seg_ids: the host plan and ids its uploads read
  bool fav_shared = false;
  SegPlan seg;
  std::vector<uint32_t> seg_ids;
  // the prepared batch's items are (committees, bits) (fav_prepare with bits): the host tables its upload reads, in
  // pinned memory so that the copy never holds the submitting thread -- comm_offs | bit_offs | slot_offs (B + 1
  // u64 each), then the items' committee ids (u32) -- refilled only after the last upload has passed ev_bits;
  // bits_B / bits_items: the batch bls_last_gather_work reads back
  uint64_t* bits_tab = nullptr;
  size_t bits_tab_cap = 0, bits_tab_bytes = 0, bits_B = 0;
  hipEvent_t ev_bits = nullptr;
  bool bits_up_pending = false;
  const BitsItem* bits_items = nullptr;
  std::vector<uint64_t> bits_n;  // bits_plan's member counts
  // last bisection fallback: final-exponentiation checks and rounds (levels); the checks of a FAV bisection are
  // counted on the device (bis_dev_checks, read after the job's stream by bls_last_fallback_stats)
  uint64_t bis_checks = 0, bis_rounds = 0;
  uint32_t* bis_dev_checks = nullptr;
};

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
  double prof_ms[16] = {0};
  uint64_t prof_cnt[16] = {0};
};

static const char* const PROF_NAMES[] = {"fav_gather", "sig_decode", "fav_hash", "g2_sum",        "sig_pair", "miller",
                                         "fp12_prod",  "final_exp",  "fav_finish", "partials_prod", "sig_vm",
                                         "msm",        "miller_lines", "key_validate", "bits_expand"};
static const int PROF_N = sizeof(PROF_NAMES) / sizeof(PROF_NAMES[0]);

namespace {

int fail(bls_ctx* c, hipError_t e, const char* where) {
  char b[256];
  snprintf(b, sizeof b, "%s: %s", where, hipGetErrorString(e));
  c->err = b;
  return BLS_E_DEVICE;
}

#define HIPCK(x)                                     \
  do {                                               \
    hipError_t e_ = (x);                             \
    if (e_ != hipSuccess) return fail(ctx, e_, #x); \
  } while (0)

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

#define SCR(slot, n, ptr)                       \
  do {                                          \
    int r_ = scratch(ctx, slot, (n), &(ptr));   \
    if (r_) return r_;                          \
  } while (0)

int h2d(bls_ctx* ctx, void* d, const void* h, size_t n) {
  if (n) HIPCK(hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, ctx->j->stream));
  return 0;
}
int d2h(bls_ctx* ctx, void* h, const void* d, size_t n) {
  if (n) HIPCK(hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, ctx->j->stream));
  HIPCK(hipStreamSynchronize(ctx->j->stream));
  return 0;
}

#define CK(x)            \
  do {                   \
    int r_ = (x);        \
    if (r_) return r_;   \
  } while (0)
#define LK(x)                                                   \
  do {                                                          \
    hipError_t e_ = (x);                                        \
    if (e_ != hipSuccess) return fail(ctx, e_, #x);             \
  } while (0)

// AggregateVerify: one wide workgroup per message up to this many (tools/av_probe.py: 1,024 messages 7.95 -> 6.85
// ms; 8,192 took 15.1 -> 31.5 ms, past the chip's CUs); knob BLS_WIDE_H2C_MAX
static const size_t WIDE_H2C_MAX = getenv("BLS_WIDE_H2C_MAX") ? (size_t)atol(getenv("BLS_WIDE_H2C_MAX")) : 1024;
// the Miller values of the per-call pairing APIs (AggregateVerify, pairing checks, multi-pairings): the wide kernel
// on ceil(n / 2) workgroups up to this many pairs, the wave-program kernel beyond (AggregateVerify(512) 5.54 -> 4.17
// ms, (1,024) 7.95 -> 7.31; at 8,192 pairs the wave programs' throughput wins); *nf = the number of f values written;
// knob BLS_WIDE_MILLER_MAX
static const size_t WIDE_MILLER_MAX = getenv("BLS_WIDE_MILLER_MAX") ? (size_t)atol(getenv("BLS_WIDE_MILLER_MAX")) : 1100;
// qz: Jacobian Z of every Q, which only the wide kernel takes: a call with qz beyond WIDE_MILLER_MAX is refused
// (the wave-program kernel would read Jacobian X, Y as affine coordinates)
static hipError_t launch_miller_call(hipStream_t st, const G1A* P, const G2A* Q, size_t n, Fp12* f, size_t* nf,
                                     const Fp2* qz = nullptr) {
  if (n <= WIDE_MILLER_MAX) {
    *nf = miller_wide_nf(n);
    return launch_miller_wide_n(st, P, Q, nullptr, n, f, qz);
  }
  if (qz) return hipErrorInvalidValue;
  *nf = n;
  return launch_miller_wave(st, P, Q, nullptr, n, f);
}
constexpr size_t WIDE_KEYS_MAX = 4096;  // KeyValidate of a call's keys: two keys per wave up to this many

// a call's keys (per-call FastAggregateVerify, AggregateVerify, AggregatePKs): the wide kernel's latency for a few
// thousand keys, the lane kernel's throughput beyond (registry loads always take the lane kernel)
static hipError_t launch_keys(hipStream_t st, const uint8_t* pks, size_t n, G1A* out, int* ok) {
  return n <= WIDE_KEYS_MAX ? launch_key_validate_wide(st, pks, n, out, ok) : launch_key_validate(st, pks, n, out, ok);
}

// the pairing APIs' decodes of n (G1, G2) pairs at d_in (48 n bytes of G1, then 96 n of G2), identity accepted: with
// the subgroup checks on the wide kernels (latency; up to WIDE_KEYS_MAX pairs), unchecked or beyond on the lane kernels
static hipError_t launch_pairs_decode(hipStream_t st, const uint8_t* d_in, size_t n, bool subgroup, G1A* P, G2A* Q,
                                      int* ok1, int* ok2) {
  hipError_t e;
  if (subgroup && n <= WIDE_KEYS_MAX) {
    e = launch_g1_decode_checked_wide(st, d_in, n, P, ok1);
    return e != hipSuccess ? e : launch_sig_validate_wide(st, d_in + 48 * n, n, Q, ok2);
  }
  e = launch_pt_decode(st, 1, d_in, n, subgroup ? 1 : 0, P, ok1);
  return e != hipSuccess ? e : launch_pt_decode(st, 2, d_in + 48 * n, n, subgroup ? 1 : 0, Q, ok2);
}

// Copy n compressed keys, validate them on the device; returns 1 if all valid.
int validate_pks(bls_ctx* ctx, const uint8_t* pks, size_t n, G1A** outA, int** outOk) {
  uint8_t* d_in;
  G1A* d_a;
  int* d_ok;
  SCR(S_IN0, 48 * n, d_in);
  SCR(S_G1A, n + 1, d_a);
  SCR(S_OK, n + 1, d_ok);
  CK(h2d(ctx, d_in, pks, 48 * n));
  LK(launch_keys(ctx->j->stream, d_in, n, d_a, d_ok));
  std::vector<int> ok(n);
  CK(d2h(ctx, ok.data(), d_ok, n * sizeof(int)));
  *outA = d_a;
  *outOk = d_ok;
  for (size_t i = 0; i < n; i++)
    if (!ok[i]) return 0;
  return 1;
}

// Event pair around one launch when profiling is on.
struct ProfScope {
  bls_ctx* c;
  int id;
  hipStream_t st;
  std::pair<hipEvent_t, hipEvent_t> ev{nullptr, nullptr};
  ProfScope(bls_ctx* c_, int id_, hipStream_t st_ = nullptr) : c(c_), id(id_), st(st_ ? st_ : c_->j->stream) {
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

void prof_collect(bls_ctx* c) {
  for (auto& p : c->prof_pending) {
    float ms = 0;
    if (hipEventSynchronize(p.second.second) == hipSuccess &&
        hipEventElapsedTime(&ms, p.second.first, p.second.second) == hipSuccess) {
      c->prof_ms[p.first] += ms;
      c->prof_cnt[p.first] += 1;
    }
    c->prof_pool.push_back(p.second);
  }
  c->prof_pending.clear();
}

#define PROF(id, expr)          \
  do {                          \
    ProfScope ps_(ctx, id);     \
    LK(expr);                   \
  } while (0)
#define PROF2(id, st, expr)     \
  do {                          \
    ProfScope ps_(ctx, id, st); \
    LK(expr);                   \
  } while (0)

// Final-exponentiation check of the product of f[0 .. n) on the context's FE
// stream, after the current job's stream: 1 / 0.
int run_final_check(bls_ctx* ctx, const Fp12* f, int n = 1, bool wide = false) {
  int* d_r;
  SCR(S_INT, 4, d_r);
  Job& J = *ctx->j;
  // the context's FE stream, or the job's own (BLS_FE_STREAM=job: one hardware queue fewer)
  hipStream_t fe = ctx->fe_stream ? ctx->fe_stream : J.stream;
  if (fe != J.stream) {
    HIPCK(hipEventRecord(J.ev_fe, J.stream));
    HIPCK(hipStreamWaitEvent(fe, J.ev_fe, 0));
  }
  // batch checks on the one-wave k_fe_check, which leaves the CU to the other jobs (profiles/r04m_fe_ab.txt: 1.92 M vs
  // 1.84 M FAV/s with every check six-wave); single calls (wide: the pairing checks) on the six-wave k_fe_wide
  if (wide)
    PROF2(7, fe, launch_fe_wide(fe, f, n, d_r));
  else
    PROF2(7, fe, launch_final_check_wave(fe, f, n, d_r));
  int r = 0;
  HIPCK(hipMemcpyAsync(&r, d_r, sizeof r, hipMemcpyDeviceToHost, fe));
  HIPCK(hipStreamSynchronize(fe));
  return r ? 1 : 0;
}

// nsel independent checks res[k] = (FE(f[sel[k]]) == 1) on the FE stream, after
// the job's stream (bisection rounds, AggregateVerify per-item checks).
int run_final_checks_sel(bls_ctx* ctx, const Fp12* f, const uint32_t* sel, size_t nsel, uint32_t* d_sel, int* d_res,
                         int* res) {
  if (!nsel) return 0;
  Job& J = *ctx->j;
  hipStream_t fe = ctx->fe_stream ? ctx->fe_stream : J.stream;
  if (fe != J.stream) {
    HIPCK(hipEventRecord(J.ev_fe, J.stream));
    HIPCK(hipStreamWaitEvent(fe, J.ev_fe, 0));
  }
  HIPCK(hipMemcpyAsync(d_sel, sel, 4 * nsel, hipMemcpyHostToDevice, fe));
  PROF2(8, fe, launch_final_check_sel(fe, f, d_sel, nsel, d_res));
  HIPCK(hipMemcpyAsync(res, d_res, 4 * nsel, hipMemcpyDeviceToHost, fe));
  HIPCK(hipStreamSynchronize(fe));
  return 0;
}

// hash_to_G2 exceptional items (k_h2c_fallback) on the context's fallback
// stream, between the h2c phases on `st` and whatever `st` runs next.
__global__ void k_or_flags(size_t B, const int* force, int* flag) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < B && force[i]) flag[i] = 1;
}

int h2c_fallback(bls_ctx* ctx, hipStream_t st, size_t B, const uint8_t* msgs, const uint64_t* offs, int* flag,
                 G2A* H) {
  Job& J = *ctx->j;
  if (ctx->force_fb && B) {  // test hook only: the mask's items i < min(B, n)
    const size_t nf = B < ctx->force_fb_n ? B : ctx->force_fb_n;
    hipLaunchKernelGGL(k_or_flags, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, st, nf, ctx->force_fb, flag);
    LK(hipGetLastError());
  }
  HIPCK(hipEventRecord(J.ev_h2c, st));
  HIPCK(hipStreamWaitEvent(ctx->fb_stream, J.ev_h2c, 0));
  LK(launch_h2c_fallback(ctx->fb_stream, B, msgs, offs, flag, H));
  HIPCK(hipEventRecord(J.ev_fb, ctx->fb_stream));
  HIPCK(hipStreamWaitEvent(st, J.ev_fb, 0));
  return 0;
}

__global__ void k_copy_int(const int* src, int* dst) {
  if (threadIdx.x == 0) *dst = *src;
}

__global__ void k_set_neg_g1(G1A* p) {
  if (threadIdx.x || blockIdx.x) return;
  G1A g = g1_generator();
  g.y = fp_neg(g.y);
  *p = g;
}

__global__ void k_set_fp2_one(Fp2* z) {
  if (threadIdx.x || blockIdx.x) return;
  *z = fp2_one();
}

}  // namespace

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

// Hardware queues: the FAV pipeline keeps up to BLS_FAV_JOBS_INIT x 3 streams
// busy; with HIP's default of 4 hardware queues a long lane kernel blocks the
// streams sharing its queue.  The library does NOT change the process
// environment: the host sets GPU_MAX_HW_QUEUES before HIP starts
// (the Python shim does so only when it is unset).

extern "C" {

// streams: 3, or 2 with stream3 an alias of stream2 (fav_prepare's two-stream order)
static bool job_init(Job& J, int prio_hi, int streams) {
  if (streams < 3) {
    if (hipStreamCreateWithFlags(&J.stream2, hipStreamNonBlocking) != hipSuccess) return false;
    J.stream3 = J.stream2;
  } else if (hipStreamCreateWithFlags(&J.stream2, hipStreamNonBlocking) != hipSuccess ||
             hipStreamCreateWithPriority(&J.stream3, hipStreamNonBlocking, prio_hi) != hipSuccess) {
    return false;
  }
  return hipStreamCreateWithFlags(&J.stream, hipStreamNonBlocking) == hipSuccess &&
         hipEventCreateWithFlags(&J.ev_fork, hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&J.ev_join, hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&J.ev_sig, hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&J.ev_msm, hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&J.ev_gather, hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&J.ev_partial, hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&J.ev_h2c, hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&J.ev_fb, hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&J.ev_fe, hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&J.ev_bis, hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&J.ev_own, hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&J.ev_comm, hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&J.ev_cv, hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&J.ev_bits, hipEventDisableTiming) == hipSuccess &&
         hipHostMalloc((void**)&J.h_own, 2 * sizeof(int), hipHostMallocDefault) == hipSuccess &&
         hipHostMalloc((void**)&J.h_partial, 576, hipHostMallocDefault) == hipSuccess;
}

static void job_destroy(Job& J) {
  hipStream_t ss[3] = {J.stream, J.stream2, J.stream3 == J.stream2 ? nullptr : J.stream3};
  for (hipStream_t s : ss)
    if (s) (void)hipStreamSynchronize(s);
  for (auto& b : J.buf)
    if (b.p) (void)hipFree(b.p);
  hipEvent_t es[14] = {J.ev_fork, J.ev_join, J.ev_sig, J.ev_msm, J.ev_gather, J.ev_partial, J.ev_h2c,
                       J.ev_fb,   J.ev_fe,   J.ev_bis, J.ev_own, J.ev_comm,   J.ev_cv,      J.ev_bits};
  for (hipEvent_t e : es)
    if (e) (void)hipEventDestroy(e);
  if (J.h_partial) (void)hipHostFree(J.h_partial);
  if (J.bits_tab) (void)hipHostFree(J.bits_tab);
  if (J.h_own) (void)hipHostFree(J.h_own);
  for (hipStream_t s : ss)
    if (s) (void)hipStreamDestroy(s);
}

int bls_ctx_create(int device, bls_ctx** out) {
  if (!out) return BLS_E_ARG;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device || device < 0) return BLS_E_DEVICE;
  if (hipSetDevice(device) != hipSuccess) return BLS_E_DEVICE;
  bls_ctx* c = new (std::nothrow) bls_ctx();
  if (!c) return BLS_E_DEVICE;
  c->device = device;
  int prio_lo = 0, prio_hi = 0;  // the MSM branch is latency-bound: schedule it first
  (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
  // All job streams are created here, before any kernel runs (streams created
  // later, between launches, were measured to hit HSA_STATUS_ERROR_OUT_OF_RESOURCES).
  if (const char* v = getenv("BLS_FAV_JOBS_INIT")) c->njobs = atoi(v) < 1 ? 1 : atoi(v) > BLS_FAV_JOBS ? BLS_FAV_JOBS : atoi(v);
  // streams per job (BLS_JOB_STREAMS, default 2, or 3): with two, 10 jobs fit the hardware queues that held 7
  // (profiles/r05h_jobs_streams_ab.txt: C2 +3 %, C3 +13 %)
  int streams = 2;
  if (const char* v = getenv("BLS_JOB_STREAMS")) streams = atoi(v) == 3 ? 3 : 2;
  for (int k = 0; k < c->njobs; ++k) {
    if (!job_init(c->jobs[k], prio_hi, streams)) {
      bls_ctx_destroy(c);
      return BLS_E_DEVICE;
    }
  }
  // batch checks on each job's own stream (default) or on one context-wide FE stream (BLS_FE_STREAM=ctx): on one
  // stream the checks of different jobs queue behind each other
  const char* fev = getenv("BLS_FE_STREAM");
  const bool fe_job = !(fev && !strcmp(fev, "ctx"));
  if (hipStreamCreateWithFlags(&c->fb_stream, hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithFlags(&c->pc_stream, hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithFlags(&c->comm_stream, hipStreamNonBlocking) != hipSuccess ||
      (!fe_job && hipStreamCreateWithPriority(&c->fe_stream, hipStreamNonBlocking, prio_hi) != hipSuccess)) {
    bls_ctx_destroy(c);
    return BLS_E_DEVICE;
  }
  *out = c;
  return 0;
}

void bls_ctx_destroy(bls_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  if (ctx->comm) (void)ncclCommDestroy(ctx->comm);
  for (Job& J : ctx->jobs) job_destroy(J);
  for (hipStream_t s : {ctx->fb_stream, ctx->fe_stream, ctx->pc_stream, ctx->comm_stream})
    if (s) {
      (void)hipStreamSynchronize(s);
      (void)hipStreamDestroy(s);
    }
  for (auto& p : ctx->prof_pending) ctx->prof_pool.push_back(p.second);
  for (auto& p : ctx->prof_pool) {
    (void)hipEventDestroy(p.first);
    (void)hipEventDestroy(p.second);
  }
  if (ctx->reg) (void)hipFree(ctx->reg);
  for (void* p : {(void*)ctx->ctab_idx, (void*)ctx->ctab_offs, (void*)ctx->ctab_sum, (void*)ctx->ctab_stat})
    if (p) (void)hipFree(p);
  if (ctx->comb) (void)hipFree(ctx->comb);
  if (ctx->force_fb) (void)hipFree(ctx->force_fb);
  if (ctx->pc_stage) (void)hipHostFree(ctx->pc_stage);
  delete ctx;
}

const char* bls_last_error(bls_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int bls_device_info(bls_ctx* ctx, char* name, size_t name_len, int* cu_count) {
  API_ENTER(ctx);
  hipDeviceProp_t p;
  HIPCK(hipGetDeviceProperties(&p, ctx->device));
  if (name && name_len) {
    snprintf(name, name_len, "%s (%s)", p.name, p.gcnArchName);
  }
  if (cu_count) *cu_count = p.multiProcessorCount;
  return 0;
}

// Per-call CoreVerify over n keys (n = 1: Verify, E/utils/bls.py:141-151;
// n > 1: FastAggregateVerify, :167-177), on three streams, in wavefront-cooperative arithmetic:
//   stream2: hash_to_G2(msg) on one wave (k_h2c_wide)
//   stream3 (job 0's third stream, or the context's per-call stream when job 0 has two): signature decode + G2
//            subgroup check (k_sig_validate_wide)
//            then the Miller loop of (-G1, sigma) on one k_miller_wide workgroup (it overlaps the hash's tail)
//   stream1: KeyValidate of every key (+ their sum), then -- after the hash --
//            the Miller loop of (apk, H) on another, the six-wave final
//            exponentiation (k_fe_wide) of both loops' product on the same
//            stream, and both verdict words (FE, live) back in one pinned copy.
static int verify_percall(bls_ctx* ctx, const uint8_t* pks48, size_t n, const uint8_t* msg, size_t msg_len,
                          const uint8_t* sig96) {
  Job& J = *ctx->j;
  hipStream_t st = J.stream, st2 = J.stream2, st3 = J.stream3;
  uint8_t* d_in;
  G1A *keys, *P;
  G2A* Q;
  int *ok, *d_r;
  G1J *tmp, *apk;
  int* flag;
  Fp12* f;
  uint64_t* d_offs;
  const size_t in_bytes = 48 * n + 96 + msg_len;
  const size_t offs_at = (in_bytes + 7) & ~(size_t)7;  // the two message offsets after the inputs, 8-B aligned
  const size_t total = offs_at + 16;
  SCR(S_IN0, total, d_in);
  d_offs = reinterpret_cast<uint64_t*>(d_in + offs_at);
  SCR(S_G1A, n, keys);
  SCR(S_OK, n + 2, ok);  // key verdicts | sig verdict | live
  SCR(S_PC_P, 3, P);  // P[0] apk, P[1] -G1 (k_percall_pairs), P[2] -G1 (the signature's pair, its own stream)
  SCR(S_G2A, 2, Q);
  Fp2* hz = nullptr;  // H's Jacobian Z (k_h2c_wide skips its inversion; the Miller loop's additions take Q as is)
  if (!ctx->force_fb) SCR(S_G2A_B, 1, hz);  // (the forced-fallback test hook overwrites H affine after the kernel)
  Fp* pz = nullptr;  // the key sum's Jacobian Z (no inversion; the Miller loop scales its lines by Z^3)
  if (n > 1) SCR(S_PC_PZ, 1, pz);
  SCR(S_G1J_T, 1024, tmp);
  SCR(S_G1J, 1, apk);
  SCR(S_AV_FLAG, 1, flag);
  SCR(S_F, 2, f);  // f(apk, H) | f(-G1, sigma)
  SCR(S_INT, 4, d_r);
  uint8_t* d_pk = d_in;
  uint8_t* d_sig = d_in + 48 * n;
  uint8_t* d_msg = d_in + 48 * n + 96;
  const uint64_t offs[2] = {0, msg_len};
  if (ctx->pc_stage_cap < total) {  // grows to the largest call seen; the previous call has synchronised
    if (ctx->pc_stage) HIPCK(hipHostFree(ctx->pc_stage));
    ctx->pc_stage = nullptr;
    ctx->pc_stage_cap = 0;
    HIPCK(hipHostMalloc((void**)&ctx->pc_stage, total, hipHostMallocDefault));
    ctx->pc_stage_cap = total;
  }
  memcpy(ctx->pc_stage, pks48, 48 * n);
  memcpy(ctx->pc_stage + 48 * n, sig96, 96);
  if (msg_len) memcpy(ctx->pc_stage + 48 * n + 96, msg, msg_len);
  memcpy(ctx->pc_stage + offs_at, offs, sizeof offs);
  CK(h2d(ctx, d_in, ctx->pc_stage, total));
  // a two-stream job 0 (stream3 aliases stream2): the signature check on the context's per-call stream, beside
  // the hash and the keys (on stream1 ahead of the keys it made stream1 as long as the hash: 0.8 + 0.7 ms)
  const hipStream_t ss = st3 != st2 ? st3 : ctx->pc_stream;
  HIPCK(hipEventRecord(J.ev_fork, st));
  HIPCK(hipStreamWaitEvent(st2, J.ev_fork, 0));
  if (ss != st) HIPCK(hipStreamWaitEvent(ss, J.ev_fork, 0));
  // one wave of wavefront-cooperative arithmetic for the one message (bls_wide.h); 32-byte messages (every
  // signing root) take the register-resident expand_message_xmd
  const uint64_t* h_offs = msg_len == 32 ? nullptr : d_offs;
  LK(launch_h2c_wide(st2, 1, d_msg, h_offs, Q, flag, hz));
  CK(h2c_fallback(ctx, st2, 1, d_msg, h_offs, flag, Q));
  HIPCK(hipEventRecord(J.ev_join, st2));
  LK(launch_sig_validate_wide(ss, d_sig, 1, Q + 1, ok + n));
  HIPCK(hipEventRecord(J.ev_sig, ss));
  // (-G1, sigma)'s Miller loop right behind the signature check, beside the hash (constant lines for a rejected
  // signature): one pair per workgroup, so the critical path after the hash is one pair's loop, not two
  hipLaunchKernelGGL(k_set_neg_g1, dim3(1), dim3(64), 0, ss, P + 2);
  LK(hipGetLastError());
  LK(launch_miller_wide(ss, P + 2, Q + 1, ok + n, nullptr, 1, f + 1));
  HIPCK(hipEventRecord(J.ev_msm, ss));
  LK(launch_keys(st, d_pk, n, keys, ok));
  if (n > 1) LK(launch_g1_sum_aff(st, keys, nullptr, n, tmp, apk));
  HIPCK(hipStreamWaitEvent(st, J.ev_sig, 0));
  LK(launch_percall_pairs(st, keys, ok, n, apk, ok + n, P, ok + n + 1, pz));
  HIPCK(hipStreamWaitEvent(st, J.ev_join, 0));
  // (apk, H): rejected inputs are identities there, `live` decides
  LK(launch_miller_wide(st, P, Q, nullptr, nullptr, 1, f, hz, pz));
  HIPCK(hipStreamWaitEvent(st, J.ev_msm, 0));
  // the six-wave final check of f(apk, H) f(-G1, sigma) on the same stream, then both verdict words in one copy
  // (FE | live) and one sync
  PROF2(7, st, launch_fe_wide(st, f, 2, d_r));
  hipLaunchKernelGGL(k_copy_int, dim3(1), dim3(64), 0, st, ok + n + 1, d_r + 1);
  LK(hipGetLastError());
  int res[2] = {0, 0};
  HIPCK(hipMemcpyAsync(ctx->pc_stage, d_r, sizeof res, hipMemcpyDeviceToHost, st));
  HIPCK(hipStreamSynchronize(st));
  memcpy(res, ctx->pc_stage, sizeof res);
  return (res[0] && res[1]) ? 1 : 0;
}

int bls_verify(bls_ctx* ctx, const uint8_t* pk48, const uint8_t* msg, size_t msg_len, const uint8_t* sig96) {
  API_ENTER(ctx);
  if (!pk48 || !sig96 || (!msg && msg_len) || msg_len > 0xffffffffu) return BLS_E_ARG;
  return verify_percall(ctx, pk48, 1, msg, msg_len, sig96);
}

int bls_fast_aggregate_verify(bls_ctx* ctx, const uint8_t* pks48, size_t n, const uint8_t* msg, size_t msg_len,
                              const uint8_t* sig96) {
  API_ENTER(ctx);
  if ((!pks48 && n) || !sig96 || (!msg && msg_len) || msg_len > 0xffffffffu) return BLS_E_ARG;
  if (n == 0) return 0;
  return verify_percall(ctx, pks48, n, msg, msg_len, sig96);
}

int bls_aggregate_verify(bls_ctx* ctx, const uint8_t* pks48, size_t n, const uint8_t* msgs, const size_t* msg_lens,
                         const uint8_t* sig96) {
  API_ENTER(ctx);
  if ((!pks48 || !msg_lens) && n) return BLS_E_ARG;
  if (!sig96) return BLS_E_ARG;
  if (n == 0) return 0;
  std::vector<uint64_t> offs(n + 1, 0);
  for (size_t i = 0; i < n; i++) {
    if (msg_lens[i] > 0xffffffffu) return BLS_E_ARG;
    offs[i + 1] = offs[i] + msg_lens[i];
  }
  if (offs[n] && !msgs) return BLS_E_ARG;
  // three streams as verify_percall: the signature's decode + subgroup check (stream3) and the n hashes
  // (stream2) run beside the keys' validation (stream1, which synchronises for the verdicts), the Miller loops
  // join them; a rejected signature is reported through its verdict word next to the FE result
  Job& J = *ctx->j;
  hipStream_t st = J.stream, st2 = J.stream2, st3 = J.stream3;
  uint8_t *d_sig, *d_msgs;
  uint64_t* d_offs;
  G2A* Q;
  int* d_w;
  Fp12 *f, *ft, *fo;
  Fd* d_hf;
  int* d_flag;
  SCR(S_IN1, 96, d_sig);
  SCR(S_IN2, offs[n], d_msgs);
  SCR(S_OFFS, n + 1, d_offs);
  SCR(S_G2A, n + 1, Q);
  SCR(S_INT, 4, d_w);  // sig verdict | FE verdict
  SCR(S_F, n + 1, f);
  SCR(S_F_T, (n + 1) / 8 + 16, ft);
  SCR(S_FPART, 1, fo);
  SCR(S_AV_HCF, h2c_scratch_fd(n), d_hf);
  SCR(S_AV_FLAG, n, d_flag);
  // the hashes in Jacobian coordinates when both the hash and the Miller loop take the wide kernels (no inversion
  // per message; Z of the signature's pair 1); not under the forced-fallback test hook (it rewrites H affine)
  Fp2* hz = nullptr;
  if (n <= WIDE_H2C_MAX && n + 1 <= WIDE_MILLER_MAX && !ctx->force_fb) SCR(S_G2A_B, n + 1, hz);
  CK(h2d(ctx, d_sig, sig96, 96));
  CK(h2d(ctx, d_msgs, msgs, offs[n]));
  CK(h2d(ctx, d_offs, offs.data(), (n + 1) * sizeof(uint64_t)));
  const hipStream_t ss = st3 != st2 ? st3 : ctx->pc_stream;  // two-stream job 0: the per-call stream (verify_percall)
  HIPCK(hipEventRecord(J.ev_fork, st));
  HIPCK(hipStreamWaitEvent(st2, J.ev_fork, 0));
  if (ss != st) HIPCK(hipStreamWaitEvent(ss, J.ev_fork, 0));
  LK(launch_sig_validate_wide(ss, d_sig, 1, Q + n, d_w));
  if (hz) {
    hipLaunchKernelGGL(k_set_fp2_one, dim3(1), dim3(64), 0, ss, hz + n);
    LK(hipGetLastError());
  }
  HIPCK(hipEventRecord(J.ev_sig, ss));
  bool m32 = true;  // all signing roots: the FAV batches' 32-byte h2c kernels (msgs are then 32 B apart)
  for (size_t i = 0; i < n && m32; i++) m32 = msg_lens[i] == 32;
  if (n <= WIDE_H2C_MAX)  // up to ~a thousand messages: one wide workgroup each, lower latency than the lane chains
    LK(launch_h2c_wide(st2, n, d_msgs, m32 ? nullptr : d_offs, Q, d_flag, hz));
  else if (m32)
    LK(launch_h2c(st2, n, d_msgs, nullptr, d_hf, Q, d_flag));
  else
    LK(launch_h2c_msgs(st2, n, d_msgs, d_offs, d_hf, Q, d_flag));
  CK(h2c_fallback(ctx, st2, n, d_msgs, m32 ? nullptr : d_offs, d_flag, Q));
  HIPCK(hipEventRecord(J.ev_join, st2));
  G1A* P;
  int* ok;
  const int v = validate_pks(ctx, pks48, n, &P, &ok);  // synchronises stream1
  if (v <= 0) {
    HIPCK(hipStreamSynchronize(st2));  // the scratch of the side streams is reused by the next call
    HIPCK(hipStreamSynchronize(ss));
    return v;
  }
  HIPCK(hipStreamWaitEvent(st, J.ev_sig, 0));
  HIPCK(hipStreamWaitEvent(st, J.ev_join, 0));
  hipLaunchKernelGGL(k_set_neg_g1, dim3(1), dim3(64), 0, st, P + n);
  LK(hipGetLastError());
  size_t nf = 0;
  LK(launch_miller_call(st, P, Q, n + 1, f, &nf, hz));  // a rejected signature: constant lines there
  LK(launch_fp12_prod_vm(st, f, nf, ft, fo));
  PROF2(7, st, launch_fe_wide(st, fo, 1, d_w + 1));
  int w[2] = {0, 0};
  CK(d2h(ctx, w, d_w, sizeof w));
  return (w[0] && w[1]) ? 1 : 0;
}

int bls_aggregate(bls_ctx* ctx, const uint8_t* sigs96, size_t n, uint8_t* out96) {
  API_ENTER(ctx);
  if ((!sigs96 && n) || !out96) return BLS_E_ARG;
  if (n == 0) return 0;
  uint8_t *d_in, *d_out;
  G2A* a;
  int* d_ok;
  G2J *tmp, *s;
  SCR(S_IN0, 96 * n, d_in);
  SCR(S_G2A, n, a);
  SCR(S_OK, n, d_ok);
  SCR(S_G2J_T, 1024, tmp);
  SCR(S_G2J, 1, s);
  SCR(S_IN1, 96, d_out);
  CK(h2d(ctx, d_in, sigs96, 96 * n));
  LK(launch_sig_validate(ctx->j->stream, d_in, n, a, d_ok));
  std::vector<int> ok(n);
  CK(d2h(ctx, ok.data(), d_ok, n * sizeof(int)));
  for (size_t i = 0; i < n; i++)
    if (!ok[i]) return 0;
  LK(launch_g2_sum_aff(ctx->j->stream, a, nullptr, n, tmp, s));
  LK(launch_g2_compress(ctx->j->stream, s, d_out));
  CK(d2h(ctx, out96, d_out, 96));
  return 1;
}

int bls_aggregate_pks(bls_ctx* ctx, const uint8_t* pks48, size_t n, uint8_t* out48) {
  API_ENTER(ctx);
  if ((!pks48 && n) || !out48) return BLS_E_ARG;
  if (n == 0) return 0;
  G1A* a;
  int* ok;
  int v = validate_pks(ctx, pks48, n, &a, &ok);
  if (v <= 0) return v;
  G1J *tmp, *s;
  uint8_t* d_out;
  SCR(S_G1J_T, 1024, tmp);
  SCR(S_G1J, 1, s);
  SCR(S_IN1, 48, d_out);
  LK(launch_g1_sum_aff(ctx->j->stream, a, nullptr, n, tmp, s));
  LK(launch_g1_compress(ctx->j->stream, s, d_out, nullptr));
  CK(d2h(ctx, out48, d_out, 48));
  return 1;
}

int bls_key_validate(bls_ctx* ctx, const uint8_t* pk48) {
  API_ENTER(ctx);
  if (!pk48) return BLS_E_ARG;
  G1A* a;
  int* ok;
  return validate_pks(ctx, pk48, 1, &a, &ok);
}

static int sign_impl(bls_ctx* ctx, const uint8_t* sks, const uint8_t* msgs, const uint64_t* offs, size_t n,
                     uint8_t* out96, int* all_ok) {
  uint8_t *d_sk, *d_m, *d_out;
  uint64_t* d_offs;
  int* d_ok;
  SCR(S_IN0, 32 * n, d_sk);
  SCR(S_IN1, offs[n], d_m);
  SCR(S_IN2, 96 * n, d_out);
  SCR(S_OFFS, n + 1, d_offs);
  SCR(S_OK, n, d_ok);
  CK(h2d(ctx, d_sk, sks, 32 * n));
  CK(h2d(ctx, d_m, msgs, offs[n]));
  CK(h2d(ctx, d_offs, offs, (n + 1) * sizeof(uint64_t)));
  LK(launch_sign_many(ctx->j->stream, d_sk, d_m, d_offs, n, d_out, d_ok));
  std::vector<int> ok(n);
  CK(d2h(ctx, ok.data(), d_ok, n * sizeof(int)));
  CK(d2h(ctx, out96, d_out, 96 * n));
  *all_ok = 1;
  for (size_t i = 0; i < n; i++)
    if (!ok[i]) *all_ok = 0;
  return 0;
}

int bls_sign(bls_ctx* ctx, const uint8_t* sk32, const uint8_t* msg, size_t msg_len, uint8_t* out96) {
  API_ENTER(ctx);
  if (!sk32 || !out96 || (!msg && msg_len) || msg_len > 0xffffffffu) return BLS_E_ARG;
  uint64_t offs[2] = {0, msg_len};
  int ok = 0;
  CK(sign_impl(ctx, sk32, msg, offs, 1, out96, &ok));
  return ok;
}

int bls_sign_batch(bls_ctx* ctx, const uint8_t* sks32, const uint8_t* msgs32, size_t B, uint8_t* out96) {
  API_ENTER(ctx);
  if ((!sks32 || !msgs32 || !out96) && B) return BLS_E_ARG;
  if (!B) return 1;
  std::vector<uint64_t> offs(B + 1);
  for (size_t i = 0; i <= B; i++) offs[i] = 32 * i;
  int ok = 0;
  CK(sign_impl(ctx, sks32, msgs32, offs.data(), B, out96, &ok));
  return ok;
}

static int sk_to_pk_impl(bls_ctx* ctx, const uint8_t* sks, size_t n, uint8_t* out48) {
  uint8_t *d_sk, *d_out;
  int* d_ok;
  SCR(S_IN0, 32 * n, d_sk);
  SCR(S_IN2, 48 * n, d_out);
  SCR(S_OK, n, d_ok);
  CK(h2d(ctx, d_sk, sks, 32 * n));
  LK(launch_sk_to_pk_many(ctx->j->stream, d_sk, n, d_out, d_ok));
  std::vector<int> ok(n);
  CK(d2h(ctx, ok.data(), d_ok, n * sizeof(int)));
  CK(d2h(ctx, out48, d_out, 48 * n));
  for (size_t i = 0; i < n; i++)
    if (!ok[i]) return 0;
  return 1;
}

int bls_sk_to_pk(bls_ctx* ctx, const uint8_t* sk32, uint8_t* out48) {
  API_ENTER(ctx);
  if (!sk32 || !out48) return BLS_E_ARG;
  return sk_to_pk_impl(ctx, sk32, 1, out48);
}

int bls_sk_to_pk_batch(bls_ctx* ctx, const uint8_t* sks32, size_t B, uint8_t* out48) {
  API_ENTER(ctx);
  if ((!sks32 || !out48) && B) return BLS_E_ARG;
  if (!B) return 1;
  return sk_to_pk_impl(ctx, sks32, B, out48);
}

int bls_hash_to_g2(bls_ctx* ctx, const uint8_t* msg, size_t msg_len, const uint8_t* dst, size_t dst_len,
                   uint8_t* out96) {
  API_ENTER(ctx);
  if (!out96 || (!msg && msg_len) || !dst || dst_len == 0 || dst_len > 255 || msg_len > 0xffffffffu) return BLS_E_ARG;
  uint8_t *d_m, *d_dst, *d_out;
  uint64_t* d_offs;
  G2A* h;
  SCR(S_IN0, msg_len, d_m);
  SCR(S_IN1, dst_len, d_dst);
  SCR(S_IN2, 96, d_out);
  SCR(S_OFFS, 2, d_offs);
  SCR(S_G2A, 1, h);
  uint64_t offs[2] = {0, msg_len};
  CK(h2d(ctx, d_m, msg, msg_len));
  CK(h2d(ctx, d_dst, dst, dst_len));
  CK(h2d(ctx, d_offs, offs, sizeof offs));
  LK(launch_hash_many(ctx->j->stream, d_m, d_offs, 1, d_dst, (uint32_t)dst_len, h));
  LK(launch_g2_compress_aff(ctx->j->stream, h, d_out));
  CK(d2h(ctx, out96, d_out, 96));
  return 1;
}

// ------------------------------------------------------------ test hooks --
// Route the items i < n with mask[i] != 0 of every later hash_to_G2 through k_h2c_fallback (the reference-path
// formulas) as if the lane kernels had flagged them; n = 0 clears.  The lane kernels flag only g(x1) = 0, g(x) in
// Fp, a vanishing isogeny denominator or an exceptional chain addition, none of which hash outputs reach in
// practice, so without this the routing and the fallback's overwrite of H[i] would go untested on the device.
int bls_test_force_h2c_fallback(bls_ctx* ctx, const uint8_t* mask, size_t n) {
  API_ENTER(ctx);
  if (!mask && n) return BLS_E_ARG;
  // the one hook that changes later calls' routing: refused unless the process opted in (tests/conftest.py)
  const char* opt = getenv("BLSMI355X_TEST_HOOKS");
  if (!opt || strcmp(opt, "1") != 0) {
    ctx->err = "bls_test_force_h2c_fallback needs BLSMI355X_TEST_HOOKS=1";
    return BLS_E_ARG;
  }
  HIPCK(hipDeviceSynchronize());
  if (ctx->force_fb) HIPCK(hipFree(ctx->force_fb));
  ctx->force_fb = nullptr;
  ctx->force_fb_n = 0;
  if (!n) return 0;
  std::vector<int> m(n);
  for (size_t i = 0; i < n; i++) m[i] = mask[i] ? 1 : 0;
  HIPCK(hipMalloc(&ctx->force_fb, n * sizeof(int)));
  HIPCK(hipMemcpy(ctx->force_fb, m.data(), n * sizeof(int), hipMemcpyHostToDevice));
  ctx->force_fb_n = n;
  return 0;
}

__global__ void k_g2_compress_many(size_t n, const G2A* in, uint8_t* out96) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) g2_compress(out96 + 96 * i, in[i]);
}

// hash_to_G2 of n 32-byte messages (DST POP) through the FAV batch's lane kernels and fallback routing
// (launch_h2c + h2c_fallback, exactly as bls_fav_* run them), compressed: out96[96 i ..] = H(m_i).
// the same through the one-wave-per-message kernel of the per-call path (launch_h2c_wide + h2c_fallback)
int bls_test_hash_to_g2_wide(bls_ctx* ctx, const uint8_t* msgs32, size_t n, uint8_t* out96) {
  API_ENTER(ctx);
  if ((!msgs32 || !out96) && n) return BLS_E_ARG;
  if (!n) return 0;
  uint8_t *d_m, *d_out;
  G2A* H;
  int* flag;
  SCR(S_IN0, 32 * n, d_m);
  SCR(S_IN2, 96 * n, d_out);
  SCR(S_AV_FLAG, n, flag);
  SCR(S_G2A, n, H);
  hipStream_t st = ctx->j->stream;
  CK(h2d(ctx, d_m, msgs32, 32 * n));
  LK(launch_h2c_wide(st, n, d_m, nullptr, H, flag));
  CK(h2c_fallback(ctx, st, n, d_m, nullptr, flag, H));
  hipLaunchKernelGGL(k_g2_compress_many, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, n, H, d_out);
  LK(hipGetLastError());
  CK(d2h(ctx, out96, d_out, 96 * n));
  return 0;
}

// final-exponentiation check of the product of n raw Fp12 values (576 bytes each: 12 little-endian Montgomery Fp,
// tower order) with the six-wave kernel (wide != 0) or the one-wave lane kernel: *out = 1 / 0
int bls_test_final_check(bls_ctx* ctx, const uint8_t* f576, size_t n, int wide, int32_t* out) {
  API_ENTER(ctx);
  if (!f576 || !out || !n || n > 64) return BLS_E_ARG;
  Fp12* d_f;
  int* d_r;
  SCR(S_F, n, d_f);
  SCR(S_INT, 4, d_r);
  hipStream_t st = ctx->j->stream;
  CK(h2d(ctx, d_f, f576, 576 * n));
  uint64_t* d_ts = nullptr;
  if (wide == 2) SCR(S_OFFS, 16, d_ts);
  if (wide)
    LK(launch_fe_wide(st, d_f, (int)n, d_r, d_ts));
  else
    LK(launch_final_check_wave(st, d_f, (int)n, d_r));
  CK(d2h(ctx, out, d_r, sizeof(int32_t)));
  if (d_ts) CK(d2h(ctx, out + 2, d_ts, 8 * 8));
  return 0;
}

// stages of the one-wave hash for one 32-byte message (k_h2c_wide_dbg): 33 x 48-byte little-endian raw Fp
int bls_test_h2c_wide_stages(bls_ctx* ctx, const uint8_t* msg32, uint8_t* out) {
  API_ENTER(ctx);
  if (!msg32 || !out) return BLS_E_ARG;
  uint8_t* d_m;
  Fp* d_out;
  SCR(S_IN0, 32, d_m);
  SCR(S_G2A, 100, d_out);
  CK(h2d(ctx, d_m, msg32, 32));
  LK(launch_h2c_wide_dbg(ctx->j->stream, d_m, d_out));
  CK(d2h(ctx, out, d_out, 72 * sizeof(Fp) + 320 * 4));
  return 0;
}

// The product of n pairings through each Miller-loop form of the batch path, final-exponentiated: out576[576 k ..]
// for form k = 0 split (k_miller_lines2 + k_miller_acc4q<2>), 1 fused G = 2, 2 fused G = 1, 3 split G = 4, 4 the
// wave-program kernel (the reference form of bls_multi_pairing), 5 split G = 8, 6 split G = 4 lines first
// (k_miller_acc4l), 7 split G = 1 on eight lanes per f (k_miller_acc8).  Points are decoded without subgroup checks;
// identity points are skipped pairs.  Returns 1, or 0 if an encoding is invalid.
int bls_test_miller_forms(bls_ctx* ctx, const uint8_t* g1s48, const uint8_t* g2s96, size_t n, uint8_t* out576) {
  API_ENTER(ctx);
  if (!n || !g1s48 || !g2s96 || !out576) return BLS_E_ARG;
  hipStream_t st = ctx->j->stream;
  uint8_t *d_in, *d_out;
  G1A* P;
  G2A* Q;
  int *ok1, *ok2;
  Fp12 *f, *ft, *fo;
  uint32_t* L;
  SCR(S_KZ_IN, 144 * n, d_in);
  SCR(S_KZ_P, n, P);
  SCR(S_KZ_Q, n, Q);
  SCR(S_KZ_OK, n, ok1);
  SCR(S_KZ_OK2, n, ok2);
  SCR(S_KZ_F, n, f);
  SCR(S_KZ_FT, n / 8 + 16, ft);
  SCR(S_FPART, 1, fo);
  SCR(S_PT_OUT, 8 * 576, d_out);
  SCR(S_KZ_J, miller_lines_u32(n), L);
  CK(h2d(ctx, d_in, g1s48, 48 * n));
  CK(h2d(ctx, d_in + 48 * n, g2s96, 96 * n));
  LK(launch_pt_decode(st, 1, d_in, n, 0, P, ok1));
  LK(launch_pt_decode(st, 2, d_in + 48 * n, n, 0, Q, ok2));
  std::vector<int> a(n), b(n);
  CK(d2h(ctx, a.data(), ok1, n * sizeof(int)));
  CK(d2h(ctx, b.data(), ok2, n * sizeof(int)));
  for (size_t i = 0; i < n; i++)
    if (!a[i] || !b[i]) return 0;
  for (int k = 0; k < 8; ++k) {
    size_t nf = n;
    if (k == 7) {
      LK(launch_miller_lines(st, Q, n, L));
      LK(launch_miller_acc8(st, P, Q, nullptr, n, L, miller_lines_ld(n), f));
    } else if (k == 6) {
      LK(launch_miller_lines(st, Q, n, L));
      LK(launch_miller_acc4l(st, P, Q, nullptr, n, L, miller_lines_ld(n), f));
      nf = (n + 3) / 4;
    } else if (k == 0 || k == 3 || k == 5) {
      const int G = k == 0 ? 2 : (k == 3 ? 4 : 8);
      LK(launch_miller_lines(st, Q, n, L));
      LK(launch_miller_acc4(st, P, Q, nullptr, n, L, miller_lines_ld(n), f, G));
      nf = (n + G - 1) / G;
    } else if (k == 1 || k == 2) {
      const int G = k == 1 ? 2 : 1;
      LK(launch_miller_fused(st, P, Q, nullptr, n, f, G));
      nf = (n + G - 1) / G;
    } else {
      LK(launch_miller_wave(st, P, Q, nullptr, n, f));
    }
    LK(launch_fp12_prod_vm(st, f, nf, ft, fo));
    LK(launch_gt_final_exp(st, fo, d_out + 576 * k));
  }
  CK(d2h(ctx, out576, d_out, 8 * 576));
  return 1;
}

int bls_test_hash_to_g2_batch(bls_ctx* ctx, const uint8_t* msgs32, size_t n, uint8_t* out96) {
  API_ENTER(ctx);
  if ((!msgs32 || !out96) && n) return BLS_E_ARG;
  if (!n) return 0;
  uint8_t *d_m, *d_out;
  Fd* hf;
  G2A* H;
  int* flag;
  SCR(S_IN0, 32 * n, d_m);
  SCR(S_IN2, 96 * n, d_out);
  SCR(S_AV_HCF, h2c_scratch_fd(n), hf);
  SCR(S_AV_FLAG, n, flag);
  SCR(S_G2A, n, H);
  hipStream_t st = ctx->j->stream;
  CK(h2d(ctx, d_m, msgs32, 32 * n));
  LK(launch_h2c(st, n, d_m, nullptr, hf, H, flag));
  CK(h2c_fallback(ctx, st, n, d_m, nullptr, flag, H));
  hipLaunchKernelGGL(k_g2_compress_many, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, n, H, d_out);
  LK(hipGetLastError());
  CK(d2h(ctx, out96, d_out, 96 * n));
  return 0;
}

// Device self-test of the wavefront-cooperative products (bls_wide.h) against the lane form: nw waves, each on four
// inputs (48-byte big-endian integers < p); bad[w] = bitmask of the forms whose results differ (0 = all equal).
int bls_test_wide_selftest(bls_ctx* ctx, const uint8_t* in48, size_t nw, int32_t* bad) {
  API_ENTER(ctx);
  if ((!in48 || !bad) && nw) return BLS_E_ARG;
  if (!nw) return 0;
  uint8_t* d_in;
  int* d_bad;
  SCR(S_IN0, 4 * 48 * nw, d_in);
  SCR(S_OK, nw, d_bad);
  CK(h2d(ctx, d_in, in48, 4 * 48 * nw));
  LK(launch_wide_selftest(ctx->j->stream, nw, d_in, d_bad));
  CK(d2h(ctx, bad, d_bad, nw * sizeof(int)));
  return 0;
}

// ------------------------------------------------------------- registry --
// Decode + KeyValidate n keys into reg[first ..] (valid[] = the verdicts).
static int registry_fill(bls_ctx* ctx, const uint8_t* pks48, size_t n, size_t first, uint8_t* out_valid) {
  uint8_t *d_in, *d_valid;
  G1A* d_a;
  int* d_ok;
  SCR(S_IN0, 48 * n, d_in);
  SCR(S_G1A, n, d_a);
  SCR(S_OK, n, d_ok);
  SCR(S_IN3, n, d_valid);
  CK(h2d(ctx, d_in, pks48, 48 * n));
  PROF(13, launch_key_validate(ctx->j->stream, d_in, n, d_a, d_ok));
  LK(launch_reg_pack(ctx->j->stream, d_a, d_ok, n, ctx->reg + first, d_valid));
  if (out_valid) CK(d2h(ctx, out_valid, d_valid, n));
  HIPCK(hipStreamSynchronize(ctx->j->stream));
  return 0;
}

// A new registry replaces the old one: wait for every job's batches that may
// still read it.
static int registry_replace(bls_ctx* ctx, size_t n) {
  HIPCK(hipDeviceSynchronize());
  if (ctx->reg) HIPCK(hipFree(ctx->reg));
  ctx->reg = nullptr;
  ctx->reg_n = 0;
  ctx->reg_gen++;
  HIPCK(hipMalloc(&ctx->reg, (n ? n : 1) * sizeof(RegKey)));
  ctx->reg_cap = n ? n : 1;
  return 0;
}

int bls_registry_load(bls_ctx* ctx, const uint8_t* pks48, size_t n, uint8_t* out_valid) {
  API_ENTER(ctx);
  if (!pks48 && n) return BLS_E_ARG;
  if (n > 0xffffffffu) return BLS_E_ARG;
  CK(registry_replace(ctx, n));
  if (n) CK(registry_fill(ctx, pks48, n, 0, out_valid));
  ctx->reg_n = n;
  return 1;
}

int bls_registry_append(bls_ctx* ctx, const uint8_t* pks48, size_t n, uint8_t* out_valid) {
  API_ENTER(ctx);
  if (!pks48 && n) return BLS_E_ARG;
  if (ctx->reg_n + n > 0xffffffffu) return BLS_E_ARG;
  if (n == 0) return 1;
  const size_t need = ctx->reg_n + n;
  if (need > ctx->reg_cap) {  // grow by >= 1/4 so a run of deposits reallocates rarely
    HIPCK(hipDeviceSynchronize());  // batches in flight on any job read the old table
    size_t cap = ctx->reg_cap + ctx->reg_cap / 4;
    if (cap < need) cap = need;
    RegKey* nreg;
    HIPCK(hipMalloc(&nreg, cap * sizeof(RegKey)));
    if (ctx->reg_n) {
      HIPCK(hipMemcpyAsync(nreg, ctx->reg, ctx->reg_n * sizeof(RegKey), hipMemcpyDeviceToDevice, ctx->j->stream));
      HIPCK(hipStreamSynchronize(ctx->j->stream));
    }
    if (ctx->reg) HIPCK(hipFree(ctx->reg));
    ctx->reg = nreg;
    ctx->reg_cap = cap;
  }
  CK(registry_fill(ctx, pks48, n, ctx->reg_n, out_valid));
  ctx->reg_n = need;
  return 1;
}

size_t bls_registry_size(bls_ctx* ctx) { return ctx ? ctx->reg_n : 0; }

int bls_registry_generate(bls_ctx* ctx, uint64_t first_sk, size_t n, uint8_t* out_pks48) {
  API_ENTER(ctx);
  if (n > 0xffffffffu || first_sk == 0 || first_sk + n < first_sk || first_sk + n >= (1ull << 62)) return BLS_E_ARG;
  CK(registry_replace(ctx, n));
  G1J* tmp;
  uint8_t* d_out = nullptr;
  SCR(S_G1J_T, n, tmp);
  if (out_pks48) SCR(S_IN0, 48 * n, d_out);
  LK(launch_registry_generate(ctx->j->stream, first_sk, n, tmp, ctx->reg, d_out));
  if (out_pks48) CK(d2h(ctx, out_pks48, d_out, 48 * n));
  HIPCK(hipStreamSynchronize(ctx->j->stream));
  ctx->reg_n = n;
  return 1;
}

uint64_t bls_registry_generation(bls_ctx* ctx) { return ctx ? ctx->reg_gen : 0; }

// ------------------------------------------------------ committee table --
// The lists and their offsets stay in HBM; one launch of the bits gather over the table itself (every committee a
// direct item whose list is its members) gives csum[c], and its members_ok output is cstat[c] -- apart from the
// identity check, so an empty committee or one whose keys cancel is usable (cstat 1) with the identity as its sum.
int bls_committees_load(bls_ctx* ctx, const uint32_t* idx, const uint64_t* offsets, size_t C) {
  API_ENTER(ctx);
  if (!ctx->reg || !ctx->reg_n) {
    ctx->err = "no registry loaded";
    return BLS_E_NOREG;
  }
  if (!offsets || C >= 0x80000000u) return BLS_E_ARG;
  for (size_t c = 0; c < C; c++)
    if (offsets[c + 1] < offsets[c] || offsets[c + 1] - offsets[c] > 0xffffffffull) return BLS_E_ARG;
  const uint64_t o0 = offsets[0], total = offsets[C] - o0;
  if (total && !idx) return BLS_E_ARG;
  HIPCK(hipDeviceSynchronize());  // batches in flight on any job read the old table
  ctx->ctab_loaded = false;
  for (void** p : {(void**)&ctx->ctab_idx, (void**)&ctx->ctab_offs, (void**)&ctx->ctab_sum, (void**)&ctx->ctab_stat}) {
    if (*p) HIPCK(hipFree(*p));
    *p = nullptr;
  }
  HIPCK(hipMalloc(&ctx->ctab_idx, (total ? total : 1) * 4));
  HIPCK(hipMalloc(&ctx->ctab_offs, (C + 1) * 8));
  HIPCK(hipMalloc(&ctx->ctab_sum, (C ? C : 1) * sizeof(G1P)));
  HIPCK(hipMalloc(&ctx->ctab_stat, (C ? C : 1) * sizeof(int)));
  ctx->ctab_offs_h.resize(C + 1);
  std::vector<BitsItem> items(C);
  for (size_t c = 0; c <= C; c++) ctx->ctab_offs_h[c] = offsets[c] - o0;
  for (size_t c = 0; c < C; c++)
    items[c] = BitsItem{ctx->ctab_offs_h[c], (uint32_t)(ctx->ctab_offs_h[c + 1] - ctx->ctab_offs_h[c]), BITS_F_SOME};
  BitsItem* d_items;
  int* d_st;
  ctx->j->bits_B = 0;  // the slot's item records become the table's: no batch's work is left to read there
  SCR(S_BITEM, C, d_items);
  SCR(S_OK, C, d_st);
  hipStream_t st = ctx->j->stream;
  if (total) HIPCK(hipMemcpyAsync(ctx->ctab_idx, idx + o0, total * 4, hipMemcpyHostToDevice, st));
  HIPCK(hipMemcpyAsync(ctx->ctab_offs, ctx->ctab_offs_h.data(), (C + 1) * 8, hipMemcpyHostToDevice, st));
  if (C) HIPCK(hipMemcpyAsync(d_items, items.data(), C * sizeof(BitsItem), hipMemcpyHostToDevice, st));
  LK(launch_fav_gather_bits(st, ctx->ctab_idx, d_items, C, ctx->reg, (uint32_t)ctx->reg_n, nullptr, nullptr, nullptr,
                            ctx->ctab_sum, d_st, ctx->ctab_stat));
  HIPCK(hipStreamSynchronize(st));
  ctx->ctab_gen = ctx->reg_gen;
  ctx->ctab_loaded = true;
  return 1;
}

size_t bls_committees_count(bls_ctx* ctx) {
  return (ctx && ctx->ctab_loaded) ? ctx->ctab_offs_h.size() - 1 : 0;
}

int bls_profile_enable(bls_ctx* ctx, int on) {
  API_ENTER(ctx);
  HIPCK(hipStreamSynchronize(ctx->j->stream));
  prof_collect(ctx);
  ctx->prof_on = on != 0;
  for (int i = 0; i < 16; i++) {
    ctx->prof_ms[i] = 0;
    ctx->prof_cnt[i] = 0;
  }
  return 0;
}

int bls_profile_read(bls_ctx* ctx, double* total_ms, uint64_t* counts, int max) {
  API_ENTER(ctx);
  HIPCK(hipStreamSynchronize(ctx->j->stream));
  prof_collect(ctx);
  int n = max < PROF_N ? max : PROF_N;
  for (int i = 0; i < n; i++) {
    if (total_ms) total_ms[i] = ctx->prof_ms[i];
    if (counts) counts[i] = ctx->prof_cnt[i];
  }
  return PROF_N;
}

const char* bls_profile_name(int i) { return (i >= 0 && i < PROF_N) ? PROF_NAMES[i] : ""; }

// ---------------------------------------------------------- FAV batches --
// A FAV batch's Miller loops run split -- the line kernel on stream2 right after the hash, the f accumulation on
// stream1 -- or, with BLS_MILLER_FUSED=1, as one fused kernel (k_miller_fused).  The fused kernel holds a SIMD per
// line wave for the whole loop, so per batch it costs more SIMD time than the two kernels at full occupancy (C2
// 2.32 -> 2.14 M FAV/s, C3 1.51 -> 1.46 M: profiles/r05o_miller_fused_ab.txt) although its launch alone runs the
// Miller loop at 0.0995 of peak against the accumulation kernel's 0.070; the latency-bound callers -- the
// bisection's per-item values and AggregateVerify batches -- always take it.
static bool miller_fused() {
  static const bool on = getenv("BLS_MILLER_FUSED") && !strcmp(getenv("BLS_MILLER_FUSED"), "1");
  return on;
}
constexpr size_t ACC8_MAX = 2048;  // items per FAV batch below which one pair per f runs on eight lanes
constexpr size_t ACC_SHARED_MIN = 4096;  // items per FAV batch from which k_miller_acc4q shares f between two pairs

// msg_id (host, B entries, nullable) / M: a shared-message batch -- d_msgs is a table of M messages and item i signs
// entry msg_id[i].  The per-item stages (gather, decode, r_i apk_i chains, MSM) run over the B items as ever; the
// per-message stages (hash_to_G2, G2 lines, f accumulation) run over M + MSM_UPAIRS pairs whose G1 side is the
// segmented sum of the items' r_i apk_i (bls_g1_segsum.h), and the kernel-form thresholds key on M.  Without a
// grouping (every existing entry point) the launches are what they always were.
//
// bits (nullable): the items are (committees, participation bits) over the context's committee table instead of
// index lists (d_idx / d_offs unused).  bits_plan has checked the arguments and left the host tables in the job;
// a pre-stage expands every item into the list its gather adds, and the gather variant of bls_gather_bits.hip
// writes the same apka / gstat the index gather would have written for the expanded list.  Nothing after them
// knows the difference.  Without bits the launches are what they always were.
struct BitsArgs {
  const uint8_t* d_bits;  // device: the items' bit bytes, item b at bit_offs[b]
  int mode;
};

// The host half of a bits batch, before any device call: every committee id names a table entry, item b carries
// exactly ceil(n_b / 8) bytes (n_b the members of its committees), and the table is the registry's.  Leaves the
// job-owned copies (committee ids rebased to 0, comm_offs | bit_offs | slot_offs) that fav_prepare uploads.
static int bits_plan(bls_ctx* ctx, const uint32_t* comm_ids, const uint64_t* comm_offs, const uint64_t* bit_offs,
                     size_t B, int mode) {
  if (!ctx->ctab_loaded) {
    ctx->err = "no committee table loaded (bls_committees_load)";
    return BLS_E_ARG;
  }
  if (ctx->ctab_gen != ctx->reg_gen) {
    ctx->err = "the committee table is stale: the registry was replaced after bls_committees_load";
    return BLS_E_ARG;
  }
  if (mode != BITS_MODE_AUTO && mode != BITS_MODE_DIRECT && mode != BITS_MODE_COMPLEMENT) {
    ctx->err = "mode must be 0 (auto), 1 (direct) or 2 (complement)";
    return BLS_E_ARG;
  }
  if (!comm_offs || !bit_offs) return BLS_E_ARG;
  const size_t C = ctx->ctab_offs_h.size() - 1;
  const uint64_t c0 = comm_offs[0];
  for (size_t b = 0; b < B; b++)
    if (comm_offs[b + 1] < comm_offs[b] || bit_offs[b + 1] < bit_offs[b]) return BLS_E_ARG;
  const uint64_t ncomm = comm_offs[B] - c0;
  if (ncomm && !comm_ids) return BLS_E_ARG;
  Job& J = *ctx->j;
  std::vector<uint64_t>& n = J.bits_n;
  n.resize(B);
  for (size_t b = 0; b < B; b++) {
    n[b] = 0;
    for (uint64_t j = comm_offs[b]; j < comm_offs[b + 1]; j++) {
      const uint32_t c = comm_ids[j];
      if (c >= C) {
        ctx->err = "committee id out of range";
        return BLS_E_ARG;
      }
      n[b] += ctx->ctab_offs_h[c + 1] - ctx->ctab_offs_h[c];
    }
    if (n[b] > 0xffffffffull || bit_offs[b + 1] - bit_offs[b] != (n[b] + 7) / 8) {
      ctx->err = "an item needs ceil(n / 8) bytes of bits for the n members of its committees";
      return BLS_E_ARG;
    }
  }
  // the arguments stand: now the job's tables (an upload still in flight reads the old ones)
  J.bits_B = 0;
  if (J.bits_up_pending) {
    HIPCK(hipEventSynchronize(J.ev_bits));
    J.bits_up_pending = false;
  }
  const size_t bytes = 3 * (B + 1) * 8 + ncomm * 4;
  if (J.bits_tab_cap < bytes) {
    if (J.bits_tab) HIPCK(hipHostFree(J.bits_tab));
    J.bits_tab = nullptr;
    J.bits_tab_cap = 0;
    HIPCK(hipHostMalloc((void**)&J.bits_tab, bytes + bytes / 4, hipHostMallocDefault));
    J.bits_tab_cap = bytes + bytes / 4;
  }
  J.bits_tab_bytes = bytes;
  uint64_t* co = J.bits_tab;
  uint64_t *bo = co + (B + 1), *so = bo + (B + 1);
  so[0] = 0;
  for (size_t b = 0; b < B; b++) so[b + 1] = so[b] + n[b];
  for (size_t b = 0; b <= B; b++) {
    co[b] = comm_offs[b] - c0;
    bo[b] = bit_offs[b];
  }
  if (ncomm) memcpy(so + (B + 1), comm_ids + c0, ncomm * 4);
  return 0;
}

static int fav_prepare(bls_ctx* ctx, const uint32_t* d_idx, const uint64_t* d_offs, size_t B, const uint8_t* d_msgs,
                       const uint8_t* d_sigs, const uint8_t* seed32, Fp12** out_f, size_t M = 0,
                       const uint32_t* msg_id = nullptr, const BitsArgs* bits = nullptr) {
  if (!ctx->reg || !ctx->reg_n) {
    ctx->err = "no registry loaded";
    return BLS_E_NOREG;
  }
  const bool shared = msg_id != nullptr;
  if (shared) {  // the plan first: a bad id is refused before any device call
    Job& Jp = *ctx->j;
    if (!seg_plan(msg_id, B, M, Jp.seg)) {
      ctx->err = "msg_id out of range (or an empty message table)";
      return BLS_E_ARG;
    }
    Jp.seg_ids.assign(msg_id, msg_id + B);
  }
  const size_t NH = shared ? M : B;  // messages hashed = pairs of the H side
  // pairs 0 .. B: (r_i apk_i, H_i); pairs B .. B + 64: (-w_b G1, U_b), the MSM's bit-sums (bls_msm.hip).  The 64
  // scalar bits read as r_i = a + b lambda (a the low, b the high half; lambda = -x^2 mod r, phi's eigenvalue on
  // G1): bit b weighs w_b = 2^b below 32 and 2^(b - 32) lambda above, on both sides (bls_g1_endo.h, the comb)
  const size_t NP = NH + MSM_UPAIRS;
  int *status, *gstat, *flag, *dstat;
  G1P *apka, *rpj;
  G1A* rP;
  G2A *sig, *H;
  Fp12 *f, *ft, *fo;
  Fd *msmf, *hcf;
  uint64_t* rsc;
  uint32_t* msmu;
  uint8_t* d_seed;
  SCR(S_STATUS, shared ? B : NP, status);
  SCR(S_GSTAT, B, gstat);
  SCR(S_APKA, B, apka);
  SCR(S_SIG, B, sig);
  SCR(S_RP, shared ? B : NP, rP);
  SCR(S_H, NP, H);
  SCR(S_FLAG, NH, flag);
  SCR(S_RSC, B, rsc);
  SCR(S_MSMU, msm_scratch_u32(B), msmu);
  SCR(S_MSMF, msm_scratch_fd(), msmf);
  SCR(S_HCF, h2c_scratch_fd(NH), hcf);
  SCR(S_RPJ, B, rpj);
  // the Miller pairs' status and G1 side: the item arrays themselves, [0, B) items then the MSM pairs -- or, shared,
  // arrays of their own, [0, M) group sums then the MSM pairs, beside item arrays of B
  int* pstat = status;
  G1A* pP = rP;
  G1P *gsum = nullptr, *sega = nullptr, *segb = nullptr;
  SegRun* d_runs = nullptr;
  uint32_t *d_items = nullptr, *d_msgid = nullptr;
  if (shared) {
    const SegPlan& sp = ctx->j->seg;
    SCR(S_PSTAT, NP, pstat);
    SCR(S_GP, NP, pP);
    SCR(S_GSUM, M, gsum);
    SCR(S_SEGA, sp.max_tmp(), sega);
    SCR(S_SEGB, sp.levels() > 1 ? sp.level_tmp[1] : 0, segb);
    SCR(S_SEGRUN, sp.runs.size(), d_runs);
    SCR(S_SEGIT, B, d_items);
    SCR(S_MSGID, B, d_msgid);
  }
  // Miller loop of all NP pairs, split: G2 lines (k_miller_lines2) on stream2 after hash_to_G2 and the MSM, f
  // accumulated on stream1 by k_miller_acc4q (four lanes per f, G pairs per f: one squaring per step for all G)
  uint32_t* mlines = nullptr;
  if (!miller_fused()) SCR(S_MLINES, miller_lines_u32(NP), mlines);
  SCR(S_MSTAT, B, dstat);
  SCR(S_FAV_F, NP, f);  // per-item (or per-group) f, kept for the bisection: not S_F, which per-call checks use
  SCR(S_FAV_FT, NP / 8 + 16, ft);
  SCR(S_FPART, 1, fo);
  SCR(S_SEED, 32, d_seed);
  Job& J = *ctx->j;
  hipStream_t st = J.stream, st2 = J.stream2, st3 = J.stream3;
  if (!ctx->comb) {  // the -G1 comb (bls_bisect.hip): the MSM pairs' -w_b G1 and the bisection's -r_i G1
    G1A* tab = nullptr;
    HIPCK(hipMalloc(&tab, neg_g1_comb_entries() * sizeof(G1A)));
    hipError_t e = launch_neg_g1_comb_table(st, tab);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {  // never keep a table whose build did not complete
      (void)hipFree(tab);
      return fail(ctx, e, "launch_neg_g1_comb_table");
    }
    ctx->comb = tab;
  }
  // the job's own-product verdict belongs to the batch job_submit prepares; any other batch prepared on this slot
  // (the host-buffer calls on job 0) invalidates it
  J.own_pending = false;
  J.own_state = -1;
  J.comm_pending = false;
  // a two-stream job (stream3 == stream2, BLS_JOB_STREAMS=2, the default): the decode and the MSM run on stream1
  // around the gather, off the hash -> lines chain of stream2
  const bool two = st3 == st2;
  hipStream_t sd = two ? st : st3;
  // the branches fork from stream1's tail -- or, after a bisection still running there, from the point where it
  // has copied everything it reads of the state stream2 / stream3 write (fav_bisect); the seed goes on the
  // decode's stream, its reader, so the fork need not follow stream1
  if (shared) {
    // the grouping's tables on stream1, behind anything (a bisection's per-item H gather) that still reads the
    // previous ids; the branches then fork from here, not from a bisection's ev_bis
    const SegPlan& sp = J.seg;
    HIPCK(hipMemcpyAsync(d_msgid, J.seg_ids.data(), B * 4, hipMemcpyHostToDevice, st));
    HIPCK(hipMemcpyAsync(d_items, sp.grp_items.data(), B * 4, hipMemcpyHostToDevice, st));
    HIPCK(hipMemcpyAsync(d_runs, sp.runs.data(), sp.runs.size() * sizeof(SegRun), hipMemcpyHostToDevice, st));
    J.bis_pending = false;
  }
  J.fav_shared = shared;
  HIPCK(hipMemcpyAsync(d_seed, seed32, 32, hipMemcpyHostToDevice, sd));
  // Branches, three streams:
  //   stream1: registry gather (affine apk) -> subgroup / r_i apk_i chains -> f accumulation
  //   stream2: hash_to_G2 of every message -> (after the MSM) the G2 lines of all NP pairs
  //   stream3: signature decompression + RLC scalars -> MSM bit-sums U_b of S = sum r_i sigma_i
  // two streams: stream3's work on stream1 (decode before the gather, MSM after it)
  hipEvent_t fork = J.ev_fork;
  if (J.bis_pending) {
    fork = J.ev_bis;
    J.bis_pending = false;
  } else {
    HIPCK(hipEventRecord(fork, st));
  }
  HIPCK(hipStreamWaitEvent(st2, fork, 0));
  if (!two) HIPCK(hipStreamWaitEvent(st3, fork, 0));
  uint32_t* d_list = nullptr;
  uint64_t* d_tab = nullptr;
  BitsItem* d_bitems = nullptr;
  if (bits) {
    // (committees, bits) items, the pre-stage: the job's tables up in one copy, then one wave per item expands it
    // into its index list at the slot the host computed (the prefix sum of the member counts).  On stream2, in
    // front of the hash -- whose chain waits for the MSM anyway -- so that the expansion runs beside the signature
    // decode instead of in front of the gather: a job's latency, which a fixed pipeline depth turns into
    // throughput, stays what the index form's is.  The gather waits for ev_bits.
    SCR(S_BTAB, (J.bits_tab_bytes + 7) / 8, d_tab);
    SCR(S_BLIST, J.bits_tab[3 * (B + 1) - 1], d_list);
    SCR(S_BITEM, B, d_bitems);
    HIPCK(hipMemcpyAsync(d_tab, J.bits_tab, J.bits_tab_bytes, hipMemcpyHostToDevice, st2));
    const uint32_t* d_comm = reinterpret_cast<const uint32_t*>(d_tab + 3 * (B + 1));
    PROF2(14, st2, launch_bits_expand(st2, B, bits->mode, d_comm, d_tab, bits->d_bits, d_tab + (B + 1),
                                      d_tab + 2 * (B + 1), ctx->ctab_idx, ctx->ctab_offs, ctx->ctab_stat, d_list,
                                      d_bitems));
    HIPCK(hipEventRecord(J.ev_bits, st2));
    J.bits_up_pending = true;
  }
  PROF2(2, st2, launch_h2c(st2, NH, d_msgs, nullptr, hcf, H, flag));
  CK(h2c_fallback(ctx, st2, NH, d_msgs, nullptr, flag, H));
  if (shared)
    PROF2(1, sd, launch_sig_decode_idx(sd, B, d_msgs, d_msgid, d_sigs, d_seed, sig, rsc, dstat));
  else
    PROF2(1, sd, launch_sig_decode(sd, B, d_msgs, d_sigs, d_seed, sig, rsc, dstat));
  HIPCK(hipEventRecord(J.ev_sig, sd));
  // the registry gather: the complete-formula kernel (k_fav_gather_q; 204 registers by the compiler's report, two
  // waves per SIMD), or with BLS_GATHER=affine (read per batch) affine additions sharing one inversion per level
  // (bls_gather_aff.hip: 42 % fewer VALU instructions per aggregate, 234 registers; C2 measured the same within
  // +-1 % over three A/Bs, profiles/r06_gather_ab.txt); aggregates with an exceptional pair are redone by the
  // complete formulas.  The gather is not free: 2,500 waves of a C2 batch, 30 % of the instructions the batch issues
  // and about a quarter of a C2 step (C2 / C4 = 1.39 per item, the work model's 1.38).  The affine
  // A/B did not show that because its waves held their SIMDs alone, 28.5 % of the time waiting on HBM level lists
  // (~790 exclusive SIMD-ms, as much as it saved); cutting the complete kernel's own instructions by 15.8 % (one
  // reduction per output coordinate, bls_fq_g1.h) gained C2 3.1 % (profiles/g1dot_ab.txt).
  const char* gv = getenv("BLS_GATHER");
  const size_t gw = (gv && !strcmp(gv, "affine") && !bits) ? fav_gather_aff_words(B) : 0;
  if (bits) {
    // the gather variant sums the expanded lists -- and, for complement items, subtracts them from the committees'
    // cached sums.  The affine gather has no such form.
    HIPCK(hipStreamWaitEvent(st, J.ev_bits, 0));
    PROF(0, launch_fav_gather_bits(st, d_list, d_bitems, B, ctx->reg, (uint32_t)ctx->reg_n,
                                   reinterpret_cast<const uint32_t*>(d_tab + 3 * (B + 1)), d_tab, ctx->ctab_sum, apka,
                                   gstat, nullptr));
    J.bits_B = B;
    J.bits_items = d_bitems;
    ctx->work_job = &J;
  } else if (gw) {
    uint32_t* gscr;
    int* redo;
    SCR(S_GAFF, gw, gscr);
    SCR(S_GREDO, B, redo);
    PROF(0, launch_fav_gather_aff(st, d_idx, d_offs, B, ctx->reg, (uint32_t)ctx->reg_n, apka, gstat, gscr, redo));
    LK(launch_fav_gather_redo(st, d_idx, d_offs, B, ctx->reg, (uint32_t)ctx->reg_n, apka, gstat, redo));
  } else {
    PROF(0, launch_fav_gather(st, d_idx, d_offs, B, ctx->reg, (uint32_t)ctx->reg_n, apka, gstat));
  }
  HIPCK(hipEventRecord(J.ev_gather, st));
  // The MSM covers every decoded signature of a valid aggregate key, before
  // the subgroup checks: a decodable signature outside G2 stays in S, so the
  // batch check fails and fav_finish re-checks every item individually.  It
  // reads only gstat (gather) and dstat (decode), which no kernel writes
  // after ev_gather / ev_sig; the subgroup verdicts go to `status`, written on
  // stream1 while (or after) the MSM runs.
  hipStream_t sm = two ? st : st3;
  if (!two) HIPCK(hipStreamWaitEvent(sm, J.ev_gather, 0));
  PROF2(11, sm, launch_msm_upairs(sm, B, gstat, dstat, rsc, sig, msmu, msmf, ctx->comb, pP + NH, H + NH, pstat + NH));
  HIPCK(hipEventRecord(J.ev_msm, sm));
  // the Miller loops of all NP pairs: the G2 lines on stream2 after the hash and the MSM, then the f accumulation on
  // stream1 -- or (BLS_MILLER_FUSED=1) one fused kernel (k_miller_fused, lines in LDS) on stream1
  const bool fused = miller_fused();
  if (!fused) {
    HIPCK(hipStreamWaitEvent(st2, J.ev_msm, 0));
    PROF2(12, st2, launch_miller_lines(st2, H, NP, mlines));
  }
  HIPCK(hipEventRecord(J.ev_join, st2));
  if (!two) HIPCK(hipStreamWaitEvent(st, J.ev_sig, 0));
  PROF(10, launch_sig_vm(st, B, gstat, status, dstat, apka, sig, rsc, rpj, rP));
  if (shared) {
    // the segmented sum of the items' affine r_i apk_i into one point per message: a launch per fold level, the
    // partial arrays alternating, then the M sums to affine (ok 0 -- an empty, rejected or cancelling group --
    // gives .inf, a dead pair whose factor is 1)
    const SegPlan& sp = J.seg;
    for (size_t l = 0; l < sp.levels(); ++l) {
      const uint32_t n = sp.level_off[l + 1] - sp.level_off[l];
      G1P *in = (l & 1) ? sega : segb, *out = (l & 1) ? segb : sega;
      LK(launch_g1_seg_fold(st, (int)l, d_runs + sp.level_off[l], n, d_items, status, rP, in, out, gsum, pstat));
    }
    LK(launch_g1_affine(st, M, pstat, gsum, pP));
  }
  HIPCK(hipStreamWaitEvent(st, J.ev_join, 0));
  if (fused && !two) HIPCK(hipStreamWaitEvent(st, J.ev_msm, 0));
  // four pairs share each f (one squaring per step for all four) on full batches: the least work per pair, and
  // the pipeline is bound by work (C2 +3.0 % over two pairs per f, profiles/r06a_g4_ab.txt, although the launch
  // fills only 0.15 of the SIMDs); below ACC_SHARED_MIN items the launch under-fills the chip and the chain latency
  // is what counts, so one pair per f (a step is a squaring and ONE line: ~37 % shorter chains for ~24 % more
  // products).  Knob BLS_ACC_G = 1 / 2 / 4 / 8.
  static const int acc_g = getenv("BLS_ACC_G") ? atoi(getenv("BLS_ACC_G")) : 4;  // pairs per f of full batches
  static const size_t shared_min = getenv("BLS_ACC_SHARED_MIN") ? (size_t)atol(getenv("BLS_ACC_SHARED_MIN"))
                                                                : ACC_SHARED_MIN;
  const int mg = NH >= shared_min ? (acc_g == 8 || acc_g == 4 || acc_g == 1 ? acc_g : 2) : 1;
  J.fav_mg = mg;
  // knob BLS_ACC_LL = 1: G = 4 with each step's four lines multiplied together before they meet f
  // (k_miller_acc4l: 12 Fp2 products per lane per round of four lines instead of 16, but the Karatsuba sums'
  // normalisations, selects and exchanges leave it 3 % fewer VALU instructions, 13 % waiting, 5.10 ms per launch
  // against 4.81: profiles/r06u_acc_ll_ab.txt)
  static const bool acc_ll = getenv("BLS_ACC_LL") && atoi(getenv("BLS_ACC_LL")) != 0;
  // below ACC8_MAX items one pair per f runs on eight lanes (k_miller_acc8: ~40 % fewer product rounds per step for
  // twice the waves): a latency win for the small batches whose chain decides (C5's 1,024: +2.4 %), a loss where
  // the SIMD time does (C3's 2,048: -8.6 %; profiles/r06y_acc8_ab.txt).  Knob BLS_ACC8_MAX.
  static const size_t acc8_max = getenv("BLS_ACC8_MAX") ? (size_t)atol(getenv("BLS_ACC8_MAX")) : ACC8_MAX;
  if (fused)
    PROF(5, launch_miller_fused(st, pP, H, pstat, NP, f, mg));
  else if (mg == 1 && NH < acc8_max)
    PROF(5, launch_miller_acc8(st, pP, H, pstat, NP, mlines, miller_lines_ld(NP), f));
  else if (mg == 4 && acc_ll)
    PROF(5, launch_miller_acc4l(st, pP, H, pstat, NP, mlines, miller_lines_ld(NP), f));
  else
    PROF(5, launch_miller_acc4(st, pP, H, pstat, NP, mlines, miller_lines_ld(NP), f, mg));
  PROF(6, launch_fp12_prod_vm(st, f, (NP + mg - 1) / mg, ft, fo));
  ctx->last_hashes = NH;
  ctx->last_pairs = NP;
  J.fav_B = B;
  J.fav_ready = true;
  *out_f = fo;
  return 0;
}

// Bisection fallback ("a failing batch falls back to
// per-signature bisection"), on the job's own stream with no host round trip.
// The leaves are the items' Miller values from the batch's own kernels:
//   f_H,i   = ML(r_i apk_i, H_i): the batch's per-item f (one pair per f below
//             ACC_SHARED_MIN items) or k_miller_fused<1> over the batch's
//             r_i apk_i and H_i again (shared-f batches);
//   f_sig,i = ML(-r_i G1, sigma_i): -r_i G1 from a fixed-base comb (8 mixed
//             additions, k_neg_rg1; its upper four windows hold phi images, so
//             r_i = a + b lambda as in the batch), f by k_miller_fused<1>;
// leaf_i = f_H,i f_sig,i, and a 16-ary product tree above the leaves.  A node's
// check is FE(node) == 1: the product of e(r_i apk_i, H_i) e(-r_i G1, sigma_i)
// over its items, the random linear combination of their checks.  The first
// checked level is the lowest with at most 64 nodes (all of them checked; the
// root first when the caller does not know it fails); every level below is one
// launch of k_fe_check_gated that checks exactly the nodes whose parent failed,
// reading the parent's result on the device.  A leaf that fails is an invalid
// item; every item under a passing node keeps its per-item status.  With k bad
// items among B this is ~64 + 16 k (log16(B) - 2) checks.  Items with status 0
// (rejected before the pairing) have leaf 1 and keep verdict 0.  root_bad: the
// caller already knows the product fails.
static int fav_bisect(bls_ctx* ctx, bool root_bad, uint8_t* d_out) {
  Job& J = *ctx->j;
  const size_t B = J.fav_B;
  const int* status = (const int*)J.buf[S_STATUS].p;
  const uint64_t* rsc0 = (const uint64_t*)J.buf[S_RSC].p;
  const G1A* rP = (const G1A*)J.buf[S_RP].p;
  const G2A* H = (const G2A*)J.buf[S_H].p;  // per item; per message for a shared-message batch (H_item below)
  const G2A* sig0 = (const G2A*)J.buf[S_SIG].p;
  Fp12* fb = (Fp12*)J.buf[S_FAV_F].p;
  std::vector<size_t> off{0}, cnt{B};
  while (cnt.back() > 1) {
    off.push_back(off.back() + cnt.back());
    cnt.push_back((cnt.back() + 15) / 16);
  }
  const int R = (int)cnt.size() - 1;
  int T = 0;  // first checked level below the root: the lowest with at most 64 nodes
  while (T < R && cnt[T] > 64) T++;
  const int top = root_bad ? T : R;  // highest level the tree must be built to
  const size_t total = off[top] + cnt[top];
  G1A* Ps;
  G1P* Pj;
  Fp12 *fS, *fH, *tree;
  int* res;
  uint32_t* nchk;
  G2A* sig;
  uint64_t* rsc;
  SCR(S_BP, B, Ps);
  SCR(S_BQ, B, Pj);
  SCR(S_BS, B, fS);
  SCR(S_BT, total, tree);
  SCR(S_BRES, total, res);
  SCR(S_BBAD, 1, nchk);
  SCR(S_BSIG, B, sig);
  SCR(S_BRSC, B, rsc);

  // per-item f_H: the batch's own f (one pair per f), else recomputed -- always for a shared-message batch, whose
  // pairs are per message: over the items' r_i apk_i and H_item[i] = H[msg_id[i]]
  const bool refH = J.fav_mg > 1 || J.fav_shared;
  G2A* Hit = nullptr;
  if (J.fav_shared) SCR(S_BHIT, B, Hit);
  if (refH) SCR(S_BSEL, B, fH);
  else fH = fb;
  hipStream_t st = J.stream;
  // first everything read of the state that the job's next batch writes from stream2 / stream3 (H and the line
  // records, sigma_i, r_i); that batch forks from ev_bis (fav_prepare) while the rest runs here
  if (J.fav_shared) {
    LK(launch_g2a_gather(st, B, H, (const uint32_t*)J.buf[S_MSGID].p, Hit));
    H = Hit;
  }
  if (refH) LK(launch_miller_fused(st, rP, H, status, B, fH, 1));
  HIPCK(hipMemcpyAsync(sig, sig0, B * sizeof(G2A), hipMemcpyDeviceToDevice, st));
  HIPCK(hipMemcpyAsync(rsc, rsc0, B * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
  HIPCK(hipEventRecord(J.ev_bis, st));
  J.bis_pending = true;
  LK(launch_neg_rg1(st, B, status, rsc, ctx->comb, Pj, Ps));
  LK(launch_miller_fused(st, Ps, sig, status, B, fS, 1));
  LK(launch_fp12_chunk_prod2(st, fH, fS, B, 1, tree));
  for (int L = 0; L < top; L++) LK(launch_fp12_chunk_prod(st, tree + off[L], cnt[L], 16, tree + off[L + 1]));
  HIPCK(hipMemsetAsync(nchk, 0, sizeof(uint32_t), st));
  // the gated levels on the one-wave k_fe_check (chip time: with ten jobs in flight, C5 578k vs 519k FAV/s on the
  // six-wave k_fe_wide, profiles/r05k_c5_bisect_fe_ab.txt) or, BLS_BISECT_FE=wide, on k_fe_wide (latency)
  static const bool wide_fe = getenv("BLS_BISECT_FE") && !strcmp(getenv("BLS_BISECT_FE"), "wide");
  auto gated = wide_fe ? launch_fe_wide_gated : launch_final_check_gated;
  uint64_t rounds = 0;
  const int* parent = nullptr;
  uint32_t pdiv = 1;
  if (!root_bad && T < R) {  // the root first; level T then runs only if it failed
    LK(gated(st, tree + off[R], 1, nullptr, 1, res + off[R], nchk));
    parent = res + off[R];
    pdiv = (uint32_t)cnt[T];
    rounds++;
  }
  for (int L = T; L >= 0; L--) {
    LK(gated(st, tree + off[L], cnt[L], parent, pdiv, res + off[L], nchk));
    parent = res + off[L];
    pdiv = 16;
    rounds++;
  }
  LK(launch_verdicts_res(st, status, res, B, d_out));
  J.bis_rounds = rounds;
  J.bis_dev_checks = nchk;  // read (after the stream) by bls_last_fallback_stats
  ctx->stats_job = &J;
  return 0;
}

static int fav_finish(bls_ctx* ctx, int batch_ok, bool root_bad, uint8_t* d_out) {
  if (!ctx->j->fav_ready) {
    ctx->err = "no prepared FAV batch";
    return BLS_E_ARG;
  }
  size_t B = ctx->j->fav_B;
  if (!B) return 0;  // an empty shard (job_submit with the device exchange): no verdicts
  int* status = (int*)ctx->j->buf[S_STATUS].p;
  if (batch_ok) {
    ctx->j->bis_checks = ctx->j->bis_rounds = 0;
    ctx->j->bis_dev_checks = nullptr;
    ctx->stats_job = ctx->j;
    PROF(8, launch_status_to_u8(ctx->j->stream, status, B, d_out));
    return 0;
  }
  return fav_bisect(ctx, root_bad, d_out);
}

// Entropy source of the RLC seeds; only bls_set_entropy_source (a test hook) changes it.
static char g_entropy_path[256] = "/dev/urandom";

int bls_set_entropy_source(const char* path) {
  if (!path || strlen(path) >= sizeof(g_entropy_path)) return BLS_E_ARG;
  strcpy(g_entropy_path, path);
  return 0;
}

// RLC scalars must be unpredictable to whoever produced the signatures (hard part 6): a short
// read fails the call closed (BLS_E_DEVICE) instead of continuing with a predictable seed.
int bls_host_seed(uint8_t* seed32) {
  if (!seed32) return BLS_E_ARG;
  FILE* f = fopen(g_entropy_path, "rb");
  size_t got = f ? fread(seed32, 1, 32, f) : 0;
  if (f) fclose(f);
  if (got != 32) {
    memset(seed32, 0, 32);
    return BLS_E_DEVICE;
  }
  return 0;
}

static int host_seed(bls_ctx* ctx, uint8_t seed[32]) {
  if (bls_host_seed(seed) != 0) {
    ctx->err = "could not read 32 bytes of entropy for the RLC seed";
    return BLS_E_DEVICE;
  }
  return 0;
}

// One host-buffer FAV batch: copies in, RLC batch check, bisection on failure.
// msg_id (nullable) / M: msgs32 is a table of M messages and item b signs entry msg_id[b] (fav_prepare)
// bits / bits_bytes (nullable): a committee-bitfield batch -- idx / offsets unused, bits_plan has run, and the
// bit bytes go up in the index list's place
static int fav_batch_host(bls_ctx* ctx, const uint32_t* idx, const uint64_t* offsets, size_t B, const uint8_t* msgs32,
                          const uint8_t* sigs96, uint8_t* out, size_t M = 0, const uint32_t* msg_id = nullptr,
                          const uint8_t* bits = nullptr, size_t bits_bytes = 0, int mode = 0) {
  if (msg_id) {  // before any device call
    if (!M) return BLS_E_ARG;
    for (size_t b = 0; b < B; b++)
      if (msg_id[b] >= M) return BLS_E_ARG;
  }
  const size_t nmsg = msg_id ? M : B;
  uint32_t* d_idx = nullptr;
  uint64_t* d_offs = nullptr;
  uint8_t *d_m, *d_s, *d_out, *d_bits = nullptr;
  if (bits) {
    SCR(S_IN0, bits_bytes, d_bits);
    CK(h2d(ctx, d_bits, bits, bits_bytes));
  } else {
    const uint64_t nidx = offsets[B];
    if (nidx && !idx) return BLS_E_ARG;
    if (nidx > 0xffffffffull * 64) return BLS_E_ARG;
    for (size_t b = 0; b < B; b++)
      if (offsets[b + 1] < offsets[b]) return BLS_E_ARG;
    SCR(S_IN0, nidx, d_idx);
    SCR(S_OFFS, B + 1, d_offs);
    CK(h2d(ctx, d_idx, idx, nidx * 4));
    CK(h2d(ctx, d_offs, offsets, (B + 1) * 8));
  }
  SCR(S_IN1, 32 * nmsg, d_m);
  SCR(S_IN2, 96 * B, d_s);
  SCR(S_IN3, B, d_out);
  CK(h2d(ctx, d_m, msgs32, 32 * nmsg));
  CK(h2d(ctx, d_s, sigs96, 96 * B));
  uint8_t seed[32];
  CK(host_seed(ctx, seed));
  // the inputs were just copied on stream1: the hash on stream2 forks after them, never from a bisection's ev_bis
  // (an earlier call's, recorded before these copies; the hash would read the previous contents of S_IN1)
  ctx->j->bis_pending = false;
  Fp12* f;
  const BitsArgs ba{d_bits, mode};
  CK(fav_prepare(ctx, d_idx, d_offs, B, d_m, d_s, seed, &f, M, msg_id, bits ? &ba : nullptr));
  int ok = run_final_check(ctx, f);
  if (ok < 0) return ok;
  CK(fav_finish(ctx, ok, true, d_out));
  CK(d2h(ctx, out, d_out, B));
  return 1;
}

int bls_fav_batch_indexed(bls_ctx* ctx, const uint32_t* idx, const uint64_t* offsets, size_t B, const uint8_t* msgs32,
                          const uint8_t* sigs96, uint8_t* out) {
  API_ENTER(ctx);
  if ((!offsets || !msgs32 || !sigs96 || !out) && B) return BLS_E_ARG;
  if (!B) return 1;
  return fav_batch_host(ctx, idx, offsets, B, msgs32, sigs96, out);
}

// Gossip firehose: B independent Verify calls with
// registry keys = B FastAggregateVerify calls of one key each, through the
// same RLC batch (one final exponentiation) and bisection path.
int bls_verify_batch_indexed(bls_ctx* ctx, const uint32_t* idx, size_t B, const uint8_t* msgs32, const uint8_t* sigs96,
                             uint8_t* out) {
  API_ENTER(ctx);
  if ((!idx || !msgs32 || !sigs96 || !out) && B) return BLS_E_ARG;
  if (!B) return 1;
  std::vector<uint64_t> offs(B + 1);
  for (size_t i = 0; i <= B; i++) offs[i] = i;
  return fav_batch_host(ctx, idx, offs.data(), B, msgs32, sigs96, out);
}

int bls_fav_batch_indexed_shared(bls_ctx* ctx, const uint32_t* idx, const uint64_t* offsets, size_t B,
                                 const uint8_t* msgs32, size_t M, const uint32_t* msg_id, const uint8_t* sigs96,
                                 uint8_t* out) {
  API_ENTER(ctx);
  if ((!offsets || !msgs32 || !msg_id || !sigs96 || !out) && B) return BLS_E_ARG;
  if (!B) return 1;
  return fav_batch_host(ctx, idx, offsets, B, msgs32, sigs96, out, M, msg_id);
}

int bls_verify_batch_indexed_shared(bls_ctx* ctx, const uint32_t* idx, size_t B, const uint8_t* msgs32, size_t M,
                                    const uint32_t* msg_id, const uint8_t* sigs96, uint8_t* out) {
  API_ENTER(ctx);
  if ((!idx || !msgs32 || !msg_id || !sigs96 || !out) && B) return BLS_E_ARG;
  if (!B) return 1;
  std::vector<uint64_t> offs(B + 1);
  for (size_t i = 0; i <= B; i++) offs[i] = i;
  return fav_batch_host(ctx, idx, offs.data(), B, msgs32, sigs96, out, M, msg_id);
}

int bls_fav_batch_committee_bits(bls_ctx* ctx, const uint32_t* comm_ids, const uint64_t* comm_offs,
                                 const uint8_t* bits, const uint64_t* bit_offs, size_t B, const uint8_t* msgs32,
                                 size_t M, const uint32_t* msg_id, const uint8_t* sigs96, int mode, uint8_t* out) {
  API_ENTER(ctx);
  if ((!comm_offs || !bit_offs || !msgs32 || !sigs96 || !out) && B) return BLS_E_ARG;
  if (!B) return 1;
  CK(bits_plan(ctx, comm_ids, comm_offs, bit_offs, B, mode));
  if (bit_offs[B] && !bits) return BLS_E_ARG;
  static const uint8_t none = 0;  // a batch whose items all have no member still takes the bits route
  return fav_batch_host(ctx, nullptr, nullptr, B, msgs32, sigs96, out, M, msg_id, bits ? bits : &none,
                        (size_t)bit_offs[B], mode);
}

// The item records say what the gather added: read back and summed here, so the batch itself pays nothing for it.
int bls_last_gather_work(bls_ctx* ctx, uint64_t* points_added, uint64_t* complement_items) {
  API_ENTER(ctx);
  uint64_t pts = 0, ncompl = 0;
  if (ctx->work_job && ctx->work_job->bits_B) {
    Job& J = *ctx->work_job;
    std::vector<BitsItem> it(J.bits_B);
    HIPCK(hipMemcpyAsync(it.data(), J.bits_items, J.bits_B * sizeof(BitsItem), hipMemcpyDeviceToHost, J.stream));
    HIPCK(hipStreamSynchronize(J.stream));
    for (size_t b = 0; b < J.bits_B; b++) {
      pts += it[b].len;
      if (it[b].flags & BITS_F_COMPLEMENT) {
        pts += J.bits_tab[b + 1] - J.bits_tab[b];  // its committees' sums
        ncompl++;
      }
    }
  }
  if (points_added) *points_added = pts;
  if (complement_items) *complement_items = ncompl;
  return 0;
}

int bls_last_batch_work(bls_ctx* ctx, uint64_t* hashes, uint64_t* miller_pairs) {
  API_ENTER(ctx);
  if (hashes) *hashes = ctx->last_hashes;
  if (miller_pairs) *miller_pairs = ctx->last_pairs;
  return 0;
}

int bls_aggregate_verify_batch(bls_ctx* ctx, const uint8_t* pks48, const uint8_t* msgs, const uint64_t* msg_offs,
                               const uint64_t* item_offs, size_t B, const uint8_t* sigs96, uint8_t* out) {
  API_ENTER(ctx);
  if ((B && (!item_offs || !sigs96 || !out)) || B > 0xffffffffu) return BLS_E_ARG;
  if (B == 0) return 1;
  if (item_offs[0] != 0) return BLS_E_ARG;
  for (size_t b = 0; b < B; b++)
    if (item_offs[b + 1] < item_offs[b]) return BLS_E_ARG;
  const size_t total = item_offs[B];
  if (total && (!pks48 || !msg_offs)) return BLS_E_ARG;
  if (total > 0xffffffffu) return BLS_E_ARG;
  if (total) {
    if (msg_offs[0] != 0) return BLS_E_ARG;
    for (size_t t = 0; t < total; t++)
      if (msg_offs[t + 1] < msg_offs[t] || msg_offs[t + 1] - msg_offs[t] > 0xffffffffu) return BLS_E_ARG;
    if (msg_offs[total] && !msgs) return BLS_E_ARG;
  }
  ctx->j->bis_checks = ctx->j->bis_rounds = 0;
  ctx->j->bis_dev_checks = nullptr;
  ctx->stats_job = ctx->j;
  hipStream_t st = ctx->j->stream;
  const size_t npair = total + B;
  // inputs
  uint8_t *d_pk, *d_sig, *d_msgs;
  uint64_t *d_moffs, *d_io, *d_rsc;
  uint32_t* d_pitem;
  SCR(S_IN0, 48 * total, d_pk);
  SCR(S_IN1, 96 * B, d_sig);
  SCR(S_IN2, total ? msg_offs[total] : 0, d_msgs);
  SCR(S_OFFS, total + 1, d_moffs);
  SCR(S_AV_IO, B + 1, d_io);
  SCR(S_AV_RSC, B, d_rsc);
  SCR(S_AV_PITEM, total, d_pitem);
  std::vector<uint32_t> pitem(total);
  for (size_t b = 0; b < B; b++)
    for (uint64_t t = item_offs[b]; t < item_offs[b + 1]; t++) pitem[t] = (uint32_t)b;
  std::vector<uint64_t> rsc(B);
  {
    uint8_t seed[32];
    CK(host_seed(ctx, seed));
    uint64_t x = 0, y = 0;
    memcpy(&x, seed, 8);
    memcpy(&y, seed + 8, 8);
    for (size_t b = 0; b < B; b++) {  // splitmix64 stream keyed by the OS seed; r_b != 0
      x += 0x9e3779b97f4a7c15ull;
      uint64_t z = x ^ y;
      z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
      z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
      z ^= z >> 31;
      rsc[b] = z ? z : 1;
    }
  }
  CK(h2d(ctx, d_pk, pks48, 48 * total));
  CK(h2d(ctx, d_sig, sigs96, 96 * B));
  if (total) {
    CK(h2d(ctx, d_msgs, msgs, msg_offs[total]));
    CK(h2d(ctx, d_moffs, msg_offs, (total + 1) * sizeof(uint64_t)));
  }
  CK(h2d(ctx, d_io, item_offs, (B + 1) * sizeof(uint64_t)));
  CK(h2d(ctx, d_rsc, rsc.data(), B * sizeof(uint64_t)));
  CK(h2d(ctx, d_pitem, pitem.data(), total * sizeof(uint32_t)));
  // per-key / per-signature validation, hash_to_G2 of every message
  G1A *d_pa, *P2;
  G2A *d_sa, *d_h, *Q2;
  int *d_pok, *d_sok, *d_status, *d_res;
  Fp12 *f, *ft, *fo, *fi;
  SCR(S_G1A, total, d_pa);
  SCR(S_OK, total, d_pok);
  SCR(S_AV_SIG, B, d_sa);
  SCR(S_AV_SOK, B, d_sok);
  SCR(S_AV_H, total, d_h);
  SCR(S_AV_ST, B, d_status);
  SCR(S_AV_P, npair, P2);
  SCR(S_AV_Q, npair, Q2);
  SCR(S_AV_F, npair, f);
  SCR(S_AV_FT, npair / 8 + 16, ft);
  SCR(S_FPART, 1, fo);
  LK(launch_key_validate(st, d_pk, total, d_pa, d_pok));
  LK(launch_sig_validate(st, d_sig, B, d_sa, d_sok));
  {  // hash_to_G2 of every message (as in the FAV batch)
    Fd* d_hf;
    int* d_flag;
    SCR(S_AV_HCF, h2c_scratch_fd(total), d_hf);
    SCR(S_AV_FLAG, total, d_flag);
    LK(launch_h2c_msgs(st, total, d_msgs, d_moffs, d_hf, d_h, d_flag));
    CK(h2c_fallback(ctx, st, total, d_msgs, d_moffs, d_flag, d_h));
  }
  LK(launch_av_items(st, B, d_io, d_pok, d_sok, d_sa, d_rsc, d_status, P2, Q2));
  LK(launch_av_pairs(st, total, d_pitem, d_status, d_rsc, d_pa, d_h, P2, Q2));
  if (npair >= 256) {  // per-pair Miller values (the fallback multiplies each item's segment): the fused kernel
                       // (G2 lines and f accumulation in one workgroup, bls_miller_pair.hip, G = 1)
    PROF(5, launch_miller_fused(st, P2, Q2, nullptr, npair, f, 1));
  } else {
    PROF(5, launch_miller_wave(st, P2, Q2, nullptr, npair, f));
  }
  PROF(6, launch_fp12_prod_vm(st, f, npair, ft, fo));
  std::vector<int> status(B);
  CK(d2h(ctx, status.data(), d_status, B * sizeof(int)));
  const int batch_ok = run_final_check(ctx, fo);
  if (batch_ok < 0) return batch_ok;
  if (!batch_ok) {  // each item on its own: its segment of Miller values, one final exponentiation each
    std::vector<uint32_t> sel;
    for (size_t b = 0; b < B; b++)
      if (status[b]) sel.push_back((uint32_t)b);
    uint32_t* d_sel;
    SCR(S_AV_SEL, sel.size(), d_sel);
    SCR(S_AV_FI, B, fi);
    SCR(S_AV_RES, sel.size(), d_res);
    LK(launch_fp12_seg_prod(st, f, d_io, B, fi));
    std::vector<int> res(sel.size());
    CK(run_final_checks_sel(ctx, fi, sel.data(), sel.size(), d_sel, d_res, res.data()));
    for (size_t k = 0; k < sel.size(); k++) status[sel[k]] = res[k];
    ctx->j->bis_checks = sel.size();
    ctx->j->bis_rounds = 1;
  }
  for (size_t b = 0; b < B; b++) out[b] = status[b] ? 1 : 0;
  return 1;
}

int bls_signing_roots(bls_ctx* ctx, const uint8_t* object_roots32, const uint8_t* domains32, size_t domain_stride,
                      size_t n, uint8_t* out32) {
  API_ENTER(ctx);
  if (n && (!object_roots32 || !domains32 || !out32)) return BLS_E_ARG;
  if (domain_stride != 0 && domain_stride != 32) return BLS_E_ARG;
  if (!n) return 1;
  uint8_t *d_l, *d_r, *d_o;
  const size_t nr = domain_stride ? n : 1;
  SCR(S_SZ_A, 32 * n, d_l);
  SCR(S_SZ_B, 32 * nr, d_r);
  SCR(S_SZ_C, 32 * n, d_o);
  CK(h2d(ctx, d_l, object_roots32, 32 * n));
  CK(h2d(ctx, d_r, domains32, 32 * nr));
  LK(launch_sha256_pairs(ctx->j->stream, d_l, d_r, domain_stride, n, d_o));
  CK(d2h(ctx, out32, d_o, 32 * n));
  return 1;
}

int bls_merkleize(bls_ctx* ctx, const uint8_t* chunks32, size_t n, int depth, uint8_t* root32) {
  API_ENTER(ctx);
  if ((n && !chunks32) || !root32 || depth < 0 || depth > 63) return BLS_E_ARG;
  if (n > (1ull << depth)) return BLS_E_ARG;
  uint8_t *d_a, *d_b, *d_z, *root;
  SCR(S_SZ_A, 32 * (n ? n : 1), d_a);
  SCR(S_SZ_B, 32 * ((n + 1) / 2 + 1), d_b);
  SCR(S_SZ_Z, 32, d_z);
  HIPCK(hipMemsetAsync(d_z, 0, 32, ctx->j->stream));
  if (n == 0) {  // root of an all-zero tree: the zero hash of this depth
    for (int l = 0; l < depth; l++) {
      uint8_t* r;
      LK(launch_merkleize(ctx->j->stream, d_z, d_a, 1, 1, d_z, &r));
      HIPCK(hipMemcpyAsync(d_z, r, 32, hipMemcpyDeviceToDevice, ctx->j->stream));
    }
    CK(d2h(ctx, root32, d_z, 32));
    return 1;
  }
  CK(h2d(ctx, d_a, chunks32, 32 * n));
  LK(launch_merkleize(ctx->j->stream, d_a, d_b, n, depth, d_z, &root));
  CK(d2h(ctx, root32, root, 32));
  return 1;
}

int bls_pairing_check(bls_ctx* ctx, const uint8_t* g1s48, const uint8_t* g2s96, size_t n) {
  API_ENTER(ctx);
  if (n && (!g1s48 || !g2s96)) return BLS_E_ARG;
  if (n == 0) return 1;  // empty product
  hipStream_t st = ctx->j->stream;
  uint8_t* d_in;
  G1A* P;
  G2A* Q;
  int *ok1, *ok2;
  Fp12 *f, *ft, *fo;
  SCR(S_KZ_IN, 144 * n, d_in);
  SCR(S_KZ_P, n, P);
  SCR(S_KZ_Q, n, Q);
  SCR(S_KZ_OK, n, ok1);
  SCR(S_KZ_OK2, n, ok2);
  SCR(S_KZ_F, n, f);
  SCR(S_KZ_FT, n / 8 + 16, ft);
  SCR(S_FPART, 1, fo);
  CK(h2d(ctx, d_in, g1s48, 48 * n));
  CK(h2d(ctx, d_in + 48 * n, g2s96, 96 * n));
  LK(launch_pairs_decode(st, d_in, n, true, P, Q, ok1, ok2));
  std::vector<int> a(n), b(n);
  CK(d2h(ctx, a.data(), ok1, n * sizeof(int)));
  CK(d2h(ctx, b.data(), ok2, n * sizeof(int)));
  for (size_t i = 0; i < n; i++)
    if (!a[i] || !b[i]) return 0;
  size_t nf = 0;
  LK(launch_miller_call(st, P, Q, n, f, &nf));  // identity pairs: an Fp2 factor, 1 after the final exponentiation
  LK(launch_fp12_prod_vm(st, f, nf, ft, fo));
  return run_final_check(ctx, fo, 1, true);
}

int bls_g1_multi_exp(bls_ctx* ctx, const uint8_t* g1s48, const uint8_t* scalars32, size_t n, uint8_t* out48) {
  API_ENTER(ctx);
  if ((n && (!g1s48 || !scalars32)) || !out48) return BLS_E_ARG;
  hipStream_t st = ctx->j->stream;
  uint8_t *d_in, *d_out;
  G1A *P, *S;
  int *ok, *live;
  G1J *tmp, *sum;
  SCR(S_KZ_IN, 80 * n, d_in);
  SCR(S_KZ_P, n, P);
  SCR(S_KZ_S, n, S);
  SCR(S_KZ_OK, n, ok);
  SCR(S_KZ_OK2, n, live);
  SCR(S_KZ_J, 1024, tmp);
  SCR(S_G1J, 1, sum);
  SCR(S_KZ_OUT, 48, d_out);
  if (n) {
    CK(h2d(ctx, d_in, g1s48, 48 * n));
    CK(h2d(ctx, d_in + 48 * n, scalars32, 32 * n));
    LK(launch_g1_decode_checked(st, d_in, n, P, ok));
    std::vector<int> a(n);
    CK(d2h(ctx, a.data(), ok, n * sizeof(int)));
    for (size_t i = 0; i < n; i++)
      if (!a[i]) return 0;
    LK(launch_g1_scale(st, P, d_in + 48 * n, n, S, live));
  }
  LK(launch_g1_sum_aff(st, S, live, n, tmp, sum));
  LK(launch_g1_compress(st, sum, d_out, nullptr));
  CK(d2h(ctx, out48, d_out, 48));
  return 1;
}

// ------------------------------------------------------- curve objects --
// (E/utils/bls.py:239-392: arkworks G1Point / G2Point / GT under fastest_bls)
static int pt_width(int group) { return group == 1 ? 48 : group == 2 ? 96 : 0; }

int bls_point_decode(bls_ctx* ctx, int group, const uint8_t* in, size_t n, int subgroup_check, uint8_t* out_ok) {
  API_ENTER(ctx);
  const int W = pt_width(group);
  if (!W || (n && !in)) return BLS_E_ARG;
  if (!n) return 1;
  uint8_t* d_in;
  void* d_a;
  int* d_ok;
  SCR(S_PT_IN, (size_t)W * n, d_in);
  SCR(S_PT_A, (group == 1 ? sizeof(G1A) : sizeof(G2A)) * n, *(uint8_t**)&d_a);
  SCR(S_PT_OK, n, d_ok);
  CK(h2d(ctx, d_in, in, (size_t)W * n));
  LK(launch_pt_decode(ctx->j->stream, group, d_in, n, subgroup_check ? 1 : 0, d_a, d_ok));
  std::vector<int> ok(n);
  CK(d2h(ctx, ok.data(), d_ok, n * sizeof(int)));
  int all = 1;
  for (size_t i = 0; i < n; i++) {
    if (out_ok) out_ok[i] = ok[i] ? 1 : 0;
    if (!ok[i]) all = 0;
  }
  return all;
}

static int pt_binop(bls_ctx* ctx, int group, const uint8_t* a, const uint8_t* b, const uint8_t* k32, int op,
                    uint8_t* out) {
  const int W = pt_width(group);
  uint8_t* d;
  int* d_ok;
  SCR(S_PT_IN, 2 * (size_t)W + 32 + W, d);
  SCR(S_PT_OK, 1, d_ok);
  CK(h2d(ctx, d, a, W));
  if (op == 0) CK(h2d(ctx, d + W, b, W));
  else CK(h2d(ctx, d + 2 * W, k32, 32));
  LK(launch_pt_binop(ctx->j->stream, group, d, d + W, d + 2 * W, op, d + 2 * W + 32, d_ok));
  int ok = 0;
  CK(d2h(ctx, &ok, d_ok, sizeof ok));
  if (!ok) return 0;
  CK(d2h(ctx, out, d + 2 * W + 32, W));
  return 1;
}

int bls_point_add(bls_ctx* ctx, int group, const uint8_t* a, const uint8_t* b, uint8_t* out) {
  API_ENTER(ctx);
  if (!pt_width(group) || !a || !b || !out) return BLS_E_ARG;
  return pt_binop(ctx, group, a, b, nullptr, 0, out);
}

int bls_point_mul(bls_ctx* ctx, int group, const uint8_t* p, const uint8_t* k32, uint8_t* out) {
  API_ENTER(ctx);
  if (!pt_width(group) || !p || !k32 || !out) return BLS_E_ARG;
  return pt_binop(ctx, group, p, nullptr, k32, 1, out);
}

// -P of a compressed point is the same encoding with the sign flag flipped
// (the identity and points with y = 0 -- none exist on E1 / E2 -- are their own
// negation).  Byte logic only; the encoding is validated on the device first.
int bls_point_neg(bls_ctx* ctx, int group, const uint8_t* p, uint8_t* out) {
  const int W = pt_width(group);
  if (!W || !p || !out) return BLS_E_ARG;
  uint8_t ok = 0;
  const int v = bls_point_decode(ctx, group, p, 1, 0, &ok);
  if (v != 1) return v;
  memcpy(out, p, W);
  if (!(p[0] & 0x40)) out[0] ^= 0x20;
  return 1;
}

int bls_multi_exp(bls_ctx* ctx, int group, const uint8_t* pts, const uint8_t* scalars32, size_t n, int subgroup_check,
                  uint8_t* out) {
  API_ENTER(ctx);
  const int W = pt_width(group);
  if (!W || (n && (!pts || !scalars32)) || !out) return BLS_E_ARG;
  if (!n) return 0;  // the reference raises on an empty input (E/utils/bls.py:270-271)
  hipStream_t st = ctx->j->stream;
  uint8_t *d_in, *d_a, *d_tmp, *d_out;
  int* d_ok;
  SCR(S_PT_IN, ((size_t)W + 32) * n, d_in);
  SCR(S_PT_A, (group == 1 ? sizeof(G1A) : sizeof(G2A)) * n, d_a);
  SCR(S_PT_OK, n, d_ok);
  SCR(S_PT_TMP, pt_msm_scratch_bytes(group, n), d_tmp);
  SCR(S_PT_OUT, W, d_out);
  CK(h2d(ctx, d_in, pts, (size_t)W * n));
  CK(h2d(ctx, d_in + (size_t)W * n, scalars32, 32 * n));
  LK(launch_pt_decode(st, group, d_in, n, subgroup_check ? 1 : 0, d_a, d_ok));
  std::vector<int> ok(n);
  CK(d2h(ctx, ok.data(), d_ok, n * sizeof(int)));
  for (size_t i = 0; i < n; i++)
    if (!ok[i]) return 0;
  LK(launch_pt_msm(st, group, d_a, d_in + (size_t)W * n, n, d_tmp, d_out));
  CK(d2h(ctx, out, d_out, W));
  return 1;
}

// prod_i e(P_i, Q_i) after the final exponentiation, as 576 bytes
int bls_multi_pairing(bls_ctx* ctx, const uint8_t* g1s48, const uint8_t* g2s96, size_t n, int subgroup_check,
                      uint8_t* out576) {
  API_ENTER(ctx);
  if ((n && (!g1s48 || !g2s96)) || !out576) return BLS_E_ARG;
  if (!n) {  // the empty product: GT one (c0.c0.c0 = 1 in the 576-byte layout)
    memset(out576, 0, 576);
    out576[47] = 1;
    return 1;
  }
  hipStream_t st = ctx->j->stream;
  uint8_t *d_in, *d_out;
  G1A* P;
  G2A* Q;
  int *ok1, *ok2;
  Fp12 *f, *ft, *fo;
  SCR(S_KZ_IN, 144 * n, d_in);
  SCR(S_KZ_P, n, P);
  SCR(S_KZ_Q, n, Q);
  SCR(S_KZ_OK, n, ok1);
  SCR(S_KZ_OK2, n, ok2);
  SCR(S_KZ_F, n, f);
  SCR(S_KZ_FT, n / 8 + 16, ft);
  SCR(S_FPART, 1, fo);
  SCR(S_PT_OUT, 576, d_out);
  CK(h2d(ctx, d_in, g1s48, 48 * n));
  CK(h2d(ctx, d_in + 48 * n, g2s96, 96 * n));
  LK(launch_pairs_decode(st, d_in, n, subgroup_check != 0, P, Q, ok1, ok2));
  std::vector<int> a(n), b(n);
  CK(d2h(ctx, a.data(), ok1, n * sizeof(int)));
  CK(d2h(ctx, b.data(), ok2, n * sizeof(int)));
  for (size_t i = 0; i < n; i++)
    if (!a[i] || !b[i]) return 0;
  size_t nf = 0;
  LK(launch_miller_call(st, P, Q, n, f, &nf));  // identity pairs: an Fp2 factor, 1 after the final exponentiation
  LK(launch_fp12_prod_vm(st, f, nf, ft, fo));
  LK(launch_gt_final_exp(st, fo, d_out));
  CK(d2h(ctx, out576, d_out, 576));
  return 1;
}

int bls_gt_mul(bls_ctx* ctx, const uint8_t* a576, const uint8_t* b576, uint8_t* out576) {
  API_ENTER(ctx);
  if (!a576 || !b576 || !out576) return BLS_E_ARG;
  uint8_t* d;
  SCR(S_PT_IN, 3 * 576, d);
  CK(h2d(ctx, d, a576, 576));
  CK(h2d(ctx, d + 576, b576, 576));
  LK(launch_gt_mul(ctx->j->stream, d, d + 576, d + 1152));
  CK(d2h(ctx, out576, d + 1152, 576));
  return 1;
}

// pairing_check with the subgroup checks optional (arkworks multi_pairing on
// already-decoded curve objects checks none)
int bls_pairing_check_ex(bls_ctx* ctx, const uint8_t* g1s48, const uint8_t* g2s96, size_t n, int subgroup_check) {
  API_ENTER(ctx);
  if (n && (!g1s48 || !g2s96)) return BLS_E_ARG;
  if (n == 0) return 1;  // empty product
  hipStream_t st = ctx->j->stream;
  uint8_t* d_in;
  G1A* P;
  G2A* Q;
  int *ok1, *ok2;
  Fp12 *f, *ft, *fo;
  SCR(S_KZ_IN, 144 * n, d_in);
  SCR(S_KZ_P, n, P);
  SCR(S_KZ_Q, n, Q);
  SCR(S_KZ_OK, n, ok1);
  SCR(S_KZ_OK2, n, ok2);
  SCR(S_KZ_F, n, f);
  SCR(S_KZ_FT, n / 8 + 16, ft);
  SCR(S_FPART, 1, fo);
  CK(h2d(ctx, d_in, g1s48, 48 * n));
  CK(h2d(ctx, d_in + 48 * n, g2s96, 96 * n));
  LK(launch_pairs_decode(st, d_in, n, subgroup_check != 0, P, Q, ok1, ok2));
  std::vector<int> a(n), b(n);
  CK(d2h(ctx, a.data(), ok1, n * sizeof(int)));
  CK(d2h(ctx, b.data(), ok2, n * sizeof(int)));
  for (size_t i = 0; i < n; i++)
    if (!a[i] || !b[i]) return 0;
  size_t nf = 0;
  LK(launch_miller_call(st, P, Q, n, f, &nf));
  LK(launch_fp12_prod_vm(st, f, nf, ft, fo));
  return run_final_check(ctx, fo, 1, true);
}

int bls_last_fallback_stats(bls_ctx* ctx, uint64_t* fe_checks, uint64_t* rounds) {
  API_ENTER(ctx);
  Job& J = *ctx->stats_job;
  if (J.bis_dev_checks) {
    uint32_t n = 0;
    HIPCK(hipMemcpyAsync(&n, J.bis_dev_checks, sizeof n, hipMemcpyDeviceToHost, J.stream));
    HIPCK(hipStreamSynchronize(J.stream));
    J.bis_checks = n;
    J.bis_dev_checks = nullptr;
  }
  if (fe_checks) *fe_checks = J.bis_checks;
  if (rounds) *rounds = J.bis_rounds;
  return 0;
}

// ------------------------------------------------------ device-resident --
void* bls_dev_alloc(bls_ctx* ctx, size_t bytes) {
  if (!ctx) return nullptr;
  std::lock_guard<std::mutex> lock_(ctx->mu);
  if (hipSetDevice(ctx->device) != hipSuccess) return nullptr;
  void* p = nullptr;
  if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) return nullptr;
  return p;
}

int bls_dev_free(bls_ctx* ctx, void* p) {
  API_ENTER(ctx);
  HIPCK(hipStreamSynchronize(ctx->j->stream));
  HIPCK(hipFree(p));
  return 0;
}

int bls_h2d(bls_ctx* ctx, void* dst, const void* src, size_t bytes) {
  API_ENTER(ctx);
  CK(h2d(ctx, dst, src, bytes));
  HIPCK(hipStreamSynchronize(ctx->j->stream));
  return 0;
}

// every job stream of the context (a job's bisection fallback writes its verdicts asynchronously)
static int sync_jobs(bls_ctx* ctx) {
  for (int k = 0; k < ctx->njobs; k++) HIPCK(hipStreamSynchronize(ctx->jobs[k].stream));
  return 0;
}

int bls_d2h(bls_ctx* ctx, void* dst, const void* src, size_t bytes) {
  API_ENTER(ctx);
  CK(sync_jobs(ctx));
  CK(d2h(ctx, dst, src, bytes));
  return 0;
}

int bls_sync(bls_ctx* ctx) {
  API_ENTER(ctx);
  CK(sync_jobs(ctx));
  return 0;
}

// ------------------------------------------- grouped signature aggregation --
// G Aggregate calls in one (include/blsmi355x.h): decode every signature once (k_sig_validate, or the unchecked
// k_pt_decode), fold the members of each group with the segmented G2 sum (bls_g2_segsum.h over seg_plan's runs, one
// launch per level), and turn the G sums into compressed bytes and ok (k_g2_seg_finish).  No per-item flag returns
// to the host: a failed decode travels with its group's partial.  Everything is enqueued on job 0's stream into the
// S_AGG_* slots, which no other call uses -- a FAV batch prepared on job 0 keeps its state, and its finish simply
// runs behind this call.  `plan` was made from the caller's ids before any device call; the uploads read the
// context's copy of it, which the next grouped call replaces only after waiting for this one's stream.
static int aggregate_grouped_dev(bls_ctx* ctx, SegPlan& plan, const uint8_t* d_sigs, size_t B, size_t G,
                                 const uint8_t* d_include, int subgroup_check, uint8_t* d_out96, uint8_t* d_ok) {
  hipStream_t st = ctx->j->stream;
  std::swap(ctx->agg_plan, plan);
  const SegPlan& sp = ctx->agg_plan;
  const size_t PB = g2_seg_partial_bytes();
  G2A* a;
  int* ok;
  SegRun* d_runs;
  uint32_t* d_items;
  uint8_t *pa, *pb, *gsum;
  SCR(S_AGG_A, B, a);
  SCR(S_AGG_OK, B, ok);
  SCR(S_AGG_RUN, sp.runs.size(), d_runs);
  SCR(S_AGG_IT, B, d_items);
  SCR(S_AGG_PA, PB * sp.max_tmp(), pa);
  SCR(S_AGG_PB, PB * (sp.levels() > 1 ? sp.level_tmp[1] : 0), pb);
  SCR(S_AGG_SUM, PB * G, gsum);
  CK(h2d(ctx, d_runs, sp.runs.data(), sp.runs.size() * sizeof(SegRun)));
  CK(h2d(ctx, d_items, sp.grp_items.data(), B * sizeof(uint32_t)));
  if (subgroup_check)
    LK(launch_sig_validate(st, d_sigs, B, a, ok));
  else
    LK(launch_pt_decode(st, 2, d_sigs, B, 0, a, ok));
  for (size_t l = 0; l < sp.levels(); ++l) {
    const uint32_t n = sp.level_off[l + 1] - sp.level_off[l];
    const G2SP* in = (const G2SP*)((l & 1) ? pa : pb);
    G2SP* out = (G2SP*)((l & 1) ? pb : pa);
    LK(launch_g2_seg_fold(st, (int)l, d_runs + sp.level_off[l], n, d_items, ok, d_include, a, in, out, (G2SP*)gsum));
  }
  LK(launch_g2_seg_finish(st, G, (const G2SP*)gsum, d_out96, d_ok));
  return 1;
}

int bls_aggregate_grouped(bls_ctx* ctx, const uint8_t* sigs96, size_t B, const uint32_t* group_id, size_t G,
                          const uint8_t* include, int subgroup_check, uint8_t* out96, uint8_t* out_ok) {
  API_ENTER(ctx);
  if ((B && (!sigs96 || !group_id)) || (G && (!out96 || !out_ok))) return BLS_E_ARG;
  SegPlan plan;
  if (!seg_plan(group_id, B, G, plan)) {
    ctx->err = "group_id out of range (or no groups)";
    return BLS_E_ARG;
  }
  if (!B) {
    if (G) {
      memset(out96, 0, 96 * G);
      memset(out_ok, 0, G);
    }
    return 1;
  }
  HIPCK(hipStreamSynchronize(ctx->j->stream));  // an earlier grouped call's uploads read the context's plan
  uint8_t *d_in, *d_inc = nullptr, *d_out;
  SCR(S_AGG_IN, 96 * B, d_in);
  SCR(S_AGG_OUT, 97 * G, d_out);
  CK(h2d(ctx, d_in, sigs96, 96 * B));
  if (include) {
    SCR(S_AGG_INC, B, d_inc);
    CK(h2d(ctx, d_inc, include, B));
  }
  const int r = aggregate_grouped_dev(ctx, plan, d_in, B, G, d_inc, subgroup_check, d_out, d_out + 96 * G);
  if (r < 0) return r;
  HIPCK(hipMemcpyAsync(out96, d_out, 96 * G, hipMemcpyDeviceToHost, ctx->j->stream));
  CK(d2h(ctx, out_ok, d_out + 96 * G, G));
  return 1;
}

int bls_aggregate_grouped_dev(bls_ctx* ctx, const uint8_t* d_sigs96, size_t B, const uint32_t* group_id, size_t G,
                              const uint8_t* d_include, int subgroup_check, uint8_t* d_out96, uint8_t* d_ok) {
  API_ENTER(ctx);
  if ((B && (!d_sigs96 || !group_id)) || (G && (!d_out96 || !d_ok))) return BLS_E_ARG;
  SegPlan plan;
  if (!seg_plan(group_id, B, G, plan)) {
    ctx->err = "group_id out of range (or no groups)";
    return BLS_E_ARG;
  }
  CK(sync_jobs(ctx));  // a failing job's bisection writes the verdicts that d_include may be
  if (!B) {
    if (G) {
      HIPCK(hipMemsetAsync(d_out96, 0, 96 * G, ctx->j->stream));
      HIPCK(hipMemsetAsync(d_ok, 0, G, ctx->j->stream));
    }
    return 1;
  }
  return aggregate_grouped_dev(ctx, plan, d_sigs96, B, G, d_include, subgroup_check, d_out96, d_ok);
}

// ---------------------------------------------- pipelined FAV batches --
static int nccl_fail(bls_ctx* c, ncclResult_t r, const char* where);  // multi-GPU exchange, below
static void comm_fail_abort(bls_ctx* ctx);
__global__ void k_fp12_set_one(Fp12* f) {
  if (threadIdx.x || blockIdx.x) return;
  *f = fp12_one();
}

// The device-side exchange of a submitted job (multi-GPU, a communicator on the context), enqueued at submit: the
// comm stream waits for the partial, all-gathers the world's 576-byte partials (the collectives of all jobs on one
// stream, in submission order -- every rank submits the same jobs in the same order, so the collectives match),
// and the job's stream multiplies them inside the final-exponentiation kernel and copies the 4-byte verdict to
// h_own[1] (ev_cv).  No host step between a job's product and its verdict.
static int enqueue_comm_check(bls_ctx* ctx) {
  Job& J = *ctx->j;
  const int W = ctx->comm_world;
  uint8_t* d_all;
  Fp12* fw;
  int* d_cv;
  SCR(S_COMM, 576 * (size_t)W, d_all);
  SCR(S_FCHK, W, fw);
  SCR(S_CV, 1, d_cv);
  HIPCK(hipStreamWaitEvent(ctx->comm_stream, J.ev_partial, 0));
  const ncclResult_t r = ncclAllGather(J.buf[S_BYTES].p, d_all, 576, ncclUint8, ctx->comm, ctx->comm_stream);
  if (r != ncclSuccess) return nccl_fail(ctx, r, "ncclAllGather");
  HIPCK(hipEventRecord(J.ev_comm, ctx->comm_stream));
  HIPCK(hipStreamWaitEvent(J.stream, J.ev_comm, 0));
  PROF(9, launch_fp12_from_bytes(J.stream, d_all, W, fw));
  PROF(7, launch_final_check_wave(J.stream, fw, W, d_cv));
  HIPCK(hipMemcpyAsync(J.h_own + 1, d_cv, sizeof(int), hipMemcpyDeviceToHost, J.stream));
  HIPCK(hipEventRecord(J.ev_cv, J.stream));
  J.comm_pending = true;
  return 0;
}

// exchange: the job API with a communicator on the context (bls_fav_job_submit_dev) -- the all-gather and the
// combined check go on the device here and the job's own check is left for a failing combined check (read_own);
// otherwise (one GPU, or the host-exchange API bls_fav_batch_partial_dev) the own check is enqueued right behind the
// product.  B == 0 (a rank whose shard is empty) is allowed only with the exchange: its partial is the identity, so
// the rank still joins every all-gather and its peers never wait for it.
static int job_submit(bls_ctx* ctx, const uint32_t* d_idx, const uint64_t* d_offsets, size_t B, const uint8_t* d_msgs32,
                      const uint8_t* d_sigs96, const uint8_t* seed32, bool exchange, size_t M = 0,
                      const uint32_t* msg_id = nullptr, const BitsArgs* bits = nullptr) {
  exchange = exchange && ctx->comm;
  if (!seed32 || (B && ((!d_offsets && !bits) || !d_msgs32 || !d_sigs96)) || (!B && !exchange)) return BLS_E_ARG;
  Job& J = *ctx->j;
  Fp12* f;
  if (B) {
    CK(fav_prepare(ctx, d_idx, d_offsets, B, d_msgs32, d_sigs96, seed32, &f, M, msg_id, bits));
  } else {
    SCR(S_FPART, 1, f);
    hipLaunchKernelGGL(k_fp12_set_one, dim3(1), dim3(64), 0, J.stream, f);
    LK(hipGetLastError());
    J.fav_B = 0;
    J.fav_ready = true;
    J.comm_pending = false;
  }
  uint8_t* d_b;
  SCR(S_BYTES, 576, d_b);
  LK(launch_fp12_to_bytes(J.stream, f, d_b));
  HIPCK(hipMemcpyAsync(J.h_partial, d_b, 576, hipMemcpyDeviceToHost, J.stream));
  HIPCK(hipEventRecord(J.ev_partial, J.stream));
  J.partial_pending = true;
  if (exchange) {
    CK(enqueue_comm_check(ctx));
    J.own_pending = false;
    J.own_state = B ? -2 : 1;  // -2: computed on demand (read_own); an empty shard passes
    return 1;
  }
  // this job's own check, right behind its product on its stream: a single-GPU caller reads it with
  // bls_fav_job_check_own (no host round trip of the partial), and a multi-GPU failure is localised by it
  int* d_own;
  SCR(S_OWN, 1, d_own);
  // knob BLS_FE_WIDE_MAX: the check of batches below that size on the six-wave k_fe_wide (0.65 ms against 1.13, six
  // waves against one): C3 -4.5 %, C5 unchanged (profiles/r06y_acc8_ab.txt), so off
  static const size_t fe_wide_max = getenv("BLS_FE_WIDE_MAX") ? (size_t)atol(getenv("BLS_FE_WIDE_MAX")) : 0;
  if (B < fe_wide_max)
    PROF(7, launch_fe_wide(J.stream, f, 1, d_own));
  else
    PROF(7, launch_final_check_wave(J.stream, f, 1, d_own));
  HIPCK(hipMemcpyAsync(J.h_own, d_own, sizeof(int), hipMemcpyDeviceToHost, J.stream));
  HIPCK(hipEventRecord(J.ev_own, J.stream));
  J.own_pending = true;
  J.own_state = -1;
  return 1;
}

// *state = the job's own verdict (1 / 0): waits for the check job_submit enqueued or, after a submit with the
// device exchange, runs it now (a failing combined check is the only reader).  Returns 0 or BLS_E_* (no verdict:
// no batch submitted on this job, or another batch prepared on the slot since).
static int read_own(bls_ctx* ctx, int* state) {
  Job& J = *ctx->j;
  if (J.own_state == -2) {
    int* d_own;
    SCR(S_OWN, 1, d_own);
    PROF(7, launch_final_check_wave(J.stream, (const Fp12*)J.buf[S_FPART].p, 1, d_own));
    HIPCK(hipMemcpyAsync(J.h_own, d_own, sizeof(int), hipMemcpyDeviceToHost, J.stream));
    HIPCK(hipEventRecord(J.ev_own, J.stream));
    J.own_pending = true;
  }
  if (J.own_pending) {
    HIPCK(hipEventSynchronize(J.ev_own));
    J.own_state = J.h_own[0] ? 1 : 0;
    J.own_pending = false;
  }
  if (J.own_state < 0) {
    ctx->err = "no submitted FAV batch on this job";
    return BLS_E_ARG;
  }
  *state = J.own_state;
  return 0;
}

static int job_check_own(bls_ctx* ctx) {
  int own = 0;
  CK(read_own(ctx, &own));
  ctx->j->partial_pending = false;  // the partial's host copy is not needed
  return own;
}

static int job_partial(bls_ctx* ctx, uint8_t* partial576) {
  Job& J = *ctx->j;
  if (!partial576) return BLS_E_ARG;
  if (!J.partial_pending) {
    ctx->err = "no submitted FAV batch on this job";
    return BLS_E_ARG;
  }
  HIPCK(hipEventSynchronize(J.ev_partial));
  memcpy(partial576, J.h_partial, 576);
  J.partial_pending = false;
  return 1;
}

static int job_check(bls_ctx* ctx, const uint8_t* partials576, size_t n) {
  if (!partials576 || !n) return BLS_E_ARG;
  uint8_t* d_b;
  Fp12* f;
  SCR(S_IN0, 576 * n, d_b);
  SCR(S_FCHK, n, f);
  CK(h2d(ctx, d_b, partials576, 576 * n));
  PROF(9, launch_fp12_from_bytes(ctx->j->stream, d_b, n, f));
  return run_final_check(ctx, f, (int)n);  // the n partials are multiplied inside the FE kernel
}

// Verdicts are written on the job's stream: a failing batch's bisection runs there without a host round trip, so
// the caller can check the next job meanwhile (bls_sync / bls_d2h wait for every job stream).
static int job_finish(bls_ctx* ctx, int batch_ok, uint8_t* d_out) {
  if (!d_out && ctx->j->fav_B) return BLS_E_ARG;
  bool root_bad = false;
  Job& J = *ctx->j;
  // a failed product of several shards (or of given partials): this job's own check decides.  Without a verdict
  // of its own (another batch was prepared on the slot since its submit) the bisection starts at the root, whose
  // check it runs first.
  if (!batch_ok && (J.own_pending || J.own_state != -1)) {
    int own = 0;
    CK(read_own(ctx, &own));
    if (own == 1) batch_ok = 1;  // its own product passes: the failure is elsewhere, every status stands
    else root_bad = true;        // its own product fails: bisect below the root
  }
  CK(fav_finish(ctx, batch_ok, root_bad, d_out));
  return 1;
}

int bls_fav_batch_partial_dev(bls_ctx* ctx, const uint32_t* d_idx, const uint64_t* d_offsets, size_t B,
                              const uint8_t* d_msgs32, const uint8_t* d_sigs96, const uint8_t* seed32,
                              uint8_t* partial576) {
  API_ENTER(ctx);
  if (!partial576) return BLS_E_ARG;
  const int r = job_submit(ctx, d_idx, d_offsets, B, d_msgs32, d_sigs96, seed32, false);
  if (r < 0) return r;
  return job_partial(ctx, partial576);
}

int bls_partials_check(bls_ctx* ctx, const uint8_t* partials576, size_t n) {
  API_ENTER(ctx);
  return job_check(ctx, partials576, n);
}

int bls_fav_batch_finish_dev(bls_ctx* ctx, int batch_ok, uint8_t* d_out) {
  API_ENTER(ctx);
  return job_finish(ctx, batch_ok, d_out);
}

int bls_fav_job_submit_dev(bls_ctx* ctx, int job, const uint32_t* d_idx, const uint64_t* d_offsets, size_t B,
                           const uint8_t* d_msgs32, const uint8_t* d_sigs96, const uint8_t* seed32) {
  JOB_ENTER(ctx, job);
  const int r = job_submit(ctx, d_idx, d_offsets, B, d_msgs32, d_sigs96, seed32, true);
  // with a communicator, a rank that fails here never enqueues the all-gather its peers are (or will be) in:
  // abort, so their collectives fail instead of hanging (comm_fail_abort)
  if (r < 0 && ctx->comm) comm_fail_abort(ctx);
  return r;
}

int bls_fav_job_submit_shared_dev(bls_ctx* ctx, int job, const uint32_t* d_idx, const uint64_t* d_offsets, size_t B,
                                  const uint8_t* d_msgs32, size_t M, const uint32_t* msg_id,
                                  const uint8_t* d_sigs96, const uint8_t* seed32) {
  JOB_ENTER(ctx, job);
  int r = BLS_E_ARG;
  if (!B || msg_id)  // an empty shard has no ids; fav_prepare refuses M == 0 and ids >= M before any device call
    r = job_submit(ctx, d_idx, d_offsets, B, d_msgs32, d_sigs96, seed32, true, M, B ? msg_id : nullptr);
  if (r < 0 && ctx->comm) comm_fail_abort(ctx);
  return r;
}

// msg_id == nullptr: one message per item; else the shared-message form over a table of M.  An empty shard
// (B == 0, the device exchange only) takes no table and no bits.
int bls_fav_job_submit_bits_dev(bls_ctx* ctx, int job, const uint32_t* comm_ids, const uint64_t* comm_offs,
                                const uint8_t* d_bits, const uint64_t* bit_offs, size_t B, const uint8_t* d_msgs32,
                                size_t M, const uint32_t* msg_id, const uint8_t* d_sigs96, int mode,
                                const uint8_t* seed32) {
  JOB_ENTER(ctx, job);
  int r = B ? bits_plan(ctx, comm_ids, comm_offs, bit_offs, B, mode) : 0;
  if (r == 0 && B && bit_offs[B] && !d_bits) r = BLS_E_ARG;
  if (r == 0) {
    const BitsArgs ba{d_bits, mode};
    r = job_submit(ctx, nullptr, nullptr, B, d_msgs32, d_sigs96, seed32, true, msg_id ? M : 0, B ? msg_id : nullptr,
                   B ? &ba : nullptr);
  }
  if (r < 0 && ctx->comm) comm_fail_abort(ctx);
  return r;
}

int bls_fav_job_partial(bls_ctx* ctx, int job, uint8_t* partial576) {
  JOB_ENTER(ctx, job);
  return job_partial(ctx, partial576);
}

int bls_fav_job_check(bls_ctx* ctx, int job, const uint8_t* partials576, size_t n) {
  JOB_ENTER(ctx, job);
  return job_check(ctx, partials576, n);
}

int bls_fav_job_check_own(bls_ctx* ctx, int job) {
  JOB_ENTER(ctx, job);
  return job_check_own(ctx);
}

int bls_fav_job_finish_dev(bls_ctx* ctx, int job, int batch_ok, uint8_t* d_out) {
  JOB_ENTER(ctx, job);
  return job_finish(ctx, batch_ok, d_out);
}

// ------------------------------------------- multi-GPU exchange (RCCL) --
// every rank reduces its shard to one 576-byte Fp12 Miller
// partial; ncclAllGather moves the world x 576 bytes over xGMI (the transfer
// is latency-bound, not bandwidth-bound), and every rank multiplies the
// partials inside its final-exponentiation kernel -- no broadcast.  Fp12
// multiplication is not an elementwise sum, so this is an all-gather, not an
// all-reduce.
static int nccl_fail(bls_ctx* c, ncclResult_t r, const char* where) {
  char b[256];
  snprintf(b, sizeof b, "%s: %s", where, ncclGetErrorString(r));
  c->err = b;
  return BLS_E_DEVICE;
}

int bls_comm_unique_id(uint8_t* out128) {
  if (!out128) return BLS_E_ARG;
  ncclUniqueId id;
  if (ncclGetUniqueId(&id) != ncclSuccess) return BLS_E_DEVICE;
  static_assert(sizeof(id) == 128, "ncclUniqueId is 128 bytes");
  memcpy(out128, &id, sizeof id);
  return 0;
}

int bls_comm_init(bls_ctx* ctx, const uint8_t* uid128, int rank, int world) {
  API_ENTER(ctx);
  if (!uid128 || world < 1 || rank < 0 || rank >= world) return BLS_E_ARG;
  if (ctx->comm) {
    (void)ncclCommDestroy(ctx->comm);
    ctx->comm = nullptr;
  }
  ncclUniqueId id;
  memcpy(&id, uid128, sizeof id);
  const ncclResult_t r = ncclCommInitRank(&ctx->comm, world, id, rank);
  if (r != ncclSuccess) {
    ctx->comm = nullptr;
    return nccl_fail(ctx, r, "ncclCommInitRank");
  }
  ctx->comm_rank = rank;
  ctx->comm_world = world;
  ctx->comm_abort_cause.clear();
  return 0;
}

int bls_comm_destroy(bls_ctx* ctx) {
  API_ENTER(ctx);
  if (ctx->comm) {
    HIPCK(hipStreamSynchronize(ctx->comm_stream));  // every all-gather enqueued by a submit has run
    const ncclResult_t r = ncclCommDestroy(ctx->comm);
    ctx->comm = nullptr;
    if (r != ncclSuccess) return nccl_fail(ctx, r, "ncclCommDestroy");
  }
  ctx->comm_rank = 0;
  ctx->comm_world = 1;
  return 0;
}

static int comm_abort_locked(bls_ctx* ctx) {
  if (ctx->comm) {
    (void)ncclCommAbort(ctx->comm);
    ctx->comm = nullptr;
  }
  ctx->comm_rank = 0;
  ctx->comm_world = 1;
  return 0;
}

int bls_comm_abort(bls_ctx* ctx) {
  API_ENTER(ctx);
  return comm_abort_locked(ctx);
}

// any error on the exchange path -- a local one included (this rank then skips an all-gather its peers are in)
// -- leaves the peers waiting in this or a later all-gather: abort so their collectives fail instead of hanging.
// The first failure's text stays in ctx->err and is repeated by every later call on this context.
static void comm_fail_abort(bls_ctx* ctx) {
  ctx->comm_abort_cause = ctx->err;
  comm_abort_locked(ctx);
  ctx->err = "RCCL communicator aborted: " + ctx->comm_abort_cause;
}

// The verdict of job `job`'s combined check: its partial all-gathered with every rank's and the product
// final-exponentiated, both enqueued by its submit (enqueue_comm_check), so this only waits for the 4-byte
// verdict: 1 / 0.  The host never sees the partials.  Every rank submits the same jobs in the same order.
static int job_check_comm(bls_ctx* ctx) {
  Job& J = *ctx->j;
  if (J.comm_pending) {  // enqueued by job_submit: only the verdict is left to read
    HIPCK(hipEventSynchronize(J.ev_cv));
    J.comm_pending = false;
    J.partial_pending = false;
    return J.h_own[1] ? 1 : 0;
  }
  if (!J.partial_pending || !J.buf[S_BYTES].p) {
    ctx->err = "no submitted FAV batch on this job";
    return BLS_E_ARG;
  }
  // a job submitted before the communicator existed: the exchange now (every rank must do the same)
  CK(enqueue_comm_check(ctx));
  return job_check_comm(ctx);
}

int bls_fav_job_check_comm(bls_ctx* ctx, int job) {
  JOB_ENTER(ctx, job);
  if (!ctx->comm) {
    ctx->err = ctx->comm_abort_cause.empty()
                   ? "bls_comm_init was not called"
                   : "the RCCL communicator was aborted after an earlier failure: " + ctx->comm_abort_cause;
    return BLS_E_ARG;
  }
  const int r = job_check_comm(ctx);
  if (r < 0) comm_fail_abort(ctx);
  return r;
}

}  // extern "C"
