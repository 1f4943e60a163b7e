// C ABI, the context: its lifecycle and its jobs', the knob table, the helpers the other pieces share
// (bls_capi_internal.h), the profiler and the device-resident buffers.
#include "bls_capi_internal.h"

static const char* const PROF_NAMES[] = {"fav_gather", "sig_decode", "fav_hash", "g2_sum",        "sig_pair", "miller",
                                         "fp12_prod",  "final_exp",  "fav_finish", "partials_prod", "sig_vm",
                                         "msm",        "miller_lines", "key_validate", "bits_expand"};
static_assert(sizeof(PROF_NAMES) / sizeof(PROF_NAMES[0]) == PROF_N, "one name per ProfId, in its order");

namespace capi {

static long env_long(const char* name, long dflt) { return getenv(name) ? atol(getenv(name)) : dflt; }
static bool env_is(const char* name, const char* value) { return getenv(name) && !strcmp(getenv(name), value); }

const Knobs& knobs() {
  static const Knobs table = [] {
    Knobs k;
    k.wide_h2c_max = (size_t)env_long("BLS_WIDE_H2C_MAX", 1024);      // tools/av_probe.py (bls_aggregate_verify)
    k.wide_miller_max = (size_t)env_long("BLS_WIDE_MILLER_MAX", 1100);  // tools/av_probe.py (launch_miller_call)
    k.miller_fused = env_is("BLS_MILLER_FUSED", "1");  // off: profiles/r05o_miller_fused_ab.txt (lines_stage)
    k.acc_g = (int)env_long("BLS_ACC_G", 4);           // 1 / 2 / 4 / 8: profiles/r06a_g4_ab.txt (acc_stage)
    k.acc_shared_min = (size_t)env_long("BLS_ACC_SHARED_MIN", 4096);  // items from which pairs share an f (acc_stage)
    k.acc_ll = env_long("BLS_ACC_LL", 0) != 0;                 // off: profiles/r06u_acc_ll_ab.txt (acc_stage)
    k.acc8_max = (size_t)env_long("BLS_ACC8_MAX", 2048);       // profiles/r06y_acc8_ab.txt (acc_stage)
    k.bisect_fe_wide = env_is("BLS_BISECT_FE", "wide");        // off: profiles/r05k_c5_bisect_fe_ab.txt (fav_bisect)
    k.fe_wide_max = (size_t)env_long("BLS_FE_WIDE_MAX", 0);    // off: profiles/r06y_acc8_ab.txt (job_submit)
    return k;
  }();
  return table;
}

int fail(bls_ctx* c, hipError_t e, const char* where) {
  char b[256];
  snprintf(b, sizeof b, "%s: %s", where, hipGetErrorString(e));
  c->err = b;
  return BLS_E_DEVICE;
}

int h2d(bls_ctx* ctx, void* d, const void* h, size_t n) {
  if (n) HIPCK(hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, ctx->j->stream));
  return 0;
}
int d2h(bls_ctx* ctx, void* h, const void* d, size_t n) {
  if (n) HIPCK(hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, ctx->j->stream));
  HIPCK(hipStreamSynchronize(ctx->j->stream));
  return 0;
}

int all_ok(bls_ctx* ctx, const int* d_ok, size_t n) {
  std::vector<int> ok(n);
  CK(d2h(ctx, ok.data(), d_ok, n * sizeof(int)));
  for (size_t i = 0; i < n; i++)
    if (!ok[i]) return 0;
  return 1;
}

// every job stream of the context (a job's bisection fallback writes its verdicts asynchronously)
int sync_jobs(bls_ctx* ctx) {
  for (int k = 0; k < ctx->njobs; k++) HIPCK(hipStreamSynchronize(ctx->jobs[k].stream));
  return 0;
}

// the Miller values of the per-call pairing APIs (AggregateVerify, pairing checks, multi-pairings): the wide kernel
// on ceil(n / 2) workgroups up to wide_miller_max pairs, the wave-program kernel beyond (AggregateVerify(512) 5.54 ->
// 4.17 ms, (1,024) 7.95 -> 7.31; at 8,192 pairs the wave programs' throughput wins); *nf = the number of f values
// written; knob BLS_WIDE_MILLER_MAX
// qz: Jacobian Z of every Q, which only the wide kernel takes: a call with qz beyond the bound is refused
// (the wave-program kernel would read Jacobian X, Y as affine coordinates)
hipError_t launch_miller_call(hipStream_t st, const G1A* P, const G2A* Q, size_t n, Fp12* f, size_t* nf,
                              const Fp2* qz) {
  if (n <= knobs().wide_miller_max) {
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
hipError_t launch_keys(hipStream_t st, const uint8_t* pks, size_t n, G1A* out, int* ok) {
  return n <= WIDE_KEYS_MAX ? launch_key_validate_wide(st, pks, n, out, ok) : launch_key_validate(st, pks, n, out, ok);
}

// a keys batch's table (bls_fav_batch_keys): the same two kernels and the same switch, writing RegKey records with
// the verdict in REG_VALID straight from the key bytes (bls_key_out.h); valid (nullable): the verdicts as bytes
hipError_t launch_key_table(hipStream_t st, const uint8_t* pks, size_t n, RegKey* rec, uint8_t* valid) {
  return n <= WIDE_KEYS_MAX ? launch_key_records_wide(st, pks, n, rec, valid)
                            : launch_key_records(st, pks, n, rec, valid);
}

// the pairing APIs' decodes of n (G1, G2) pairs at d_in (48 n bytes of G1, then 96 n of G2), identity accepted: with
// the subgroup checks on the wide kernels (latency; up to WIDE_KEYS_MAX pairs), unchecked or beyond on the lane kernels
hipError_t launch_pairs_decode(hipStream_t st, const uint8_t* d_in, size_t n, bool subgroup, G1A* P, G2A* Q,
                               int* ok1, int* ok2) {
  hipError_t e;
  if (subgroup && n <= WIDE_KEYS_MAX) {
    e = launch_g1_decode_checked_wide(st, d_in, n, P, ok1);
    return e != hipSuccess ? e : launch_sig_validate_wide(st, d_in + 48 * n, n, Q, ok2);
  }
  e = launch_pt_decode(st, 1, d_in, n, subgroup ? 1 : 0, P, ok1);
  return e != hipSuccess ? e : launch_pt_decode(st, 2, d_in + 48 * n, n, subgroup ? 1 : 0, Q, ok2);
}

// the -G1 comb (bls_bisect.hip), built on first use: the MSM pairs' -w_b G1 and the bisection's -r_i G1
int ensure_comb(bls_ctx* ctx, hipStream_t st) {
  if (ctx->comb) return 0;
  G1A* tab = nullptr;
  HIPCK(hipMalloc(&tab, neg_g1_comb_entries() * sizeof(G1A)));
  hipError_t e = launch_neg_g1_comb_table(st, tab);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {  // never keep a table whose build did not complete
    (void)hipFree(tab);
    return fail(ctx, e, "launch_neg_g1_comb_table");
  }
  ctx->comb = tab;
  return 0;
}

// Copy n compressed keys, validate them on the device; returns 1 if all valid.
int validate_pks(bls_ctx* ctx, const uint8_t* pks, size_t n, G1A** outA, int** outOk) {
  uint8_t* d_in;
  SCR(S_IN0, 48 * n, d_in);
  SCR(S_G1A, n + 1, *outA);
  SCR(S_OK, n + 1, *outOk);
  CK(h2d(ctx, d_in, pks, 48 * n));
  HIPCK(launch_keys(ctx->j->stream, d_in, n, *outA, *outOk));
  return all_ok(ctx, *outOk, n);
}

// The hand-off from the job's stream to the stream its final-exponentiation checks run on: the context's FE
// stream, or the job's own (BLS_FE_STREAM=job, the default: one hardware queue fewer)
static int fe_handoff(bls_ctx* ctx, hipStream_t* fe) {
  Job& J = *ctx->j;
  *fe = ctx->fe_stream ? ctx->fe_stream : J.stream;
  if (*fe != J.stream) {
    HIPCK(hipEventRecord(J.ev[EV_FE], J.stream));
    HIPCK(hipStreamWaitEvent(*fe, J.ev[EV_FE], 0));
  }
  return 0;
}

// Final-exponentiation check of the product of f[0 .. n) on the context's FE
// stream, after the current job's stream: 1 / 0.
int run_final_check(bls_ctx* ctx, const Fp12* f, int n, bool wide) {
  int* d_r;
  SCR(S_INT, 4, d_r);
  hipStream_t fe;
  CK(fe_handoff(ctx, &fe));
  // batch checks on the one-wave k_fe_check, which leaves the CU to the other jobs (profiles/r04m_fe_ab.txt: 1.92 M vs
  // 1.84 M FAV/s with every check six-wave); single calls (wide: the pairing checks) on the six-wave k_fe_wide
  if (wide)
    PROF2(P_FINAL_EXP, fe, launch_fe_wide(fe, f, n, d_r));
  else
    PROF2(P_FINAL_EXP, fe, launch_final_check_wave(fe, f, n, d_r));
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
  hipStream_t fe;
  CK(fe_handoff(ctx, &fe));
  HIPCK(hipMemcpyAsync(d_sel, sel, 4 * nsel, hipMemcpyHostToDevice, fe));
  PROF2(P_FAV_FINISH, fe, launch_final_check_sel(fe, f, d_sel, nsel, d_res));
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
    HIPCK(hipGetLastError());
  }
  HIPCK(hipEventRecord(J.ev[EV_H2C], st));
  HIPCK(hipStreamWaitEvent(ctx->fb_stream, J.ev[EV_H2C], 0));
  HIPCK(launch_h2c_fallback(ctx->fb_stream, B, msgs, offs, flag, H));
  HIPCK(hipEventRecord(J.ev[EV_FB], ctx->fb_stream));
  HIPCK(hipStreamWaitEvent(st, J.ev[EV_FB], 0));
  return 0;
}

static void prof_collect(bls_ctx* c) {
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

}  // namespace capi

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
  if (hipStreamCreateWithFlags(&J.stream, hipStreamNonBlocking) != hipSuccess) return false;
  for (hipEvent_t& e : J.ev)
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return false;
  return hipHostMalloc((void**)&J.h_own, 2 * sizeof(int), hipHostMallocDefault) == hipSuccess &&
         hipHostMalloc((void**)&J.h_partial, 576, hipHostMallocDefault) == hipSuccess;
}

static void job_destroy(Job& J) {
  hipStream_t ss[3] = {J.stream, J.stream2, J.stream3 == J.stream2 ? nullptr : J.stream3};
  for (hipStream_t s : ss)
    if (s) (void)hipStreamSynchronize(s);
  for (auto& b : J.buf)
    if (b.p) (void)hipFree(b.p);
  for (hipEvent_t e : J.ev)
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
  if (ctx->g1t) (void)hipFree(ctx->g1t);
  if (ctx->g1t_stat) (void)hipFree(ctx->g1t_stat);
  if (ctx->comb) (void)hipFree(ctx->comb);
  if (ctx->kzg_dom) (void)hipFree(ctx->kzg_dom);
  if (ctx->kzg_negtau) (void)hipFree(ctx->kzg_negtau);
  if (ctx->kzg_idx) (void)hipFree(ctx->kzg_idx);
  if (ctx->kzc_tab) (void)hipFree(ctx->kzc_tab);
  if (ctx->kzc_negtau64) (void)hipFree(ctx->kzc_negtau64);
  if (ctx->kzc_idx) (void)hipFree(ctx->kzc_idx);
  if (ctx->kp_idx) (void)hipFree(ctx->kp_idx);
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

int bls_profile_enable(bls_ctx* ctx, int on) {
  API_ENTER(ctx);
  HIPCK(hipStreamSynchronize(ctx->j->stream));
  prof_collect(ctx);
  ctx->prof_on = on != 0;
  memset(ctx->prof_ms, 0, sizeof ctx->prof_ms);
  memset(ctx->prof_cnt, 0, sizeof ctx->prof_cnt);
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

}  // extern "C"
