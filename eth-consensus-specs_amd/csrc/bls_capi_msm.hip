// C ABI, the resident G1 point table and its batched bucket MSM (kernels: bls_g1_table.hip).
#include "bls_capi_internal.h"

constexpr size_t G1T_MAX = (size_t)1 << 26;  // entries: a record number 32 cap + i fits 32 bits
constexpr int G1T_WINDOWS = 32;
constexpr size_t G1M_BMAX = 65536;           // vectors per call: 256 B bucket slots fit 24 bits
constexpr size_t G1VM_BMAX = 256;            // rows per bls_g1_msm call: 8,192 B bucket slots (2^21), five words each

// Decode n encodings into entries first .. first + n (records of all 32 windows, state bytes on both sides).
static int g1t_fill(bls_ctx* ctx, const uint8_t* pts48, size_t n, size_t first, int subgroup, uint8_t* out_ok) {
  hipStream_t st = ctx->j->stream;
  uint8_t *d_in, *d_verd;
  G1A *d_a, *d_aff;
  G1P* d_cur;
  int *d_ok, *d_live;
  SCR(S_G1T_IN, 48 * n, d_in);
  SCR(S_G1T_A, n, d_a);
  SCR(S_G1T_OK, n, d_ok);
  SCR(S_G1T_CUR, n, d_cur);
  SCR(S_G1T_LIVE, n, d_live);
  SCR(S_G1T_AFF, n, d_aff);
  SCR(S_G1T_VERD, n, d_verd);
  CK(h2d(ctx, d_in, pts48, 48 * n));
  HIPCK(launch_pt_decode(st, 1, d_in, n, subgroup ? 1 : 0, d_a, d_ok));
  HIPCK(launch_g1_table_fill(st, d_a, d_ok, n, ctx->g1t, ctx->g1t_cap, first, ctx->g1t_stat, d_cur, d_live, d_aff,
                             d_verd));
  ctx->g1t_stat_h.resize(first + n);
  CK(d2h(ctx, ctx->g1t_stat_h.data() + first, ctx->g1t_stat + first, n));
  if (out_ok) CK(d2h(ctx, out_ok, d_verd, n));
  return 0;
}

static int g1t_alloc(bls_ctx* ctx, size_t cap, RegKey** tab, uint8_t** stat) {
  HIPCK(hipMalloc(tab, cap * G1T_WINDOWS * sizeof(RegKey)));
  HIPCK(hipMalloc(stat, cap));
  return 0;
}

int capi::g1_var_msm_dev(bls_ctx* ctx, const G1A* pts, const int* ok, size_t n, size_t B, const uint8_t* k32,
                         G1A* aff, int* live, uint8_t* out48, const uint32_t** d_entries) {
  const G1MsmPlan p = g1_var_msm_plan(n, B);
  uint32_t* d_u32;
  RegKey* d_rec;
  G1P *d_pa, *d_pb, *d_u, *d_w, *d_res;
  int *d_plive, *d_wlive;
  SCR(S_GV_REC, n, d_rec);
  SCR(S_GV_PLIVE, n, d_plive);
  SCR(S_GV_U32, p.u32_words, d_u32);
  SCR(S_GV_PA, p.part[0], d_pa);
  SCR(S_GV_PB, p.part[1], d_pb);
  SCR(S_GV_U, 8 * G1T_WINDOWS * B, d_u);
  SCR(S_GV_W, G1T_WINDOWS * B, d_w);
  SCR(S_GV_WLIVE, G1T_WINDOWS * B, d_wlive);
  SCR(S_GV_RES, B, d_res);
  HIPCK(launch_g1_var_msm(ctx->j->stream, p, pts, ok, (uint32_t)n, (uint32_t)B, k32, d_rec, d_plive, d_u32, d_pa,
                          d_pb, d_u, d_w, d_wlive, d_res, live, aff, out48, d_entries));
  ctx->g1v_msm_calls++;
  return 0;
}

extern "C" {

int bls_g1_table_load(bls_ctx* ctx, const uint8_t* pts48, size_t n, int subgroup_check, uint8_t* out_ok) {
  API_ENTER(ctx);
  if ((!pts48 && n) || n > G1T_MAX) return BLS_E_ARG;
  HIPCK(hipDeviceSynchronize());  // an MSM in flight reads the old table
  if (ctx->g1t) HIPCK(hipFree(ctx->g1t));
  if (ctx->g1t_stat) HIPCK(hipFree(ctx->g1t_stat));
  ctx->g1t = nullptr;
  ctx->g1t_stat = nullptr;
  ctx->g1t_n = ctx->g1t_cap = 0;
  ctx->g1t_stat_h.clear();
  ctx->g1t_gen++;
  CK(g1t_alloc(ctx, n ? n : 1, &ctx->g1t, &ctx->g1t_stat));
  ctx->g1t_cap = n ? n : 1;
  ctx->g1t_checked = subgroup_check != 0;
  if (n) CK(g1t_fill(ctx, pts48, n, 0, subgroup_check, out_ok));
  ctx->g1t_n = n;
  return 1;
}

int bls_g1_table_append(bls_ctx* ctx, const uint8_t* pts48, size_t n, int subgroup_check, uint8_t* out_ok) {
  API_ENTER(ctx);
  if (!ctx->g1t) {
    ctx->err = "no G1 table loaded";
    return BLS_E_NOREG;
  }
  if ((!pts48 && n) || ctx->g1t_n + n > G1T_MAX) return BLS_E_ARG;
  if (!n) return 1;
  const size_t need = ctx->g1t_n + n;
  if (need > ctx->g1t_cap) {  // the records are window-major: a larger table moves every window's slab
    HIPCK(hipDeviceSynchronize());
    size_t cap = ctx->g1t_cap + ctx->g1t_cap / 4;
    if (cap < need) cap = need;
    RegKey* tab;
    uint8_t* stat;
    CK(g1t_alloc(ctx, cap, &tab, &stat));
    hipStream_t st = ctx->j->stream;
    if (ctx->g1t_n) {
      for (int w = 0; w < G1T_WINDOWS; ++w)
        HIPCK(hipMemcpyAsync(tab + (size_t)w * cap, ctx->g1t + (size_t)w * ctx->g1t_cap, ctx->g1t_n * sizeof(RegKey),
                             hipMemcpyDeviceToDevice, st));
      HIPCK(hipMemcpyAsync(stat, ctx->g1t_stat, ctx->g1t_n, hipMemcpyDeviceToDevice, st));
      HIPCK(hipStreamSynchronize(st));
    }
    HIPCK(hipFree(ctx->g1t));
    HIPCK(hipFree(ctx->g1t_stat));
    ctx->g1t = tab;
    ctx->g1t_stat = stat;
    ctx->g1t_cap = cap;
  }
  ctx->g1t_checked = ctx->g1t_checked && subgroup_check != 0;
  CK(g1t_fill(ctx, pts48, n, ctx->g1t_n, subgroup_check, out_ok));
  ctx->g1t_n = need;
  return 1;
}

size_t bls_g1_table_size(bls_ctx* ctx) { return ctx ? ctx->g1t_n : 0; }

uint64_t bls_g1_table_generation(bls_ctx* ctx) { return ctx ? ctx->g1t_gen : 0; }

int bls_g1_table_msm(bls_ctx* ctx, const uint32_t* idx, size_t n, const uint8_t* scalars32, size_t B,
                     uint8_t* out48) {
  API_ENTER(ctx);
  if (!idx || !scalars32 || !out48 || !n || !B || B > G1M_BMAX) return BLS_E_ARG;
  if (n >= ((size_t)1 << 31) || B * n * G1T_WINDOWS >= ((size_t)1 << 31)) return BLS_E_ARG;
  if (!ctx->g1t) {
    ctx->err = "no G1 table loaded";
    return BLS_E_NOREG;
  }
  for (size_t i = 0; i < n; ++i)
    if (idx[i] >= ctx->g1t_n) return BLS_E_ARG;
  for (size_t i = 0; i < n; ++i)
    if (!ctx->g1t_stat_h[idx[i]]) return 0;  // an invalid encoding at load: the reference raises
  hipStream_t st = ctx->j->stream;
  const G1MsmPlan p = g1_msm_plan(n, B);
  uint8_t *d_in, *d_out;
  uint32_t* d_u32;
  G1P *d_pa, *d_pb, *d_u, *d_res;
  G1A* d_aff;
  int* d_live;
  const size_t kbytes = 32 * n * B;  // the scalars first: the sort reads them 16 bytes at a time
  SCR(S_G1M_IN, kbytes + 4 * n, d_in);
  SCR(S_G1M_U32, p.u32_words, d_u32);
  SCR(S_G1M_PA, p.part[0], d_pa);
  SCR(S_G1M_PB, p.part[1], d_pb);
  SCR(S_G1M_U, 8 * B, d_u);
  SCR(S_G1M_RES, B, d_res);
  SCR(S_G1M_LIVE, B, d_live);
  SCR(S_G1M_AFF, B, d_aff);
  SCR(S_G1M_OUT, 48 * B, d_out);
  CK(h2d(ctx, d_in, scalars32, kbytes));
  CK(h2d(ctx, d_in + kbytes, idx, 4 * n));
  const uint32_t* d_entries = nullptr;
  HIPCK(launch_g1_table_msm(st, p, ctx->g1t, (uint32_t)ctx->g1t_cap, ctx->g1t_stat,
                            reinterpret_cast<const uint32_t*>(d_in + kbytes), (uint32_t)n, (uint32_t)B, d_in, d_u32,
                            d_pa, d_pb, d_u, d_res, d_live, d_aff, d_out, &d_entries));
  uint32_t entries = 0;
  HIPCK(hipMemcpyAsync(&entries, d_entries, sizeof entries, hipMemcpyDeviceToHost, st));
  CK(d2h(ctx, out48, d_out, 48 * B));
  ctx->g1t_msm_calls++;
  ctx->g1t_msm_entries += entries;
  return 1;
}

int bls_g1_msm(bls_ctx* ctx, const uint8_t* pts48, size_t n, const uint8_t* scalars32, size_t B, int subgroup_check,
               uint8_t* out48) {
  API_ENTER(ctx);
  if ((n && (!pts48 || !scalars32)) || !out48 || !B || B > G1VM_BMAX) return BLS_E_ARG;
  if (n >= ((size_t)1 << 31) || B * n * G1T_WINDOWS >= ((size_t)1 << 31)) return BLS_E_ARG;
  if (!n) return 0;  // the reference raises on an empty input, as bls_multi_exp
  hipStream_t st = ctx->j->stream;
  uint8_t *d_in, *d_out;
  G1A *d_a, *d_aff;
  int *d_ok, *d_live;
  const size_t kbytes = 32 * n * B;  // the scalars first: the sort reads them 16 bytes at a time
  SCR(S_GV_IN, kbytes + 48 * n, d_in);
  SCR(S_GV_A, n, d_a);
  SCR(S_GV_OK, n, d_ok);
  SCR(S_GV_LIVE, B, d_live);
  SCR(S_GV_AFF, B, d_aff);
  SCR(S_GV_OUT, 48 * B, d_out);
  CK(h2d(ctx, d_in, scalars32, kbytes));
  CK(h2d(ctx, d_in + kbytes, pts48, 48 * n));
  HIPCK(launch_pt_decode(st, 1, d_in + kbytes, n, subgroup_check ? 1 : 0, d_a, d_ok));
  const int v = all_ok(ctx, d_ok, n);
  if (v <= 0) return v;
  const uint32_t* d_entries = nullptr;
  CK(g1_var_msm_dev(ctx, d_a, d_ok, n, B, d_in, d_aff, d_live, d_out, &d_entries));
  uint32_t entries = 0;
  HIPCK(hipMemcpyAsync(&entries, d_entries, sizeof entries, hipMemcpyDeviceToHost, st));
  CK(d2h(ctx, out48, d_out, 48 * B));
  ctx->g1v_msm_entries += entries;
  return 1;
}

int bls_g1_msm_stats(bls_ctx* ctx, uint64_t* calls, uint64_t* bucket_entries) {
  if (!ctx) return BLS_E_ARG;
  std::lock_guard<std::mutex> lock_(ctx->mu);
  if (calls) *calls = ctx->g1v_msm_calls;
  if (bucket_entries) *bucket_entries = ctx->g1v_msm_entries;
  return 0;
}

int bls_g1_table_stats(bls_ctx* ctx, uint64_t* msm_calls, uint64_t* bucket_entries) {
  if (!ctx) return BLS_E_ARG;
  std::lock_guard<std::mutex> lock_(ctx->mu);
  if (msm_calls) *msm_calls = ctx->g1t_msm_calls;
  if (bucket_entries) *bucket_entries = ctx->g1t_msm_entries;
  return 0;
}

}  // extern "C"
