// C ABI, the Deneb blob KZG functions (kernels: bls_kzg.hip; field and lane pieces: bls_fr.h, bls_kzg_blob.h).
// Everything runs on job 0's stream in the S_KB_* slots; the commitments' and proofs' MSM is the resident G1 table's
// (bls_g1_table.hip) on scalar rows that never leave the device.
#include "bls_capi_internal.h"
#include "bls_fr.h"

constexpr size_t KZG_N = 4096;        // FIELD_ELEMENTS_PER_BLOB
constexpr size_t KZG_BLOB = 32 * KZG_N;
constexpr size_t KZG_MSM_BMAX = 511;  // 32 B 4096 < 2^31 (bls_g1_table_msm's bound)
constexpr size_t KZG_BLOBS_MAX = 1024;
constexpr size_t KZG_ITEMS_MAX = 65536;

static int kzg_ensure_dom(bls_ctx* ctx) {
  if (ctx->kzg_dom) return 0;
  Fr* dom = nullptr;
  HIPCK(hipMalloc(&dom, kzg_domain_bytes()));
  hipError_t e = launch_fr_domain(ctx->j->stream, dom);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->j->stream);
  if (e != hipSuccess) {  // never keep a table whose build did not complete
    (void)hipFree(dom);
    return fail(ctx, e, "launch_fr_domain");
  }
  ctx->kzg_dom = dom;
  return 0;
}

static int kzg_need_setup(bls_ctx* ctx, bool lagrange) {
  if (!ctx->kzg_set || (lagrange && !ctx->kzg_n)) {
    ctx->err = lagrange ? "no KZG setup with Lagrange points" : "no KZG setup";
    return BLS_E_NOREG;
  }
  if (lagrange && (!ctx->g1t || ctx->kzg_gen != ctx->g1t_gen)) {
    ctx->err = "the G1 table was replaced after bls_kzg_setup";
    return BLS_E_ARG;
  }
  return 0;
}

// B blobs and their B evaluation points on the device: elements, verdicts, y_b = p_b(z_b).  Nothing is waited for.
struct KzgBlobs {
  uint8_t *blob, *y32;
  Fr *f, *z, *y, *pre;
  int *ok, *zok, *hit;
};
static int kzg_stage_blobs(bls_ctx* ctx, const uint8_t* blobs, size_t B, const uint8_t* z32, KzgBlobs& k) {
  hipStream_t st = ctx->j->stream;
  uint8_t* d_z32;
  CK(kzg_ensure_dom(ctx));
  SCR(S_KB_BLOB, KZG_BLOB * B, k.blob);
  SCR(S_KB_F, KZG_N * B, k.f);
  SCR(S_KB_PRE, KZG_N * B, k.pre);
  SCR(S_KB_OK, B, k.ok);
  SCR(S_KB_Z32, 32 * B, d_z32);
  SCR(S_KB_Y32, 32 * B, k.y32);
  SCR(S_KB_ZF, B, k.z);
  SCR(S_KB_YF, B, k.y);
  SCR(S_KB_ZOK, B, k.zok);
  SCR(S_KB_HIT, B, k.hit);
  CK(h2d(ctx, k.blob, blobs, KZG_BLOB * B));
  HIPCK(launch_blob_decode(st, k.blob, B, k.f, k.ok));
  if (z32) {
    CK(h2d(ctx, d_z32, z32, 32 * B));
    HIPCK(launch_fr_decode(st, d_z32, B, k.z, k.zok));
    HIPCK(launch_blob_eval(st, ctx->kzg_dom, k.f, k.z, k.ok, B, k.pre, k.y, k.y32, k.hit));
  }
  return 0;
}

// out48[b] = sum_i [rows[b][i]] L[i] over the setup's Lagrange entries; rows: B x 4,096 32-byte scalars on the device
static int kzg_msm(bls_ctx* ctx, const uint8_t* d_rows, size_t B, uint8_t* out48) {
  hipStream_t st = ctx->j->stream;
  const G1MsmPlan p = g1_msm_plan(KZG_N, B);
  uint8_t* d_out;
  uint32_t* d_u32;
  G1P *d_pa, *d_pb, *d_u, *d_res;
  G1A* d_aff;
  int* d_live;
  SCR(S_G1M_U32, p.u32_words, d_u32);
  SCR(S_G1M_PA, p.part[0], d_pa);
  SCR(S_G1M_PB, p.part[1], d_pb);
  SCR(S_G1M_U, 8 * B, d_u);
  SCR(S_G1M_RES, B, d_res);
  SCR(S_G1M_LIVE, B, d_live);
  SCR(S_G1M_AFF, B, d_aff);
  SCR(S_G1M_OUT, 48 * B, d_out);
  const uint32_t* d_entries = nullptr;
  HIPCK(launch_g1_table_msm(st, p, ctx->g1t, (uint32_t)ctx->g1t_cap, ctx->g1t_stat, ctx->kzg_idx, (uint32_t)KZG_N,
                            (uint32_t)B, d_rows, d_u32, d_pa, d_pb, d_u, d_res, d_live, d_aff, d_out, &d_entries));
  uint32_t entries = 0;
  HIPCK(hipMemcpyAsync(&entries, d_entries, sizeof entries, hipMemcpyDeviceToHost, st));
  CK(d2h(ctx, out48, d_out, 48 * B));
  ctx->g1t_msm_calls++;
  ctx->g1t_msm_entries += entries;
  return 1;
}

// The batch check of n items whose encodings (n commitments, then n proofs), z and y are on the device; the nullable
// verdict arrays (z < r, y < r, blob elements < r) join the decode's.  1 / 0 / BLS_E_*; out_item as bls_kzg_verify_batch.
static int kzg_verify_dev(bls_ctx* ctx, size_t n, const uint8_t* d_enc, const Fr* z, const Fr* y, const int* zok,
                          const int* yok, const int* bok, uint8_t* out_item) {
  hipStream_t st = ctx->j->stream;
  const size_t np = 3 * n + 1;
  G1A *P, *S, *PP;
  G2A* PQ;
  G1J *tmp, *sums;
  int *pok, *live, *d_res;
  uint8_t *K, *d_seed;
  uint32_t* d_sel;
  Fp12* fv;
  SCR(S_KB_P, np, P);
  SCR(S_KB_POK, 2 * n, pok);
  SCR(S_KB_K, 32 * np, K);
  SCR(S_KB_S, np, S);
  SCR(S_KB_LIVE, np, live);
  SCR(S_KB_J, 1100, tmp);
  SCR(S_KB_SUM, 2, sums);
  SCR(S_KB_SEED, 32, d_seed);
  SCR(S_KB_PP, 2 * n, PP);
  SCR(S_KB_PQ, 2 * n, PQ);
  SCR(S_KB_FV, n + 1, fv);
  SCR(S_KB_SEL, n, d_sel);
  SCR(S_KB_RES, n, d_res);
  HIPCK(launch_g1_decode_checked(st, d_enc, 2 * n, P, pok));
  std::vector<int> v(5 * n, 1);
  HIPCK(hipMemcpyAsync(v.data(), pok, 2 * n * sizeof(int), hipMemcpyDeviceToHost, st));
  if (zok) HIPCK(hipMemcpyAsync(v.data() + 2 * n, zok, n * sizeof(int), hipMemcpyDeviceToHost, st));
  if (yok) HIPCK(hipMemcpyAsync(v.data() + 3 * n, yok, n * sizeof(int), hipMemcpyDeviceToHost, st));
  if (bok) HIPCK(hipMemcpyAsync(v.data() + 4 * n, bok, n * sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCK(hipStreamSynchronize(st));
  bool good = true;
  for (size_t i = 0; i < n; ++i) {
    const bool g = v[i] && v[n + i] && v[2 * n + i] && v[3 * n + i] && v[4 * n + i];
    if (out_item) out_item[i] = g ? 1 : 0;
    good = good && g;
  }
  if (!good) return 0;
  uint8_t seed[32];
  CK(host_seed(ctx, seed));
  CK(h2d(ctx, d_seed, seed, 32));
  HIPCK(hipStreamSynchronize(st));  // the seed leaves this frame
  HIPCK(launch_kzg_rlc(st, d_seed, n, z, y, P, K));
  HIPCK(launch_g1_scale(st, P, K, np, S, live));
  HIPCK(launch_g1_sum_aff(st, S, live, 2 * n + 1, tmp, sums));
  HIPCK(launch_g1_sum_aff(st, S + 2 * n + 1, live + 2 * n + 1, n, tmp, sums + 1));
  HIPCK(launch_kzg_pairs(st, sums, ctx->kzg_negtau, PP, PQ));
  size_t nf = 0;
  HIPCK(launch_miller_call(st, PP, PQ, 2, fv, &nf, nullptr));
  const int r = run_final_check(ctx, fv, (int)nf, true);
  if (r != 0 || !out_item) return r;  // passed (out_item is all ones), failed without verdicts wanted, or an error
  // each item's own check: 2 n pairs on the two-pair kernel, whose workgroup i multiplies item i's two values
  if (miller_wide_nf(2) != 1) return BLS_E_DEVICE;
  HIPCK(launch_kzg_item_pairs(st, n, P, z, y, ctx->kzg_negtau, PP, PQ));
  HIPCK(launch_miller_wide_n(st, PP, PQ, nullptr, 2 * n, fv));
  std::vector<uint32_t> sel(n);
  for (size_t i = 0; i < n; ++i) sel[i] = (uint32_t)i;
  std::vector<int> res(n, 0);
  CK(run_final_checks_sel(ctx, fv, sel.data(), n, d_sel, d_res, res.data()));
  for (size_t i = 0; i < n; ++i) out_item[i] = res[i] ? 1 : 0;
  return 0;
}

extern "C" {

int bls_kzg_setup(bls_ctx* ctx, const uint8_t* g2_tau96, uint32_t lagrange_first, uint32_t lagrange_n) {
  API_ENTER(ctx);
  if (!g2_tau96 || (lagrange_n != 0 && lagrange_n != KZG_N)) return BLS_E_ARG;
  hipStream_t st = ctx->j->stream;
  ctx->kzg_set = false;
  ctx->kzg_n = 0;
  if (lagrange_n) {
    if (!ctx->g1t) {
      ctx->err = "no G1 table loaded";
      return BLS_E_NOREG;
    }
    if ((size_t)lagrange_first + KZG_N > ctx->g1t_n) return BLS_E_ARG;
    for (size_t i = 0; i < KZG_N; ++i)
      if (!ctx->g1t_stat_h[lagrange_first + i]) return 0;  // an invalid setup point
  }
  CK(kzg_ensure_dom(ctx));
  if (!ctx->kzg_negtau) HIPCK(hipMalloc(&ctx->kzg_negtau, sizeof(G2A)));
  if (!ctx->kzg_idx) HIPCK(hipMalloc(&ctx->kzg_idx, KZG_N * sizeof(uint32_t)));
  uint8_t* d_in;
  int* d_ok;
  SCR(S_KB_ENC, 96, d_in);
  SCR(S_KB_POK, 1, d_ok);
  CK(h2d(ctx, d_in, g2_tau96, 96));
  HIPCK(launch_pt_decode(st, 2, d_in, 1, 1, ctx->kzg_negtau, d_ok));
  HIPCK(launch_kzg_g2_neg(st, ctx->kzg_negtau));
  std::vector<uint32_t> idx(KZG_N);
  for (size_t i = 0; i < KZG_N; ++i) idx[i] = lagrange_first + (uint32_t)i;
  CK(h2d(ctx, ctx->kzg_idx, idx.data(), KZG_N * sizeof(uint32_t)));
  const int v = all_ok(ctx, d_ok, 1);  // waits for the stream: idx may go
  if (v <= 0) return v;
  ctx->kzg_first = lagrange_first;
  ctx->kzg_n = lagrange_n;
  ctx->kzg_gen = ctx->g1t_gen;
  ctx->kzg_set = true;
  return 1;
}

int bls_kzg_eval_blobs(bls_ctx* ctx, const uint8_t* blobs, size_t B, const uint8_t* z32, uint8_t* y32,
                       uint8_t* out_ok) {
  API_ENTER(ctx);
  if (B > KZG_BLOBS_MAX || (B && (!blobs || !z32 || !y32))) return BLS_E_ARG;
  if (!B) return 1;
  KzgBlobs k;
  CK(kzg_stage_blobs(ctx, blobs, B, z32, k));
  std::vector<int> ok(2 * B);
  HIPCK(hipMemcpyAsync(ok.data(), k.ok, B * sizeof(int), hipMemcpyDeviceToHost, ctx->j->stream));
  HIPCK(hipMemcpyAsync(ok.data() + B, k.zok, B * sizeof(int), hipMemcpyDeviceToHost, ctx->j->stream));
  CK(d2h(ctx, y32, k.y32, 32 * B));
  int all = 1;
  for (size_t b = 0; b < B; ++b) {
    if (!ok[B + b]) return 0;  // z >= r
    if (out_ok) out_ok[b] = ok[b] ? 1 : 0;
    all &= ok[b] ? 1 : 0;
  }
  return all;
}

int bls_kzg_blob_commitments(bls_ctx* ctx, const uint8_t* blobs, size_t B, uint8_t* out48, uint8_t* out_ok) {
  API_ENTER(ctx);
  if (B > KZG_MSM_BMAX || (B && (!blobs || !out48))) return BLS_E_ARG;
  CK(kzg_need_setup(ctx, true));
  if (!B) return 1;
  KzgBlobs k;
  CK(kzg_stage_blobs(ctx, blobs, B, nullptr, k));
  std::vector<int> ok(B);
  HIPCK(hipMemcpyAsync(ok.data(), k.ok, B * sizeof(int), hipMemcpyDeviceToHost, ctx->j->stream));
  const int m = kzg_msm(ctx, k.blob, B, out48);  // a blob is its own row of scalars
  if (m <= 0) return m;
  int all = 1;
  for (size_t b = 0; b < B; ++b) {
    if (out_ok) out_ok[b] = ok[b] ? 1 : 0;
    if (!ok[b]) memset(out48 + 48 * b, 0, 48);
    all &= ok[b] ? 1 : 0;
  }
  return all;
}

int bls_kzg_compute_proofs(bls_ctx* ctx, const uint8_t* blobs, size_t B, const uint8_t* z32, uint8_t* proofs48,
                           uint8_t* y32, uint8_t* out_ok) {
  API_ENTER(ctx);
  if (B > KZG_MSM_BMAX || (B && (!blobs || !z32 || !proofs48 || !y32))) return BLS_E_ARG;
  CK(kzg_need_setup(ctx, true));
  if (!B) return 1;
  KzgBlobs k;
  CK(kzg_stage_blobs(ctx, blobs, B, z32, k));
  uint8_t* d_q;
  SCR(S_KB_Q, KZG_BLOB * B, d_q);
  HIPCK(launch_blob_quotient(ctx->j->stream, ctx->kzg_dom, k.f, k.z, k.y, k.hit, B, k.pre, d_q));
  std::vector<int> ok(2 * B);
  HIPCK(hipMemcpyAsync(ok.data(), k.ok, B * sizeof(int), hipMemcpyDeviceToHost, ctx->j->stream));
  HIPCK(hipMemcpyAsync(ok.data() + B, k.zok, B * sizeof(int), hipMemcpyDeviceToHost, ctx->j->stream));
  HIPCK(hipMemcpyAsync(y32, k.y32, 32 * B, hipMemcpyDeviceToHost, ctx->j->stream));
  const int m = kzg_msm(ctx, d_q, B, proofs48);
  if (m <= 0) return m;
  int all = 1;
  for (size_t b = 0; b < B; ++b) {
    if (!ok[B + b]) return 0;  // z >= r
    if (out_ok) out_ok[b] = ok[b] ? 1 : 0;
    if (!ok[b]) memset(proofs48 + 48 * b, 0, 48);
    all &= ok[b] ? 1 : 0;
  }
  return all;
}

int bls_kzg_verify_batch(bls_ctx* ctx, const uint8_t* commitments48, const uint8_t* z32, const uint8_t* y32,
                         const uint8_t* proofs48, size_t n, uint8_t* out_item) {
  API_ENTER(ctx);
  if (n > KZG_ITEMS_MAX || (n && (!commitments48 || !z32 || !y32 || !proofs48))) return BLS_E_ARG;
  CK(kzg_need_setup(ctx, false));
  if (!n) return 1;
  hipStream_t st = ctx->j->stream;
  uint8_t *d_enc, *d_z32, *d_y32;
  Fr *z, *y;
  int *zok, *yok;
  SCR(S_KB_ENC, 96 * n, d_enc);
  SCR(S_KB_Z32, 32 * n, d_z32);
  SCR(S_KB_Y32, 32 * n, d_y32);
  SCR(S_KB_ZF, n, z);
  SCR(S_KB_YF, n, y);
  SCR(S_KB_ZOK, n, zok);
  SCR(S_KB_YOK, n, yok);
  CK(h2d(ctx, d_enc, commitments48, 48 * n));
  CK(h2d(ctx, d_enc + 48 * n, proofs48, 48 * n));
  CK(h2d(ctx, d_z32, z32, 32 * n));
  CK(h2d(ctx, d_y32, y32, 32 * n));
  HIPCK(launch_fr_decode(st, d_z32, n, z, zok));
  HIPCK(launch_fr_decode(st, d_y32, n, y, yok));
  return kzg_verify_dev(ctx, n, d_enc, z, y, zok, yok, nullptr, out_item);
}

int bls_kzg_verify_blob_batch(bls_ctx* ctx, const uint8_t* blobs, const uint8_t* commitments48,
                              const uint8_t* proofs48, const uint8_t* z32, size_t B, uint8_t* out_item) {
  API_ENTER(ctx);
  if (B > KZG_BLOBS_MAX || (B && (!blobs || !commitments48 || !proofs48 || !z32))) return BLS_E_ARG;
  CK(kzg_need_setup(ctx, false));
  if (!B) return 1;
  KzgBlobs k;
  CK(kzg_stage_blobs(ctx, blobs, B, z32, k));
  uint8_t* d_enc;
  SCR(S_KB_ENC, 96 * B, d_enc);
  CK(h2d(ctx, d_enc, commitments48, 48 * B));
  CK(h2d(ctx, d_enc + 48 * B, proofs48, 48 * B));
  return kzg_verify_dev(ctx, B, d_enc, k.z, k.y, k.zok, nullptr, k.ok, out_item);
}

}  // extern "C"
