// C ABI, the test hooks (bls_test_*).
#include "bls_capi_internal.h"

extern "C" {

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
// (launch_h2c + h2c_fallback, exactly as bls_fav_* run them), compressed: out96[96 i ..] = H(m_i); wide: the same
// through the one-wave-per-message kernel of the per-call path (launch_h2c_wide + h2c_fallback)
static int test_hash_to_g2(bls_ctx* ctx, const uint8_t* msgs32, size_t n, uint8_t* out96, bool wide) {
  if ((!msgs32 || !out96) && n) return BLS_E_ARG;
  if (!n) return 0;
  uint8_t *d_m, *d_out;
  Fd* hf = nullptr;
  G2A* H;
  int* flag;
  SCR(S_IN0, 32 * n, d_m);
  SCR(S_IN2, 96 * n, d_out);
  if (!wide) SCR(S_AV_HCF, h2c_scratch_fd(n), hf);
  SCR(S_AV_FLAG, n, flag);
  SCR(S_G2A, n, H);
  hipStream_t st = ctx->j->stream;
  CK(h2d(ctx, d_m, msgs32, 32 * n));
  HIPCK(wide ? launch_h2c_wide(st, n, d_m, nullptr, H, flag) : launch_h2c(st, n, d_m, nullptr, hf, H, flag));
  CK(h2c_fallback(ctx, st, n, d_m, nullptr, flag, H));
  hipLaunchKernelGGL(k_g2_compress_many, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, n, H, d_out);
  HIPCK(hipGetLastError());
  CK(d2h(ctx, out96, d_out, 96 * n));
  return 0;
}

int bls_test_hash_to_g2_wide(bls_ctx* ctx, const uint8_t* msgs32, size_t n, uint8_t* out96) {
  API_ENTER(ctx);
  return test_hash_to_g2(ctx, msgs32, n, out96, true);
}

int bls_test_hash_to_g2_batch(bls_ctx* ctx, const uint8_t* msgs32, size_t n, uint8_t* out96) {
  API_ENTER(ctx);
  return test_hash_to_g2(ctx, msgs32, n, out96, false);
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
    HIPCK(launch_fe_wide(st, d_f, (int)n, d_r, d_ts));
  else
    HIPCK(launch_final_check_wave(st, d_f, (int)n, d_r));
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
  HIPCK(launch_h2c_wide_dbg(ctx->j->stream, d_m, d_out));
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
  uint8_t* d_out;
  G1A* P;
  G2A* Q;
  Fp12 *f, *ft, *fo;
  uint32_t* L;
  SCR(S_KZ_F, n, f);
  SCR(S_KZ_FT, n / 8 + 16, ft);
  SCR(S_FPART, 1, fo);
  SCR(S_PT_OUT, 8 * 576, d_out);
  SCR(S_KZ_J, miller_lines_u32(n), L);
  const int v = stage_pairs(ctx, g1s48, g2s96, n, false, &P, &Q);
  if (v <= 0) return v;
  for (int k = 0; k < 8; ++k) {
    size_t nf = n;
    if (k == 7) {
      HIPCK(launch_miller_lines(st, Q, n, L));
      HIPCK(launch_miller_acc8(st, P, Q, nullptr, n, L, miller_lines_ld(n), f));
    } else if (k == 6) {
      HIPCK(launch_miller_lines(st, Q, n, L));
      HIPCK(launch_miller_acc4l(st, P, Q, nullptr, n, L, miller_lines_ld(n), f));
      nf = (n + 3) / 4;
    } else if (k == 0 || k == 3 || k == 5) {
      const int G = k == 0 ? 2 : (k == 3 ? 4 : 8);
      HIPCK(launch_miller_lines(st, Q, n, L));
      HIPCK(launch_miller_acc4(st, P, Q, nullptr, n, L, miller_lines_ld(n), f, G));
      nf = (n + G - 1) / G;
    } else if (k == 1 || k == 2) {
      const int G = k == 1 ? 2 : 1;
      HIPCK(launch_miller_fused(st, P, Q, nullptr, n, f, G));
      nf = (n + G - 1) / G;
    } else {
      HIPCK(launch_miller_wave(st, P, Q, nullptr, n, f));
    }
    HIPCK(launch_fp12_prod_vm(st, f, nf, ft, fo));
    HIPCK(launch_gt_final_exp(st, fo, d_out + 576 * k));
  }
  CK(d2h(ctx, out576, d_out, 8 * 576));
  return 1;
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
  HIPCK(launch_wide_selftest(ctx->j->stream, nw, d_in, d_bad));
  CK(d2h(ctx, bad, d_bad, nw * sizeof(int)));
  return 0;
}

// The 64 bit sums of the RLC signature MSM through launch_msm_upairs, the FAV batch's own stage (its scratch slots
// too), compressed.  Both status arrays are the decode's verdicts.
int bls_test_rlc_msm(bls_ctx* ctx, const uint8_t* sigs96, const uint64_t* scalars, size_t n, uint32_t run_len,
                     uint8_t* out) {
  API_ENTER(ctx);
  if (!out || ((!sigs96 || !scalars) && n) || run_len > 16) return BLS_E_ARG;
  hipStream_t st = ctx->j->stream;
  uint8_t *d_in, *d_out;
  uint64_t* rsc;
  G2A *sig, *Q;
  G1A* P;
  int *dstat, *pok;
  uint32_t* mu;
  Fd* mf;
  SCR(S_IN0, 96 * n, d_in);
  SCR(S_RSC, n, rsc);
  SCR(S_SIG, n, sig);
  SCR(S_MSTAT, n, dstat);
  SCR(S_MSMU, msm_scratch_u32(n), mu);
  SCR(S_MSMF, msm_scratch_fd(n, run_len), mf);
  SCR(S_RP, MSM_UPAIRS, P);
  SCR(S_H, MSM_UPAIRS, Q);
  SCR(S_STATUS, MSM_UPAIRS, pok);
  SCR(S_IN2, 96 * MSM_UPAIRS, d_out);
  CK(ensure_comb(ctx, st));
  if (n) {
    CK(h2d(ctx, d_in, sigs96, 96 * n));
    CK(h2d(ctx, rsc, scalars, 8 * n));
    HIPCK(launch_pt_decode(st, 2, d_in, n, 0, sig, dstat));
    const int v = all_ok(ctx, dstat, n);
    if (v <= 0) return v;
  }
  HIPCK(launch_msm_upairs(st, n, dstat, dstat, rsc, sig, mu, mf, ctx->comb, P, Q, pok, run_len));
  hipLaunchKernelGGL(k_g2_compress_many, dim3(1), dim3(64), 0, st, (size_t)MSM_UPAIRS, Q, d_out);
  HIPCK(hipGetLastError());
  CK(d2h(ctx, out, d_out, 96 * MSM_UPAIRS));
  return 1;
}

}  // extern "C"
