// C ABI, the Fulu cell KZG functions (kernels: bls_kzg_cells.hip; the transform's pieces: bls_fr_ntt.h).  Everything
// runs on job 0's stream in the S_KC_* slots (the blob decode borrows S_KB_BLOB / S_KB_F / S_KB_OK, as every blob call
// does, and the verification's rows of the resident G1 table's MSM the S_G1M_* slots, as kzg_msm does); no call leaves
// work behind on the stream.
#include "bls_capi_internal.h"
#include "bls_fr_ntt.h"

constexpr size_t KZC_BLOB = 32 * (size_t)NTT_BLOB;
constexpr size_t KZC_CELL = 32 * (size_t)NTT_CELL;   // BYTES_PER_CELL
constexpr size_t KZC_EXT = 32 * (size_t)NTT_EXT;     // a blob's 128 cells
constexpr size_t KZC_BLOBS_MAX = 128;
constexpr size_t KZC_ITEMS_MAX = 8192;  // 128 columns x 64 blobs
constexpr size_t KZC_MSM_ROWS = 511;    // rows per table MSM of the per-item path

static int kzc_ensure_tables(bls_ctx* ctx) {
  if (ctx->kzc_tab) return 0;
  Fr* tab = nullptr;
  HIPCK(hipMalloc(&tab, ntt_tables_bytes()));
  hipError_t e = launch_ntt_tables(ctx->j->stream, tab);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->j->stream);
  if (e != hipSuccess) {  // never keep a table whose build did not complete
    (void)hipFree(tab);
    return fail(ctx, e, "launch_ntt_tables");
  }
  ctx->kzc_tab = tab;
  return 0;
}

// the B coefficient forms in S_KC_COEF (4,096 each) -> their 128 cells each, as bytes in out_cells
static int kzc_extend(bls_ctx* ctx, const Fr* coef, size_t B, uint8_t* out_cells) {
  hipStream_t st = ctx->j->stream;
  Fr *x, *t;
  uint8_t* d_out;
  SCR(S_KC_X, NTT_EXT * B, x);
  SCR(S_KC_T, NTT_EXT * B, t);
  SCR(S_KC_OUT, KZC_EXT * B, d_out);
  HIPCK(launch_ntt(st, ctx->kzc_tab, 13, NTT_DST_BRP, NTT_BLOB, B, coef, NTT_BLOB, t, x, NTT_EXT));
  HIPCK(launch_fr_encode(st, x, NTT_EXT * B, d_out));
  return d2h(ctx, out_cells, d_out, KZC_EXT * B);
}

static int kzc_need_setup(bls_ctx* ctx) {
  if (!ctx->kzc_set) {
    ctx->err = "no cell KZG setup";
    return BLS_E_NOREG;
  }
  if (!ctx->g1t || ctx->kzc_gen != ctx->g1t_gen) {
    ctx->err = "the G1 table was replaced after bls_kzg_cells_setup";
    return BLS_E_ARG;
  }
  return 0;
}

// B rows of 64 scalars over the setup's monomial entries; the affine results stay at *aff (and *live) in the S_G1M_*
// slots until the next table MSM.  Nothing is waited for.
static int kzc_msm(bls_ctx* ctx, const uint8_t* d_rows, size_t B, const G1A** aff, const int** live) {
  hipStream_t st = ctx->j->stream;
  const G1MsmPlan p = g1_msm_plan(NTT_CELL, B);
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
  HIPCK(launch_g1_table_msm(st, p, ctx->g1t, (uint32_t)ctx->g1t_cap, ctx->g1t_stat, ctx->kzc_idx, NTT_CELL, (uint32_t)B,
                            d_rows, d_u32, d_pa, d_pb, d_u, d_res, d_live, d_aff, d_out, &d_entries));
  uint32_t entries = 0;
  HIPCK(hipMemcpyAsync(&entries, d_entries, sizeof entries, hipMemcpyDeviceToHost, st));
  HIPCK(hipStreamSynchronize(st));  // entries leaves this frame
  ctx->g1t_msm_calls++;
  ctx->g1t_msm_entries += entries;
  *aff = d_aff;
  *live = d_live;
  return 0;
}

extern "C" {

int bls_kzg_cells_setup(bls_ctx* ctx, const uint8_t* g2_tau64_96, uint32_t monomial_first, uint32_t monomial_n) {
  API_ENTER(ctx);
  if (!g2_tau64_96 || monomial_n != NTT_CELL) return BLS_E_ARG;
  hipStream_t st = ctx->j->stream;
  ctx->kzc_set = false;
  if (!ctx->g1t) {
    ctx->err = "no G1 table loaded";
    return BLS_E_NOREG;
  }
  if ((size_t)monomial_first + NTT_CELL > ctx->g1t_n) return BLS_E_ARG;
  for (size_t i = 0; i < NTT_CELL; ++i)
    if (!ctx->g1t_stat_h[monomial_first + i]) return 0;  // an invalid setup point
  CK(kzc_ensure_tables(ctx));
  if (!ctx->kzc_negtau64) HIPCK(hipMalloc(&ctx->kzc_negtau64, sizeof(G2A)));
  if (!ctx->kzc_idx) HIPCK(hipMalloc(&ctx->kzc_idx, NTT_CELL * sizeof(uint32_t)));
  uint8_t* d_in;
  int* d_ok;
  SCR(S_KC_ENC, 96, d_in);
  SCR(S_KC_POK, 1, d_ok);
  CK(h2d(ctx, d_in, g2_tau64_96, 96));
  HIPCK(launch_pt_decode(st, 2, d_in, 1, 1, ctx->kzc_negtau64, d_ok));
  HIPCK(launch_kzg_g2_neg(st, ctx->kzc_negtau64));
  uint32_t idx[NTT_CELL];
  for (uint32_t i = 0; i < NTT_CELL; ++i) idx[i] = monomial_first + i;
  CK(h2d(ctx, ctx->kzc_idx, idx, sizeof idx));
  const int v = all_ok(ctx, d_ok, 1);  // waits for the stream: idx may go
  if (v <= 0) return v;
  ctx->kzc_gen = ctx->g1t_gen;
  ctx->kzc_set = true;
  return 1;
}

int bls_kzg_verify_cells(bls_ctx* ctx, const uint8_t* commitments48, size_t n_commitments,
                         const uint32_t* commitment_index, const uint32_t* cell_index, const uint8_t* cells,
                         const uint8_t* proofs48, size_t n, uint8_t* out_item) {
  API_ENTER(ctx);
  if (n > KZC_ITEMS_MAX || n_commitments > KZC_ITEMS_MAX ||
      (n && (!commitments48 || !n_commitments || !commitment_index || !cell_index || !cells || !proofs48)))
    return BLS_E_ARG;
  for (size_t k = 0; k < n; ++k)
    if (commitment_index[k] >= n_commitments) return BLS_E_ARG;
  CK(kzc_need_setup(ctx));
  if (!n) return 1;
  hipStream_t st = ctx->j->stream;
  const size_t nc = n_commitments, np = nc + 2 * n + 1;
  const Fr* W = ctx->kzc_tab;
  uint8_t *d_enc, *d_cells, *K, *rli, *d_seed;
  uint32_t *cidx, *kidx, *d_sel;
  G1A *P, *S, *PP;
  G2A* PQ;
  G1J *tmp, *sums;
  int *pok, *cok, *live, *d_res;
  Fr *coef, *rfr, *part;
  Fp12* fv;
  SCR(S_KC_ENC, 48 * (nc + n), d_enc);
  SCR(S_KC_IN, KZC_CELL * n, d_cells);
  SCR(S_KC_CIDX, n, cidx);
  SCR(S_KC_KIDX, n, kidx);
  SCR(S_KC_P, np, P);
  SCR(S_KC_POK, nc + n, pok);
  SCR(S_KC_COK, n, cok);
  SCR(S_KC_CF, NTT_CELL * n, coef);
  SCR(S_KC_RFR, n, rfr);
  SCR(S_KC_PART, NTT_CELL * cells_colsum_groups(n), part);
  SCR(S_KC_RLI, 32 * NTT_CELL, rli);
  SCR(S_KC_K, 32 * np, K);
  SCR(S_KC_S, np, S);
  SCR(S_KC_LIVE, np, live);
  SCR(S_KC_J, 1100, tmp);
  SCR(S_KC_SUM, 2, sums);
  SCR(S_KC_SEED, 32, d_seed);
  SCR(S_KC_PP, 2 * n, PP);
  SCR(S_KC_PQ, 2 * n, PQ);
  SCR(S_KC_FV, n + 1, fv);
  SCR(S_KC_SEL, n, d_sel);
  SCR(S_KC_RES, n, d_res);
  CK(h2d(ctx, d_enc, commitments48, 48 * nc));
  CK(h2d(ctx, d_enc + 48 * nc, proofs48, 48 * n));
  CK(h2d(ctx, d_cells, cells, KZC_CELL * n));
  CK(h2d(ctx, cidx, commitment_index, n * sizeof(uint32_t)));
  CK(h2d(ctx, kidx, cell_index, n * sizeof(uint32_t)));
  HIPCK(launch_g1_decode_checked(st, d_enc, nc + n, P, pok));
  HIPCK(launch_cells_interp(st, d_cells, kidx, n, W, coef, cok));
  std::vector<int> v(nc + 2 * n, 1);
  HIPCK(hipMemcpyAsync(v.data(), pok, (nc + n) * sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCK(hipMemcpyAsync(v.data() + nc + n, cok, n * sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCK(hipStreamSynchronize(st));
  bool good = true;
  for (size_t k = 0; k < n; ++k) {
    const bool g = v[commitment_index[k]] && v[nc + k] && v[nc + n + k];
    if (out_item) out_item[k] = g ? 1 : 0;
    good = good && g;
  }
  if (!good) return 0;
  uint8_t seed[32];
  CK(host_seed(ctx, seed));
  CK(h2d(ctx, d_seed, seed, 32));
  HIPCK(hipStreamSynchronize(st));  // the seed leaves this frame
  HIPCK(launch_cells_rlc(st, d_seed, nc, n, cidx, kidx, W, coef, rfr, part, P, K, rli));
  const G1A* m_aff;
  const int* m_live;
  CK(kzc_msm(ctx, rli, 1, &m_aff, &m_live));  // -sum_m s_m [tau^m]_1
  HIPCK(launch_g1_scale(st, P, K, np, S, live));
  HIPCK(launch_cells_put(st, m_aff, m_live, S + nc + n, live + nc + n));
  // sums[0] = sum w_i C_i + sum r_k h_k^64 pi_k - sum_m s_m [tau^m]_1, sums[1] = sum r_k pi_k:
  // e(sums[1], -[tau^64] G2) e(sums[0], G2) is the batch's product
  HIPCK(launch_g1_sum_aff(st, S, live, nc + n + 1, tmp, sums));
  HIPCK(launch_g1_sum_aff(st, S + nc + n + 1, live + nc + n + 1, n, tmp, sums + 1));
  HIPCK(launch_kzg_pairs(st, sums, ctx->kzc_negtau64, PP, PQ));
  size_t nf = 0;
  HIPCK(launch_miller_call(st, PP, PQ, 2, fv, &nf, nullptr));
  const int r = run_final_check(ctx, fv, (int)nf, true);
  if (r != 0 || !out_item) return r;  // passed (out_item is all ones), failed without verdicts wanted, or an error
  // each item's own check: the interpolants' commitments as rows of the table MSM, then 2 n pairs on the two-pair
  // kernel, whose workgroup k multiplies item k's two values
  if (miller_wide_nf(2) != 1) return BLS_E_DEVICE;
  uint8_t* rows;
  G1A* I;
  SCR(S_KC_ROWS, KZC_CELL * n, rows);
  SCR(S_KC_I, n, I);
  HIPCK(launch_fr_encode(st, coef, NTT_CELL * n, rows));
  for (size_t s = 0; s < n; s += KZC_MSM_ROWS) {
    const size_t c = n - s < KZC_MSM_ROWS ? n - s : KZC_MSM_ROWS;
    CK(kzc_msm(ctx, rows + KZC_CELL * s, c, &m_aff, &m_live));
    HIPCK(hipMemcpyAsync(I + s, m_aff, c * sizeof(G1A), hipMemcpyDeviceToDevice, st));
  }
  HIPCK(launch_cells_item_pairs(st, nc, n, P, cidx, kidx, I, W, ctx->kzc_negtau64, PP, PQ));
  HIPCK(launch_miller_wide_n(st, PP, PQ, nullptr, 2 * n, fv));
  std::vector<uint32_t> sel(n);
  for (size_t k = 0; k < n; ++k) sel[k] = (uint32_t)k;
  std::vector<int> res(n, 0);
  CK(run_final_checks_sel(ctx, fv, sel.data(), n, d_sel, d_res, res.data()));
  for (size_t k = 0; k < n; ++k) out_item[k] = res[k] ? 1 : 0;
  return 0;
}

int bls_kzg_compute_cells(bls_ctx* ctx, const uint8_t* blobs, size_t B, uint8_t* cells, uint8_t* out_ok) {
  API_ENTER(ctx);
  if (B > KZC_BLOBS_MAX || (B && (!blobs || !cells))) return BLS_E_ARG;
  if (!B) return 1;
  hipStream_t st = ctx->j->stream;
  CK(kzc_ensure_tables(ctx));
  uint8_t* d_blob;
  Fr *f, *t, *coef;
  int* d_ok;
  SCR(S_KB_BLOB, KZC_BLOB * B, d_blob);
  SCR(S_KB_F, NTT_BLOB * B, f);
  SCR(S_KB_OK, B, d_ok);
  SCR(S_KC_T, NTT_EXT * B, t);
  SCR(S_KC_COEF, NTT_BLOB * B, coef);
  CK(h2d(ctx, d_blob, blobs, KZC_BLOB * B));
  HIPCK(launch_blob_decode(st, d_blob, B, f, d_ok));
  // the blob is p on the domain in bit-reversed order: its coefficients are the inverse transform of that order undone
  HIPCK(launch_ntt(st, ctx->kzc_tab, 12, NTT_INV | NTT_SRC_BRP, NTT_BLOB, B, f, NTT_BLOB, t, coef, NTT_BLOB));
  std::vector<int> ok(B);
  HIPCK(hipMemcpyAsync(ok.data(), d_ok, B * sizeof(int), hipMemcpyDeviceToHost, st));
  CK(kzc_extend(ctx, coef, B, cells));
  int all = 1;
  for (size_t b = 0; b < B; ++b) {
    if (out_ok) out_ok[b] = ok[b] ? 1 : 0;
    if (!ok[b]) memset(cells + KZC_EXT * b, 0, KZC_EXT);
    all &= ok[b] ? 1 : 0;
  }
  return all;
}

int bls_kzg_recover_cells(bls_ctx* ctx, const uint32_t* cell_index, size_t n_present, const uint8_t* cells, size_t B,
                          uint8_t* out_cells, uint8_t* out_ok) {
  API_ENTER(ctx);
  if (B > KZC_BLOBS_MAX || !cell_index || n_present < NTT_CELLS / 2 || n_present > NTT_CELLS ||
      (B && (!cells || !out_cells)))
    return BLS_E_ARG;
  uint8_t present[NTT_CELLS] = {0};
  for (size_t p = 0; p < n_present; ++p) {
    if (cell_index[p] >= NTT_CELLS || (p && cell_index[p] <= cell_index[p - 1])) return BLS_E_ARG;
    present[cell_index[p]] = 1;
  }
  if (!B) return 1;
  hipStream_t st = ctx->j->stream;
  CK(kzc_ensure_tables(ctx));
  const Fr *W = ctx->kzc_tab, *P7 = W + NTT_EXT, *P7I = W + 2 * NTT_EXT;
  uint8_t *d_in, *d_pres;
  uint32_t* d_idx;
  Fr *x, *y, *t, *coef, *zd, *zci;
  int* d_bad;
  SCR(S_KC_IN, KZC_CELL * n_present * B, d_in);
  SCR(S_KC_IDX, n_present, d_idx);
  SCR(S_KC_PRES, NTT_CELLS, d_pres);
  SCR(S_KC_X, NTT_EXT * B, x);
  SCR(S_KC_Y, NTT_EXT * B, y);
  SCR(S_KC_T, NTT_EXT * B, t);
  SCR(S_KC_COEF, NTT_BLOB * B, coef);
  SCR(S_KC_ZD, NTT_CELLS, zd);
  SCR(S_KC_ZCI, NTT_CELLS, zci);
  SCR(S_KC_BAD, B, d_bad);
  CK(h2d(ctx, d_in, cells, KZC_CELL * n_present * B));
  CK(h2d(ctx, d_idx, cell_index, n_present * sizeof(uint32_t)));
  CK(h2d(ctx, d_pres, present, NTT_CELLS));
  HIPCK(hipMemsetAsync(x, 0, NTT_EXT * B * sizeof(Fr), st));
  HIPCK(hipMemsetAsync(d_bad, 0, B * sizeof(int), st));
  HIPCK(launch_cells_scatter(st, d_in, d_idx, (uint32_t)n_present, B, x, d_bad));
  HIPCK(launch_cells_vanish(st, d_pres, W, zd, zci));
  // (E Z) on the domain, in natural order; its coefficients; those of (E Z)(7 X); (P Z)(7 w^n) / Z(7 w^n) = P(7 w^n);
  // the coefficients of P(7 X); those of P
  HIPCK(launch_cells_pointwise(st, x, y, NTT_EXT, B, true, zd, NTT_CELLS - 1));
  HIPCK(launch_ntt(st, W, 13, NTT_INV, NTT_EXT, B, y, NTT_EXT, t, y, NTT_EXT));
  HIPCK(launch_cells_pointwise(st, y, y, NTT_EXT, B, false, P7, NTT_EXT - 1));
  HIPCK(launch_ntt(st, W, 13, 0, NTT_EXT, B, y, NTT_EXT, t, y, NTT_EXT));
  HIPCK(launch_cells_pointwise(st, y, y, NTT_EXT, B, false, zci, NTT_CELLS - 1));
  HIPCK(launch_ntt(st, W, 13, NTT_INV, NTT_EXT, B, y, NTT_EXT, t, y, NTT_EXT));
  HIPCK(launch_cells_pointwise(st, y, coef, NTT_BLOB, B, false, P7I, NTT_EXT - 1));
  std::vector<int> bad(B);
  HIPCK(hipMemcpyAsync(bad.data(), d_bad, B * sizeof(int), hipMemcpyDeviceToHost, st));
  CK(kzc_extend(ctx, coef, B, out_cells));
  int all = 1;
  for (size_t b = 0; b < B; ++b) {
    if (out_ok) out_ok[b] = bad[b] ? 0 : 1;
    if (bad[b]) memset(out_cells + KZC_EXT * b, 0, KZC_EXT);
    all &= bad[b] ? 0 : 1;
  }
  return all;
}

}  // extern "C"
