// C ABI, the Fulu cell KZG functions (kernels: bls_kzg_cells.hip; the transform's pieces: bls_fr_ntt.h).  Everything
// runs on job 0's stream in the S_KC_* slots (the blob decode borrows S_KB_BLOB / S_KB_F / S_KB_OK, as every blob call
// does, and the verification's rows of the resident G1 table's MSM the S_G1M_* slots, as kzg_msm does); no call leaves
// work behind on the stream.  The cell proofs and the G1 transform (kernels and derivation: bls_g1_fft.hip,
// bls_g1_fft.h) work in the S_KP_* slots on the coefficient form a cell call leaves in S_KC_COEF.
#include "bls_capi_internal.h"
#include "bls_fr_ntt.h"

constexpr size_t KZC_BLOB = 32 * (size_t)NTT_BLOB;
constexpr size_t KZC_CELL = 32 * (size_t)NTT_CELL;   // BYTES_PER_CELL
constexpr size_t KZC_EXT = 32 * (size_t)NTT_EXT;     // a blob's 128 cells
constexpr size_t KZC_BLOBS_MAX = 128;
constexpr size_t KZC_ITEMS_MAX = 8192;  // 128 columns x 64 blobs
constexpr size_t KZC_MSM_ROWS = 511;    // rows per table MSM of the per-item path
constexpr size_t KZP_BLOBS_PER_MSM = 8;  // cell proofs: 63 rows per blob, 504 <= KZC_MSM_ROWS
constexpr uint32_t KZP_FFT_LOG = 7;      // the proofs' 128-point transform
constexpr size_t G1FFT_POINTS_MAX = (size_t)1 << 20;  // n B of one bls_g1_fft call

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

// B rows of n scalars over the table entries d_idx (a setup's monomial entries); the affine results stay at *aff (and
// *live) in the S_G1M_* slots until the next table MSM.
static int kzc_msm(bls_ctx* ctx, const uint32_t* d_idx, size_t n, const uint8_t* d_rows, size_t B, const G1A** aff,
                   const int** live) {
  hipStream_t st = ctx->j->stream;
  const G1MsmPlan p = g1_msm_plan(n, B);
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
  HIPCK(launch_g1_table_msm(st, p, ctx->g1t, (uint32_t)ctx->g1t_cap, ctx->g1t_stat, d_idx, (uint32_t)n, (uint32_t)B,
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

static int kzp_need_setup(bls_ctx* ctx) {
  if (!ctx->kp_set) {
    ctx->err = "no cell proof setup";
    return BLS_E_NOREG;
  }
  if (!ctx->g1t || ctx->kp_gen != ctx->g1t_gen) {
    ctx->err = "the G1 table was replaced after bls_kzg_cell_proofs_setup";
    return BLS_E_ARG;
  }
  return 0;
}

// The blobs' coefficient forms into S_KC_COEF (*coef) and, unless cells is null, their cells; good[b] = every element
// of blob b is below r.  The stream is idle on return.
static int kzc_compute(bls_ctx* ctx, const uint8_t* blobs, size_t B, uint8_t* cells, std::vector<int>& good,
                       const Fr** coef_out) {
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
  good.resize(B);
  HIPCK(hipMemcpyAsync(good.data(), d_ok, B * sizeof(int), hipMemcpyDeviceToHost, st));
  if (cells) CK(kzc_extend(ctx, coef, B, cells));
  else HIPCK(hipStreamSynchronize(st));
  *coef_out = coef;
  return 0;
}

// out_ok, the zeroed outputs of the blobs that are not good, and the call's return value
static int kzc_report(size_t B, const std::vector<int>& good, uint8_t* cells, uint8_t* proofs48, uint8_t* out_ok) {
  int all = 1;
  for (size_t b = 0; b < B; ++b) {
    if (out_ok) out_ok[b] = good[b] ? 1 : 0;
    if (!good[b] && cells) memset(cells + KZC_EXT * b, 0, KZC_EXT);
    if (!good[b] && proofs48) memset(proofs48 + 48 * NTT_CELLS * b, 0, 48 * NTT_CELLS);
    all &= good[b] ? 1 : 0;
  }
  return all;
}

static int kzc_recover_args(const uint32_t* cell_index, size_t n_present, const uint8_t* cells, size_t B,
                            const uint8_t* out, uint8_t present[NTT_CELLS]) {
  if (B > KZC_BLOBS_MAX || !cell_index || n_present < NTT_CELLS / 2 || n_present > NTT_CELLS || (B && (!cells || !out)))
    return BLS_E_ARG;
  memset(present, 0, NTT_CELLS);
  for (size_t p = 0; p < n_present; ++p) {
    if (cell_index[p] >= NTT_CELLS || (p && cell_index[p] <= cell_index[p - 1])) return BLS_E_ARG;
    present[cell_index[p]] = 1;
  }
  return 0;
}

// The recovered coefficient forms into S_KC_COEF (*coef) and, unless out_cells is null, the 128 cells of every blob;
// good[b] = every given element of blob b is below r.  The stream is idle on return.
static int kzc_recover(bls_ctx* ctx, const uint32_t* cell_index, size_t n_present, const uint8_t* present,
                       const uint8_t* cells, size_t B, uint8_t* out_cells, std::vector<int>& good,
                       const Fr** coef_out) {
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
  good.resize(B);
  HIPCK(hipMemcpyAsync(good.data(), d_bad, B * sizeof(int), hipMemcpyDeviceToHost, st));
  if (out_cells) CK(kzc_extend(ctx, coef, B, out_cells));
  else HIPCK(hipStreamSynchronize(st));
  for (size_t b = 0; b < B; ++b) good[b] = good[b] ? 0 : 1;
  *coef_out = coef;
  return 0;
}

// The 128 proofs of each of the B coefficient forms at coef, in cell order (bls_g1_fft.h has the derivation): the
// h_m as 63 rows per blob of the table MSM over the monomial entries 0 .. 4,031, KZP_BLOBS_PER_MSM blobs per call,
// copied into the transform's buffer behind each call; then one 128-point transform over all blobs, whose
// bit-reversed output order is the cells' order, and one compression.
static int kzp_proofs(bls_ctx* ctx, const Fr* coef, size_t B, uint8_t* proofs48) {
  hipStream_t st = ctx->j->stream;
  const size_t R = cellproof_rows_per_blob(), N = cellproof_row_entries();
  const size_t per = B < KZP_BLOBS_PER_MSM ? B : KZP_BLOBS_PER_MSM;
  uint8_t *rows, *d_out;
  G1P *buf, *perm;
  G1A* aff;
  int* live;
  SCR(S_KP_ROWS, 32 * N * R * per, rows);
  SCR(S_KP_BUF, NTT_CELLS * B, buf);
  SCR(S_KP_PERM, NTT_CELLS * B, perm);
  SCR(S_KP_LIVE, NTT_CELLS * B, live);
  SCR(S_KP_AFF, NTT_CELLS * B, aff);
  SCR(S_KP_OUT, 48 * NTT_CELLS * B, d_out);
  for (size_t s = 0; s < B; s += per) {
    const size_t c = B - s < per ? B - s : per;
    const G1A* m_aff;
    const int* m_live;
    HIPCK(launch_cellproof_rows(st, coef + NTT_BLOB * s, c, rows));
    CK(kzc_msm(ctx, ctx->kp_idx, N, rows, R * c, &m_aff, &m_live));
    HIPCK(launch_g1fft_load(st, m_aff, m_live, (uint32_t)R, KZP_FFT_LOG, c, buf + NTT_CELLS * s));
  }
  HIPCK(launch_g1fft(st, ctx->kzc_tab, KZP_FFT_LOG, false, B, buf));
  HIPCK(launch_g1fft_finish(st, buf, KZP_FFT_LOG, B, false, perm, live, aff, d_out));
  return d2h(ctx, proofs48, d_out, 48 * NTT_CELLS * B);
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
  CK(kzc_msm(ctx, ctx->kzc_idx, NTT_CELL, rli, 1, &m_aff, &m_live));  // -sum_m s_m [tau^m]_1
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
    CK(kzc_msm(ctx, ctx->kzc_idx, NTT_CELL, rows + KZC_CELL * s, c, &m_aff, &m_live));
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
  std::vector<int> good;
  const Fr* coef;
  CK(kzc_compute(ctx, blobs, B, cells, good, &coef));
  return kzc_report(B, good, cells, nullptr, out_ok);
}

int bls_kzg_recover_cells(bls_ctx* ctx, const uint32_t* cell_index, size_t n_present, const uint8_t* cells, size_t B,
                          uint8_t* out_cells, uint8_t* out_ok) {
  API_ENTER(ctx);
  uint8_t present[NTT_CELLS];
  CK(kzc_recover_args(cell_index, n_present, cells, B, out_cells, present));
  if (!B) return 1;
  std::vector<int> good;
  const Fr* coef;
  CK(kzc_recover(ctx, cell_index, n_present, present, cells, B, out_cells, good, &coef));
  return kzc_report(B, good, out_cells, nullptr, out_ok);
}

int bls_g1_fft(bls_ctx* ctx, const uint8_t* in48, size_t n, size_t B, int inverse, uint8_t* out48) {
  API_ENTER(ctx);
  uint32_t logn = 0;
  while (logn < 12 && ((size_t)1 << logn) < n) ++logn;
  if (n < 2 || ((size_t)1 << logn) != n || !B || B > G1FFT_POINTS_MAX / n || !in48 || !out48) return BLS_E_ARG;
  hipStream_t st = ctx->j->stream;
  CK(kzc_ensure_tables(ctx));
  const size_t total = n * B;
  uint8_t *d_in, *d_out;
  G1A *A, *aff;
  G1P *buf, *perm;
  int *ok, *live;
  SCR(S_KP_IN, 48 * total, d_in);
  SCR(S_KP_A, total, A);
  SCR(S_KP_OK, total, ok);
  SCR(S_KP_BUF, total, buf);
  SCR(S_KP_PERM, total, perm);
  SCR(S_KP_LIVE, total, live);
  SCR(S_KP_AFF, total, aff);
  SCR(S_KP_OUT, 48 * total, d_out);
  CK(h2d(ctx, d_in, in48, 48 * total));
  HIPCK(launch_g1_decode_checked(st, d_in, total, A, ok));
  const int v = all_ok(ctx, ok, total);
  if (v <= 0) return v;
  HIPCK(launch_g1fft_load(st, A, nullptr, (uint32_t)n, logn, B, buf));
  HIPCK(launch_g1fft(st, ctx->kzc_tab, logn, inverse != 0, B, buf));
  HIPCK(launch_g1fft_finish(st, buf, logn, B, true, perm, live, aff, d_out));
  CK(d2h(ctx, out48, d_out, 48 * total));
  return 1;
}

int bls_kzg_cell_proofs_setup(bls_ctx* ctx, uint32_t monomial_first, uint32_t monomial_n) {
  API_ENTER(ctx);
  if (monomial_n != NTT_BLOB) return BLS_E_ARG;
  ctx->kp_set = false;
  if (!ctx->g1t) {
    ctx->err = "no G1 table loaded";
    return BLS_E_NOREG;
  }
  if ((size_t)monomial_first + NTT_BLOB > ctx->g1t_n) return BLS_E_ARG;
  for (size_t i = 0; i < NTT_BLOB; ++i)
    if (!ctx->g1t_stat_h[monomial_first + i]) return 0;  // an invalid setup point
  CK(kzc_ensure_tables(ctx));
  if (!ctx->kp_idx) HIPCK(hipMalloc(&ctx->kp_idx, NTT_BLOB * sizeof(uint32_t)));
  std::vector<uint32_t> idx(NTT_BLOB);
  for (uint32_t i = 0; i < NTT_BLOB; ++i) idx[i] = monomial_first + i;
  CK(h2d(ctx, ctx->kp_idx, idx.data(), NTT_BLOB * sizeof(uint32_t)));
  HIPCK(hipStreamSynchronize(ctx->j->stream));  // idx may go
  ctx->kp_gen = ctx->g1t_gen;
  ctx->kp_set = true;
  return 1;
}

int bls_kzg_compute_cells_and_proofs(bls_ctx* ctx, const uint8_t* blobs, size_t B, uint8_t* cells, uint8_t* proofs48,
                                     uint8_t* out_ok) {
  API_ENTER(ctx);
  if (B > KZC_BLOBS_MAX || (B && (!blobs || !proofs48))) return BLS_E_ARG;
  CK(kzp_need_setup(ctx));
  if (!B) return 1;
  std::vector<int> good;
  const Fr* coef;
  CK(kzc_compute(ctx, blobs, B, cells, good, &coef));
  CK(kzp_proofs(ctx, coef, B, proofs48));
  return kzc_report(B, good, cells, proofs48, out_ok);
}

int bls_kzg_recover_cells_and_proofs(bls_ctx* ctx, const uint32_t* cell_index, size_t n_present, const uint8_t* cells,
                                     size_t B, uint8_t* out_cells, uint8_t* out_proofs48, uint8_t* out_ok) {
  API_ENTER(ctx);
  uint8_t present[NTT_CELLS];
  CK(kzc_recover_args(cell_index, n_present, cells, B, out_cells, present));
  if (B && !out_proofs48) return BLS_E_ARG;
  CK(kzp_need_setup(ctx));
  if (!B) return 1;
  std::vector<int> good;
  const Fr* coef;
  CK(kzc_recover(ctx, cell_index, n_present, present, cells, B, out_cells, good, &coef));
  CK(kzp_proofs(ctx, coef, B, out_proofs48));
  return kzc_report(B, good, out_cells, out_proofs48, out_ok);
}

}  // extern "C"
