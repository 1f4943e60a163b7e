// C ABI, the curve and SSZ pieces: pairing checks and products, multi-exponentiations, the curve objects, signing
// roots and merkleization.
#include "bls_capi_internal.h"

// n (G1, G2) pairs staged in the S_KZ_* slots and decoded on the job's stream, identity accepted, with or without
// the subgroup checks: 1, or 0 on a rejected point
int capi::stage_pairs(bls_ctx* ctx, const uint8_t* g1s48, const uint8_t* g2s96, size_t n, bool subgroup, G1A** P,
                      G2A** Q) {
  uint8_t* d_in;
  int *ok1, *ok2;
  SCR(S_KZ_IN, 144 * n, d_in);
  SCR(S_KZ_P, n, *P);
  SCR(S_KZ_Q, n, *Q);
  SCR(S_KZ_OK, n, ok1);
  SCR(S_KZ_OK2, n, ok2);
  CK(h2d(ctx, d_in, g1s48, 48 * n));
  CK(h2d(ctx, d_in + 48 * n, g2s96, 96 * n));
  HIPCK(launch_pairs_decode(ctx->j->stream, d_in, n, subgroup, *P, *Q, ok1, ok2));
  const int a = all_ok(ctx, ok1, n);
  if (a < 0) return a;
  const int b = all_ok(ctx, ok2, n);
  return b < 0 ? b : (a & b);
}

// The product of the Miller values of n staged pairs (identity pairs: an Fp2 factor, 1 after the final
// exponentiation) in *fo: 1, or 0 on a rejected point
static int pairs_product(bls_ctx* ctx, const uint8_t* g1s48, const uint8_t* g2s96, size_t n, bool subgroup,
                         Fp12** fo) {
  G1A* P;
  G2A* Q;
  Fp12 *f, *ft;
  SCR(S_KZ_F, n, f);
  SCR(S_KZ_FT, n / 8 + 16, ft);
  SCR(S_FPART, 1, *fo);
  const int v = stage_pairs(ctx, g1s48, g2s96, n, subgroup, &P, &Q);
  if (v <= 0) return v;
  size_t nf = 0;
  HIPCK(launch_miller_call(ctx->j->stream, P, Q, n, f, &nf, nullptr));
  HIPCK(launch_fp12_prod_vm(ctx->j->stream, f, nf, ft, *fo));
  return 1;
}

extern "C" {

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
  HIPCK(launch_sha256_pairs(ctx->j->stream, d_l, d_r, domain_stride, n, d_o));
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
      HIPCK(launch_merkleize(ctx->j->stream, d_z, d_a, 1, 1, d_z, &r));
      HIPCK(hipMemcpyAsync(d_z, r, 32, hipMemcpyDeviceToDevice, ctx->j->stream));
    }
    CK(d2h(ctx, root32, d_z, 32));
    return 1;
  }
  CK(h2d(ctx, d_a, chunks32, 32 * n));
  HIPCK(launch_merkleize(ctx->j->stream, d_a, d_b, n, depth, d_z, &root));
  CK(d2h(ctx, root32, root, 32));
  return 1;
}

// pairing_check with the subgroup checks optional (arkworks multi_pairing on
// already-decoded curve objects checks none)
int bls_pairing_check_ex(bls_ctx* ctx, const uint8_t* g1s48, const uint8_t* g2s96, size_t n, int subgroup_check) {
  API_ENTER(ctx);
  if (n && (!g1s48 || !g2s96)) return BLS_E_ARG;
  if (n == 0) return 1;  // empty product
  Fp12* fo;
  const int v = pairs_product(ctx, g1s48, g2s96, n, subgroup_check != 0, &fo);
  return v <= 0 ? v : run_final_check(ctx, fo, 1, true);
}

int bls_pairing_check(bls_ctx* ctx, const uint8_t* g1s48, const uint8_t* g2s96, size_t n) {
  return bls_pairing_check_ex(ctx, g1s48, g2s96, n, 1);
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
    HIPCK(launch_g1_decode_checked(st, d_in, n, P, ok));
    const int v = all_ok(ctx, ok, n);
    if (v <= 0) return v;
    HIPCK(launch_g1_scale(st, P, d_in + 48 * n, n, S, live));
  }
  HIPCK(launch_g1_sum_aff(st, S, live, n, tmp, sum));
  HIPCK(launch_g1_compress(st, sum, d_out, nullptr));
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
  HIPCK(launch_pt_decode(ctx->j->stream, group, d_in, n, subgroup_check ? 1 : 0, d_a, d_ok));
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
  HIPCK(launch_pt_binop(ctx->j->stream, group, d, d + W, d + 2 * W, op, d + 2 * W + 32, d_ok));
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
  HIPCK(launch_pt_decode(st, group, d_in, n, subgroup_check ? 1 : 0, d_a, d_ok));
  const int v = all_ok(ctx, d_ok, n);
  if (v <= 0) return v;
  HIPCK(launch_pt_msm(st, group, d_a, d_in + (size_t)W * n, n, d_tmp, d_out));
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
  uint8_t* d_out;
  Fp12* fo;
  SCR(S_PT_OUT, 576, d_out);
  const int v = pairs_product(ctx, g1s48, g2s96, n, subgroup_check != 0, &fo);
  if (v <= 0) return v;
  HIPCK(launch_gt_final_exp(ctx->j->stream, fo, d_out));
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
  HIPCK(launch_gt_mul(ctx->j->stream, d, d + 576, d + 1152));
  CK(d2h(ctx, out576, d + 1152, 576));
  return 1;
}

}  // extern "C"
