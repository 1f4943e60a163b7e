// C ABI, the HBM-resident tables: the key registry and the committee table.
#include "bls_capi_internal.h"

extern "C" {

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
  PROF(P_KEY_VALIDATE, launch_key_validate(ctx->j->stream, d_in, n, d_a, d_ok));
  HIPCK(launch_reg_pack(ctx->j->stream, d_a, d_ok, n, ctx->reg + first, d_valid));
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
  HIPCK(launch_registry_generate(ctx->j->stream, first_sk, n, tmp, ctx->reg, d_out));
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
  HIPCK(launch_fav_gather_bits(st, ctx->ctab_idx, d_items, C, ctx->reg, (uint32_t)ctx->reg_n, nullptr, nullptr, nullptr,
                            ctx->ctab_sum, d_st, ctx->ctab_stat));
  HIPCK(hipStreamSynchronize(st));
  ctx->ctab_gen = ctx->reg_gen;
  ctx->ctab_loaded = true;
  return 1;
}

size_t bls_committees_count(bls_ctx* ctx) {
  return (ctx && ctx->ctab_loaded) ? ctx->ctab_offs_h.size() - 1 : 0;
}

}  // extern "C"
