// C ABI, grouped signature aggregation.
#include "bls_capi_internal.h"

extern "C" {

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
    HIPCK(launch_sig_validate(st, d_sigs, B, a, ok));
  else
    HIPCK(launch_pt_decode(st, 2, d_sigs, B, 0, a, ok));
  for (size_t l = 0; l < sp.levels(); ++l) {
    const uint32_t n = sp.level_off[l + 1] - sp.level_off[l];
    const G2SP* in = (const G2SP*)((l & 1) ? pa : pb);
    G2SP* out = (G2SP*)((l & 1) ? pb : pa);
    HIPCK(launch_g2_seg_fold(st, (int)l, d_runs + sp.level_off[l], n, d_items, ok, d_include, a, in, out, (G2SP*)gsum));
  }
  HIPCK(launch_g2_seg_finish(st, G, (const G2SP*)gsum, d_out96, d_ok));
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

}  // extern "C"
