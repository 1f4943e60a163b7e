// TEST HARNESS ONLY: host build of the segmented G1 sum (bls_g1_segsum.h: the plan and the per-lane fold that
// k_g1_seg_fold runs) with the digit form's 128-bit column, value and subtraction-precondition checks compiled in
// (BLS_FQ_CHECK), for tests/test_shared_msgs_cpu.py.
#define BLS_FQ_CHECK 1
#define BLS_HD __host__ __device__ inline  // no forced inlining in this (host-only, checked) unit
#include "bls_ops.h"
#include "bls_g1_segsum.h"
#include <string.h>
#include <vector>
using namespace bls;

static Fp in_fp(const uint8_t* b) { return fp_to_mont(raw_from_be48(b)); }
static void out_fp(uint8_t* b, const Fp& a) { raw_to_be48(fp_from_mont(a), b); }

extern "C" uint32_t hc_seg_k() { return SEG_K; }

// The plan of msg_id[0 .. B) over M table entries, then every level's runs in launch order, one "lane" per run.
// rp: the items' affine points, x || y (48 B big-endian each); status: 0 = skip the item.
// out: M affine sums x || y, 96 zero bytes for the identity; ok[m] = the fold's flag (sum != identity);
// info: {levels, runs, partials of level 0}.  Returns 0, or -1 when the plan refuses its input.
extern "C" int hc_seg_sum(const uint32_t* msg_id, size_t B, size_t M, const uint8_t* rp, const int* status,
                          uint8_t* out, int* ok, uint32_t* info) {
  SegPlan p;
  if (!seg_plan(msg_id, B, M, p)) return -1;
  std::vector<G1A> rP(B);
  for (size_t i = 0; i < B; ++i) rP[i] = G1A{in_fp(rp + 96 * i), in_fp(rp + 96 * i + 48), false};
  std::vector<G1P> tmp[2], gsum(M);
  tmp[0].resize(p.max_tmp() + 1);
  tmp[1].resize(p.max_tmp() + 1);
  std::vector<int> seen(M, 0);
  for (size_t l = 0; l < p.levels(); ++l) {
    const G1P* prev = tmp[(l + 1) & 1].data();
    G1P* cur = tmp[l & 1].data();
    for (uint32_t t = p.level_off[l]; t < p.level_off[l + 1]; ++t) {
      const SegRun& r = p.runs[t];
      if (r.cnt > SEG_K) return -2;
      if (r.dst & SEG_FINAL) {
        if (seen[r.dst & ~SEG_FINAL]++) return -3;  // one final run per group
      } else if (r.dst >= p.level_tmp[l]) {
        return -4;
      }
      const G1Q acc = l == 0 ? seg_fold_items(r, p.grp_items.data(), status, rP.data()) : seg_fold_partials(r, prev);
      seg_store(r, acc, cur, gsum.data(), ok);
    }
  }
  for (size_t m = 0; m < M; ++m) {
    if (seen[m] != 1) return -5;
    memset(out + 96 * m, 0, 96);
    if (fp_is_zero(gsum[m].z)) continue;
    const Fp zi = fp_inv(gsum[m].z);
    out_fp(out + 96 * m, fp_mul(gsum[m].x, zi));
    out_fp(out + 96 * m + 48, fp_mul(gsum[m].y, zi));
  }
  info[0] = (uint32_t)p.levels();
  info[1] = (uint32_t)p.runs.size();
  info[2] = p.level_tmp.empty() ? 0 : p.level_tmp[0];
  return 0;
}
