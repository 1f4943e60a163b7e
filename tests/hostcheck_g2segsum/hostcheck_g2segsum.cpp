// TEST HARNESS ONLY: host build of the segmented G2 sum (bls_g2_segsum.h: the per-lane fold that k_g2_seg_fold runs,
// over the plan of bls_g1_segsum.h) with the digit form's 128-bit column, value and subtraction-precondition checks
// compiled in (BLS_FQ_CHECK), for tests/test_aggregate_grouped_cpu.py.
#define BLS_FQ_CHECK 1
#define BLS_HD __host__ __device__ inline  // no forced inlining in this (host-only, checked) unit
#include "bls_ops.h"
#include "bls_g2_segsum.h"
#include <string.h>
#include <vector>
using namespace bls;

static Fp in_fp(const uint8_t* b) { return fp_to_mont(raw_from_be48(b)); }
static void out_fp(uint8_t* b, const Fp& a) { raw_to_be48(fp_from_mont(a), b); }
static Fp2 in_fp2(const uint8_t* b) { return Fp2{in_fp(b), in_fp(b + 48)}; }
static void out_fp2(uint8_t* b, const Fp2& a) {
  out_fp(b, a.c0);
  out_fp(b + 48, a.c1);
}

extern "C" uint32_t hc_g2seg_k() { return SEG_K; }

// The complete formulas have no exceptional case when E2(Fp2) has no point of order 2, i.e. when its order h2 r is
// odd.  h2 = (x^8 - 4 x^7 + 5 x^6 - 4 x^4 + 6 x^3 - 4 x^2 - 4 x + 13) / 9 for the curve parameter x = -X_ABS: the
// numerator N is 9 h2, so h2 is odd exactly when N mod 18 == 9.  Returns h2 mod 2, or -1 when 9 does not divide N
// (X_ABS is not the parameter this argument is about); the test checks r's parity itself.
extern "C" int hc_g2_cofactor_parity() {
  const int x = (int)(18 - (X_ABS % 18)) % 18;  // x mod 18
  const int c[9] = {13, -4, -4, 6, -4, 0, 5, -4, 1};  // coefficients of x^0 .. x^8
  int n = 0, xp = 1;
  for (int k = 0; k < 9; ++k) {
    n = ((n + c[k] * xp) % 18 + 18) % 18;
    xp = xp * x % 18;
  }
  if (n % 9) return -1;
  return n == 9 ? 1 : 0;
}

// The plan of gid[0 .. B) over G groups, then every level's runs in launch order, one "lane" per run.
// pts: the members' affine points, x.c0 || x.c1 || y.c0 || y.c1 (48 B big-endian each); kind: 0 = that point,
// 1 = the identity (a valid member), 2 = a member whose decode failed; include: nullable mask.
// out: G affine sums in the same layout (zero bytes when not an affine point); ok[g]: 0 = not ok, 1 = ok with an
// affine sum, 2 = ok and the sum is the identity; info: {levels, runs, partials of level 0}.
// Returns 0, or -1 when the plan refuses its input.
extern "C" int hc_g2seg_sum(const uint32_t* gid, size_t B, size_t G, const uint8_t* pts, const uint8_t* kind,
                            const uint8_t* include, uint8_t* out, int* ok, uint32_t* info) {
  SegPlan p;
  if (!seg_plan(gid, B, G, p)) return -1;
  std::vector<G2A> a(B);
  std::vector<int> dok(B);
  for (size_t i = 0; i < B; ++i) {
    a[i] = G2A{in_fp2(pts + 192 * i), in_fp2(pts + 192 * i + 96), kind[i] == 1};
    dok[i] = kind[i] == 2 ? 0 : 1;
    if (kind[i]) a[i] = G2A{fp2_zero(), fp2_zero(), true};  // what the decode kernels leave for both
  }
  std::vector<G2SP> tmp[2], gsum(G);
  tmp[0].resize(p.max_tmp() + 1);
  tmp[1].resize(p.max_tmp() + 1);
  std::vector<int> seen(G, 0);
  for (size_t l = 0; l < p.levels(); ++l) {
    const G2SP* prev = tmp[(l + 1) & 1].data();
    G2SP* cur = tmp[l & 1].data();
    for (uint32_t t = p.level_off[l]; t < p.level_off[l + 1]; ++t) {
      const SegRun& r = p.runs[t];
      if (r.cnt > SEG_K) return -2;
      if (r.dst & SEG_FINAL) {
        if (seen[r.dst & ~SEG_FINAL]++) return -3;  // one final run per group
      } else if (r.dst >= p.level_tmp[l]) {
        return -4;
      }
      uint32_t flags = 0;
      const G2Q acc = l == 0 ? seg2_fold_items(r, p.grp_items.data(), dok.data(), include, a.data(), flags)
                             : seg2_fold_partials(r, prev, flags);
      seg2_store(r, acc, flags, cur, gsum.data());
    }
  }
  for (size_t g = 0; g < G; ++g) {
    if (seen[g] != 1) return -5;
    memset(out + 192 * g, 0, 192);
    ok[g] = gsum[g].flags == G2S_SOME ? 1 : 0;
    if (!ok[g]) continue;
    if (fp2_is_zero(gsum[g].z)) {
      ok[g] = 2;
      continue;
    }
    const Fp2 zi = fp2_inv(gsum[g].z);
    out_fp2(out + 192 * g, fp2_mul(gsum[g].x, zi));
    out_fp2(out + 192 * g + 96, fp2_mul(gsum[g].y, zi));
  }
  info[0] = (uint32_t)p.levels();
  info[1] = (uint32_t)p.runs.size();
  info[2] = p.level_tmp.empty() ? 0 : p.level_tmp[0];
  return 0;
}
