// TEST HARNESS ONLY: host build of the RLC signature MSM's bucket folds (bls_g2_msm.h: the per-lane code that
// k_msm_fold0 / k_msm_fold1 run) with the digit form's 128-bit column, value and subtraction-precondition checks
// compiled in (BLS_FQ_CHECK), for tests/test_g2msm_cpu.py.
#define BLS_FQ_CHECK 1
#define BLS_HD __host__ __device__ inline  // no forced inlining in this (host-only, checked) unit
#include "bls_ops.h"
#include "bls_g2_msm.h"
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

extern "C" uint32_t hc_g2msm_kmax() { return G2M_KMAX; }

// a bucket sum as k_msm_usum reads it (six packed Fp) -> out: the affine point (192 B) and 1, or 2 when Z = 0 (then
// out holds X || Y, which the complete formulas leave as (0, Y != 0)); zero bytes otherwise
static int out_sum(const Fp* s, uint8_t* out) {
  const Fp2 X{s[0], s[1]}, Y{s[2], s[3]}, Z{s[4], s[5]};
  if (fp2_is_zero(Z)) {
    out_fp2(out, X);
    out_fp2(out + 96, Y);
    return 2;
  }
  const Fp2 zi = fp2_inv(Z);
  out_fp2(out, fp2_mul(X, zi));
  out_fp2(out + 96, fp2_mul(Y, zi));
  return 1;
}

// One bucket as the two kernels treat it.  pts: affine points, x.c0 || x.c1 || y.c0 || y.c1 (48 B big-endian each);
// lst[0 .. n): the bucket's entries (indices into pts); K: entries per run.  Level 0 runs one "lane" per run of the
// even cut, level 1 the bucket's lane.  info: {runs, longest run, shortest run}.  Returns out_sum's code.
extern "C" int hc_g2msm_bucket(const uint8_t* pts, size_t npts, const uint32_t* lst, uint32_t n, uint32_t K,
                               uint8_t* out, uint32_t* info) {
  std::vector<G2A> sig(npts);
  for (size_t i = 0; i < npts; ++i) sig[i] = G2A{in_fp2(pts + 192 * i), in_fp2(pts + 192 * i + 96), false};
  const uint32_t runs = g2m_nruns(n, K);
  std::vector<G2SP> part(runs + 1);
  Fp csum[6];
  memset(csum, 0xff, sizeof csum);
  info[0] = runs, info[1] = 0, info[2] = ~0u;
  uint32_t covered = 0;
  for (uint32_t j = 0; j < runs; ++j) {  // k_msm_fold0
    const G2mRun g = g2m_run(n, runs, j);
    if (g.src != covered || !g.cnt || g.cnt > K) return -1;  // the runs tile the list, none longer than K
    covered += g.cnt;
    info[1] = g.cnt > info[1] ? g.cnt : info[1];
    info[2] = g.cnt < info[2] ? g.cnt : info[2];
    g2m_store_run(&part[j], csum, runs == 1, g2m_fold_records(sig.data(), lst + g.src, g.cnt));
  }
  if (covered != n) return -1;
  if (runs != 1) {  // k_msm_fold1
    if (!runs) g2m_store_identity(csum);
    else g2m_store_sum(csum, g2m_fold_partials(part.data(), runs));
  }
  memset(out, 0, 192);
  return out_sum(csum, out);
}

// the partial fold alone: cnt >= 1 canonical projective partials, X || Y || Z (two 48-B big-endian each)
extern "C" int hc_g2msm_partials(const uint8_t* prj, uint32_t cnt, uint8_t* out) {
  std::vector<G2SP> part(cnt);
  for (uint32_t i = 0; i < cnt; ++i)
    part[i] = G2SP{in_fp2(prj + 288 * i), in_fp2(prj + 288 * i + 96), in_fp2(prj + 288 * i + 192), 0};
  Fp csum[6];
  g2m_store_sum(csum, g2m_fold_partials(part.data(), cnt));
  memset(out, 0, 192);
  return out_sum(csum, out);
}
