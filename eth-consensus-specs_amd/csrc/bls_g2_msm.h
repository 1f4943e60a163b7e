// Bucket sums of the RLC signature MSM S = sum_i r_i sigma_i (bls_msm.hip): the per-lane folds, which the kernels
// k_msm_fold0 / k_msm_fold1 and the host check (tests/hostcheck_g2msm, with BLS_FQ_CHECK) both run.
//
// A bucket's sorted list of n entries is cut into ceil(n / K) runs of even length (39 entries at K = 16: 13 + 13 + 13).
// One lane folds one run of signatures (g2m_fold_records); a bucket with more than one run then has its run partials
// folded by one lane (g2m_fold_partials).  Additions are the complete ones of bls_g2_segsum.h (g2q_add_aff /
// g2q_add_mem, digit form, bound-typed); a fold starts from its first operand, so nothing is ever added to the
// identity and a run of n points costs n - 1 additions.
//
// Bounds.  The accumulator contract is bls_g2_segsum.h's (X < G2S_VX p, Y, Z < G2S_VYZ p, digits <= G2S_DL).  An
// accumulator that starts as a canonical point -- an affine signature as (x : y : 1), or a stored partial -- has
// values < p and exact digits: the relax<> below are the static_asserts that this lies inside G2SX / G2SYZ, so the
// declared contract stands unchanged and every later step is an output of g2q_add_aff / g2q_add_mem.
#pragma once
#include "bls_g2_segsum.h"

namespace bls {

// entries per run.  The additions are n - 1 per bucket however it is cut, and a full batch is bound by SIMD time, so
// long runs keep the waves few and even: a C2 batch's ~39 entries per bucket are three runs of 13.
constexpr uint32_t G2M_KMAX = 16;

BLS_HD uint32_t g2m_nruns(uint32_t n, uint32_t K) { return (n + K - 1) / K; }

// run j < runs of a bucket of n entries cut evenly: its first entry and its length (the first n % runs runs are one
// longer)
struct G2mRun {
  uint32_t src, cnt;
};
BLS_HD G2mRun g2m_run(uint32_t n, uint32_t runs, uint32_t j) {
  const uint32_t q = n / runs, rem = n % runs;
  return G2mRun{j * q + (j < rem ? j : rem), q + (j < rem ? 1u : 0u)};
}

// a canonical affine point of E2 (not the identity) as the accumulator (x : y : 1)
BLS_HD G2Q g2m_from_affine(const Fq2C& x, const Fq2C& y) {
  return G2Q{relax<G2S_VX, G2S_DL>(x), relax<G2S_VYZ, G2S_DL>(y), relax<G2S_VYZ, G2S_DL>(fq2b_canon(fp2_one()))};
}

// a stored partial (canonical projective) as the accumulator
BLS_HD G2Q g2m_from_partial(const G2SP* q) {
  return G2Q{relax<G2S_VX, G2S_DL>(fq2b_canon(q->x)), relax<G2S_VYZ, G2S_DL>(fq2b_canon(q->y)),
             relax<G2S_VYZ, G2S_DL>(fq2b_canon(q->z))};
}

// The fold of one run: cnt >= 1 item numbers at lst, their points sig[] affine and canonical (the sort lists only
// decoded signatures, none the identity).  The next point's load is in flight while this one is added, as in
// g1m_fold_records; the last step loads the last point again.
BLS_HD G2Q g2m_fold_records(const G2A* sig, const uint32_t* lst, uint32_t cnt) {
  uint32_t nxt = cnt > 1 ? lst[1] : lst[0];
  G2Q acc;
  {
    const G2A* p = sig + lst[0];
    acc = g2m_from_affine(fq2b_canon(p->x), fq2b_canon(p->y));
  }
  Fp2 nx = sig[nxt].x, ny = sig[nxt].y;
  nxt = cnt > 2 ? lst[2] : nxt;
#pragma unroll 1
  for (uint32_t k = 1; k < cnt; ++k) {
    const Fp2 cx = nx, cy = ny;
    nx = sig[nxt].x;
    ny = sig[nxt].y;
    nxt = k + 2 < cnt ? lst[k + 2] : nxt;
    acc = g2q_add_aff(acc, fq2b_canon(cx), fq2b_canon(cy));
  }
  return acc;
}

// the fold of one bucket's cnt >= 1 run partials
BLS_HD G2Q g2m_fold_partials(const G2SP* prev, uint32_t cnt) {
  G2Q acc = g2m_from_partial(prev);
#pragma unroll 1
  for (uint32_t k = 1; k < cnt; ++k) acc = g2q_add_mem(acc, prev + k);
  return acc;
}

// a bucket's sum where k_msm_usum reads it: six canonical packed Fp (X, Y, Z)
BLS_HD void g2m_store_sum(Fp* o, const G2Q& acc) {
  const Fp2 x = fq2b_pack(acc.x), y = fq2b_pack(acc.y), z = fq2b_pack(acc.z);
  o[0] = x.c0, o[1] = x.c1, o[2] = y.c0, o[3] = y.c1, o[4] = z.c0, o[5] = z.c1;
}
// ... and the identity (0 : 1 : 0) of a bucket without entries
BLS_HD void g2m_store_identity(Fp* o) {
  const Fp2 one = fp2_one();
  o[0] = fp_zero(), o[1] = fp_zero(), o[2] = one.c0, o[3] = one.c1, o[4] = fp_zero(), o[5] = fp_zero();
}
// a run's sum: the bucket's sum at `sum` when the bucket has this run alone (final), else the partial *part for the
// bucket's second fold.  One packing and one set of stores for both, chosen by a select -- a branch would run the
// packing's six products twice in a wave that holds both kinds of run -- which is why the six Fp go through one
// pointer: a G2SP begins with the same six Fp (asserted below).  The partial's flags word is NOT written: g2q_add_mem
// never reads it, but seg2_fold_partials does, so these partials are not input for it.
BLS_HD void g2m_store_run(G2SP* part, Fp* sum, bool final, const G2Q& acc) {
  static_assert(offsetof(G2SP, x) == 0 && offsetof(G2SP, y) == 2 * sizeof(Fp) && offsetof(G2SP, z) == 4 * sizeof(Fp),
                "a partial begins with X, Y, Z as six packed Fp");
  g2m_store_sum(final ? sum : &part->x.c0, acc);
}

}  // namespace bls
