// Bucket MSM over a call's own G1 points (bls_g1_msm; kernels in bls_g1_table.hip): the per-lane pieces that the
// resident table's MSM (bls_g1_msm.h) does not have, which the kernels and the host check (tests/hostcheck_g1vmsm,
// with BLS_FQ_CHECK) both run.
//
// The call's n points become n single-window RegKey records; there are no window multiples.  The non-zero digit d of
// window w of row v's scalar k_{v,i} goes to bucket slot (v * 32 + w) * 256 + d as record number i, so the table
// MSM's folds, bit sums and Horner (bls_g1_msm.h), run over 32 B slot groups instead of B, leave one window sum
// W_{v,w} = sum_i [d_w(k_{v,i})] P_i per (row, window).  The row's result is sum_w 2^(8w) W_{v,w}, which the table
// form gets from its precomputed multiples and this form from one doubling chain per ROW (not per point).
//
// Bounds (bls_fq_g1.h's accumulator contract), the argument of g1m_horner and g1m_window_step:
//   window chain   starts from an unpacked canonical window sum (N form); then eight g1q_dbl, whose outputs
//                  (X3 < 4p with digits <= 2^29, Y3, Z3 in N form) are inputs of g1q_dbl and of g1q_add again, and
//                  one g1q_add of the chain with an unpacked canonical window sum, whose N-form output is an input of
//                  g1q_dbl.  Every operand stays inside g1q_dbl's / g1q_add's "any coordinate below 66p".
#pragma once
#include "bls_g1_msm.h"

namespace bls {

// the bucket slot of digit d of window w of row v
BLS_HD uint32_t g1vm_slot(uint32_t v, int w, uint32_t d) { return (v * G1M_WINDOWS + (uint32_t)w) * G1M_SLOTS + d; }

// The sort's lane of (row v, one scalar): f(slot) for every non-zero digit, windows in ascending order.
template <class F>
BLS_HD void g1vm_each_slot(const uint32_t k[8], uint32_t v, F&& f) {
#pragma unroll 1
  for (int w = 0; w < G1M_WINDOWS; ++w) {
    const uint32_t d = g1m_digit(k, w);
    if (d) f(g1vm_slot(v, w, d));
  }
}

// the highest window of a row whose sum is not the identity (canonical Z != 0), 0 if there is none
BLS_HD int g1vm_top_window(const G1P* W) {
  int w = G1M_WINDOWS - 1;
  while (w > 0 && fp_is_zero(W[w].z)) --w;
  return w;
}

// sum_w 2^(8w) W[w] over a row's 32 canonical window sums by Horner from the row's top window: a row of 128-bit
// scalars pays 120 doublings, not 248.  The identity (0 : 1 : 0) as a window sum passes through the complete
// addition; a row of identities returns W[0].
BLS_HD G1Q g1vm_combine(const G1P* W) {
  int w = g1vm_top_window(W);
  G1Q r = g1m_unpack(W[w]);
#pragma unroll 1
  for (--w; w >= 0; --w) {
#pragma unroll 1
    for (int i = 0; i < 8; ++i) r = g1q_dbl(r);
    r = g1q_add(r, g1m_unpack(W[w]));
  }
  return r;
}

}  // namespace bls
