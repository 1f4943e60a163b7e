// Deneb blob KZG on F_r (specs/deneb/polynomial-commitments.md): the per-lane and per-workgroup pieces of the blob
// kernels (bls_kzg.hip), which the kernels and the host check (tests/hostcheck_fr) both run, lane by lane.
//
// A blob is a polynomial p of degree < 4,096 in evaluation form over the domain w_i = omega^brp(i) (brp: the 12-bit
// reversal; the spec's roots_of_unity_brp), f_i = p(w_i).  One workgroup of KZB_LANES lanes works on one blob; lane t
// owns the run of KZB_RUN consecutive elements i = KZB_RUN t + k.
//
//   evaluation  p(z) = (z^4096 - 1) / 4096 * sum_i f_i w_i / (z - w_i)   for z outside the domain, and f_m for
//               z = w_m.  A lane inverts its 16 denominators with one fr_inv (Montgomery's trick; the denominators
//               are formed again on the way back instead of being kept), a zero denominator is replaced by 1 and its
//               index recorded (`hit`); the lane sums are added by the workgroup and kzb_eval_finish selects f_hit or
//               scales the sum.  The 16 prefix products of a lane go to a scratch array in memory (32 B x 4,096 per
//               blob, slot k * 256 + lane), not to registers: kept in registers the two loops have to be unrolled
//               16 times, and the compiler then schedules that one block of ~80 products for parallelism, not for
//               register pressure (2.3 KiB of spills per lane at 256 VGPRs, 0.8 KiB at 512).  Rolled,
//               the kernels take ~100 VGPRs, no private segment, and compile in seconds; the 32 extra memory
//               accesses per lane are small beside the inversion's ~385 products.
//   quotient    q_i = (f_i - y) / (w_i - z), the evaluation form of (p(X) - y) / (X - z).  For z = w_m every i != m
//               is that formula and q_m = sum_{i != m} (f_i - y) w_i / (z (z - w_i)) = -(1 / z) sum_{i != m} q_i w_i,
//               so the lanes also sum q_i w_i when the evaluation reported a hit, and kzb_quot_finish writes q_m.
//               The q_i are written as 32-byte big-endian integers: rows the table MSM reads as they are.
#pragma once
#include "bls_fr.h"

namespace bls {

constexpr uint32_t KZB_N = 4096;     // FIELD_ELEMENTS_PER_BLOB
constexpr uint32_t KZB_LANES = 256;  // lanes of a blob's workgroup
constexpr uint32_t KZB_RUN = 16;     // consecutive elements per lane
static_assert(KZB_LANES * KZB_RUN == KZB_N, "a workgroup covers a blob");

// the 12-bit reversal
BLS_HD uint32_t kzb_brp12(uint32_t i) {
  i = ((i & 0x5555u) << 1) | ((i >> 1) & 0x5555u);  // the 16-bit reversal of i < 4,096 ...
  i = ((i & 0x3333u) << 2) | ((i >> 2) & 0x3333u);
  i = ((i & 0x0f0fu) << 4) | ((i >> 4) & 0x0f0fu);
  i = ((i & 0xffu) << 8) | ((i >> 8) & 0xffu);
  return i >> 4;  // ... whose low four bits are zero
}

// entry i of the domain table: omega^brp(i) in Montgomery form
BLS_HD Fr kzb_domain_entry(uint32_t i) { return fr_pow_u32(fr_omega(), kzb_brp12(i)); }

// where lane `lane` keeps the prefix product of its step k among the blob's 4,096 slots: the lanes of a wavefront
// touch consecutive slots
BLS_HD uint32_t kzb_pre_slot(uint32_t lane, uint32_t k) { return k * KZB_LANES + lane; }

struct KzbLane {
  Fr sum;
  int hit;  // the element whose denominator vanished, or -1
};

// z - w, or 1 where that is zero
BLS_HD Fr kzb_denominator(const Fr& z, const Fr& w, bool& zero) {
  const Fr d = fr_sub(z, w);
  zero = fr_is_zero(d);
  return zero ? fr_one() : d;
}

// lane `lane` of the evaluation of the blob f (4,096 Montgomery elements) at z: sum over the lane's run of
// f_i w_i / (z - w_i), the vanishing denominator taken as 1.  pre: the blob's 4,096 prefix-product slots
BLS_HD KzbLane kzb_eval_lane(const Fr* dom, const Fr* f, const Fr& z, uint32_t lane, Fr* pre) {
  const uint32_t i0 = KZB_RUN * lane;
  Fr acc = fr_one();
  int hit = -1;
#pragma unroll 1
  for (uint32_t k = 0; k < KZB_RUN; ++k) {
    bool zero;
    const Fr d = kzb_denominator(z, dom[i0 + k], zero);
    if (zero) hit = (int)(i0 + k);
    pre[kzb_pre_slot(lane, k)] = acc;  // the product of the denominators before k
    acc = fr_mul(acc, d);
  }
  Fr inv = fr_inv(acc);
  Fr sum = fr_zero();
#pragma unroll 1
  for (int k = KZB_RUN - 1; k >= 0; --k) {
    const Fr w = dom[i0 + k];
    bool zero;
    const Fr d = kzb_denominator(z, w, zero);
    const Fr dinv = fr_mul(inv, pre[kzb_pre_slot(lane, k)]);
    inv = fr_mul(inv, d);
    sum = fr_add(sum, fr_mul(fr_mul(f[i0 + k], w), dinv));
  }
  return KzbLane{sum, hit};
}

// p(z) from the sum of the lanes' sums: f_hit for z in the domain, else sum (z^4096 - 1) / 4096
BLS_HD Fr kzb_eval_finish(const Fr& total, const Fr& z, const Fr* f, int hit) {
  if (hit >= 0) return f[hit];
  Fr zn = z;
#pragma unroll 1
  for (int s = 0; s < 12; ++s) zn = fr_sqr(zn);
  return fr_mul(fr_mul(total, fr_sub(zn, fr_one())), fr_inv_4096());
}

// lane `lane` of the quotient of the blob f by (X - z), y = p(z), hit = the evaluation's: writes the run's q_i to
// q32 (the blob's row of 4,096 32-byte big-endian scalars; zero at i = hit) and returns the run's sum of q_i w_i over
// i != hit (zero without a hit: nothing reads it).  pre: the blob's 4,096 prefix-product slots
BLS_HD Fr kzb_quot_lane(const Fr* dom, const Fr* f, const Fr& z, const Fr& y, int hit, uint32_t lane, uint8_t* q32,
                        Fr* pre) {
  const uint32_t i0 = KZB_RUN * lane;
  Fr acc = fr_one();
#pragma unroll 1
  for (uint32_t k = 0; k < KZB_RUN; ++k) {
    bool zero;
    const Fr d = kzb_denominator(dom[i0 + k], z, zero);
    pre[kzb_pre_slot(lane, k)] = acc;
    acc = fr_mul(acc, d);
  }
  Fr inv = fr_inv(acc);
  Fr sum = fr_zero();
#pragma unroll 1
  for (int k = KZB_RUN - 1; k >= 0; --k) {
    const Fr w = dom[i0 + k];
    bool zero;
    const Fr d = kzb_denominator(w, z, zero);
    const Fr dinv = fr_mul(inv, pre[kzb_pre_slot(lane, k)]);
    inv = fr_mul(inv, d);
    Fr q = fr_mul(fr_sub(f[i0 + k], y), dinv);
    if (zero) q = fr_zero();
    if (hit >= 0) sum = fr_add(sum, fr_mul(q, w));
    fr_to_be32(q, q32 + 32 * (i0 + k));
  }
  return sum;
}

// q_hit = -total / z from the sum of the lanes' sums (z = w_hit is not zero)
BLS_HD void kzb_quot_finish(const Fr& total, const Fr& z, int hit, uint8_t* q32) {
  fr_to_be32(fr_neg(fr_mul(total, fr_inv(z))), q32 + 32 * (uint32_t)hit);
}

}  // namespace bls
