// Two-dimensional G1 scalar multiplication through the endomorphism phi(x, y) = (beta x, y) = [lambda](x, y),
// lambda = -x^2 mod r (x the curve parameter; bls_curve.h g1_in_subgroup relies on the same beta = FP_BETA), in
// the redundant digit form of bls_fq.h with the complete formulas of bls_fq_g1.h.
//
// The batch's 64-bit RLC scalar is read as r_i = a + b lambda (a its low, b its high 32 bits), so
// r_i A = a A + b phi(A) is one joint 32-step double-and-add (Straus / Shamir) in place of a 63-step chain.  The
// three table points cost two products:
//   A = (X : Y : Z),  phi(A) = (beta X : Y : Z),  A + phi(A) = -phi^2(A) = (beta^2 X : -Y : Z)
// (1 + lambda + lambda^2 = 0).  The other side of the pairing equation takes its bits 32 .. 63 from phi(-G1)
// (bls_bisect.hip k_neg_g1_comb_table), so both sides weigh bit 32 + j by 2^j lambda.
#pragma once
#include "bls_fq_g1.h"

namespace bls {

// a A + b phi(A).  A: N- or L-form coordinates (digits <= 2^29 + 2^4) with values below 4p, any point of the curve
// including the identity (complete formulas, no exceptional case).  Bounds of the table operand T of g1q_add
// (its first operand is always a g1q_dbl output: X < 4p with digits <= 2^29, Y, Z in N form):
//   T.x in {X, beta X, beta^2 X}: products are N form, < 2p;  T.z = Z;
//   T.y in {Y, -Y}, -Y = 64p - Y digit-wise (fq_sub from zero: Q29_K1's digits are >= any N/L digit), normalised
//   to L form (digits <= 2^29 + 1), value <= 64p.
// Then every product of g1q_add stays far below p R (R / p ~ 2^25.3): the largest is
// (p.x + p.y)(T.x + T.y) < 8p x 66p, and (p.y + p.z)(T.y + T.z) < 6p x 68p; operand digits are <= 2^30 + 2^5 on
// both sides (sums of two L forms), inside fq_mul's column bound; g1q_add proves all of this at compile time for
// any operand coordinate below 66p.  Its outputs are in N form (< 2p), which g1q_dbl takes.  The digit is chosen by
// selects and the addition is always computed: in a 64-lane wave some lane has a non-zero digit at every step.
BLS_HD G1Q g1q_mul_endo(const G1Q& A, uint32_t a, uint32_t b) {
  const Fq beta = fq_unpack(FP_BETA);
  const Fq x1 = fq_mul(A.x, beta);
  const Fq x2 = fq_mul(x1, beta);
  const Fq yn = fq_norm(fq_sub(fq_zero(), A.y));
  G1Q R{fq_zero(), fq_unpack(FP_ONE), fq_zero()};
#pragma unroll 1
  for (int i = 31; i >= 0; --i) {
    R = g1q_dbl(R);
    const uint32_t d = ((a >> i) & 1u) | (((b >> i) & 1u) << 1);
    const G1Q T{fq_select(d == 3u, x2, fq_select(d == 2u, x1, A.x)), fq_select(d == 3u, yn, A.y), A.z};
    const G1Q S = g1q_add(R, T);
    R = G1Q{fq_select(d != 0u, S.x, R.x), fq_select(d != 0u, S.y, R.y), fq_select(d != 0u, S.z, R.z)};
  }
  return R;
}

}  // namespace bls
