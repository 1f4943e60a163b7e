// Segmented G2 sum of grouped signature aggregation (bls_aggregate_grouped): sum[g] = sum of the included members
// sigma_i with group_id[i] == g.  The plan is the G1 one unchanged (seg_plan / SegRun / SEG_K of bls_g1_segsum.h,
// a group id being its msg_id): one lane folds one run of at most SEG_K entries, the next level folds each group's
// run partials, until every group has one partial.  This header is the per-lane fold that k_g2_seg_fold
// (bls_segsum.hip) and the host check (tests/hostcheck_g2segsum, with BLS_FQ_CHECK) both run.
//
// Additions are the complete projective ones (Renes-Costello-Batina alg. 7 / 8 for a = 0) on
// E2: y^2 = x^3 + 4(1 + i), b3 = 12(1 + i).  Complete means no exceptional case on a curve without a rational point
// of order 2, and #E2(Fp2) = h2 r is odd (the host check asserts the parity of h2): a duplicated signature is a
// doubling, sigma and -sigma give (0 : Y : 0), the identity enters as (0 : 1 : 0), and with subgroup_check = 0 the
// operands may lie anywhere on E2(Fp2).  The Jacobian j2q_add of bls_fq_g2.h is incomplete and is not used here.
//
// Digit form and bounds.  Every value is a bound-typed Fq2B<V, D> of bls_fqb.h (value < V p, digits 0..12 <= D), so
// each subtraction constant, each product's p R limit and each product-scanning column are static_asserts of this
// header: it compiles only if the bounds below close.  In units of p, with M = 2^29 - 1 (an exact digit):
//   accumulator (loop-carried, declared):  X < G2S_VX = 70, Y, Z < G2S_VYZ = 4, digits <= G2S_DL = M + 64
//   operand: canonical, < 1, digits <= M -- an affine member (level 0) or an unpacked stored partial (above)
//   t0, t1, t2 = X x2, Y y2, Z z2                         products, N form: < 2, digits <= M
//   t3 = (X + Y)(x2 + y2) - (t0 + t1)                     N + K(4, 2M) - ..., normalised: < 2 + c, digits <= M + 7
//   t4, and the mixed form's y2 Z + Y                     the same / < 2 + 4
//   y3 = b3 (xz cross term) = 12 xi(.)                    xi(a) = (a0 + K - a1, a0 + a1); 12 x in one carry-save pass
//   t2' = b3 t2 (or b3 Z), t0' = 3 t0                     L form again
//   z3 = t1 + t2', t1' = t1 + K - t2'                     normalised before they meet a product
//   X3 = t3 t1' + K(2, M) - t4 y3 < 2 + 64 + ..; Y3 = t1' z3 + y3 t0' < 4; Z3 = z3 t4 + t0' t3 < 4, normalised
// Every product is Fq2B's operator* (two fq_mul_dot2, the negated b1 from k_for): it checks V1 V2 + V1 K <= R / p
// = 41,291,124 and the 64-bit columns for the operands' digit bounds; the largest operand here is y3 (< 2,500).
// The host check runs the same code with the run-time 128-bit column, value and subtraction checks of bls_fq.h.
#pragma once
#include "bls_g1_segsum.h"
#include "bls_curve.h"
#include "bls_fq_g2.h"
#include "bls_fqb.h"

namespace bls {

constexpr uint64_t G2S_DL = fqb_detail::MASK + 64;
constexpr uint64_t G2S_VX = 70, G2S_VYZ = 4;
typedef Fq2B<G2S_VX, G2S_DL> G2SX;
typedef Fq2B<G2S_VYZ, G2S_DL> G2SYZ;
typedef Fq2B<1, fqb_detail::MASK> Fq2C;  // canonical

// projective accumulator (x = X / Z, y = Y / Z; identity (0 : 1 : 0))
struct G2Q {
  G2SX x;
  G2SYZ y, z;
};

// flags that travel with a partial: a group is ok when it has an included member and none of them is bad
constexpr uint32_t G2S_BAD = 1;   // an included member failed to decode (or, checked, is outside G2)
constexpr uint32_t G2S_SOME = 2;  // at least one included member

// a stored partial or a group's sum: canonical packed coordinates and the flags word beside them
struct G2SP {
  Fp2 x, y, z;
  uint32_t flags;
};

BLS_HD G2Q g2q_identity() {
  return G2Q{fq2b_zero<G2S_VX, G2S_DL>(), relax<G2S_VYZ, G2S_DL>(fq2b_canon(fp2_one())), fq2b_zero<G2S_VYZ, G2S_DL>()};
}

// b3 a = 12 (1 + i) a, L form
template <uint64_t V, uint64_t D>
BLS_HD auto g2s_b3(const Fq2B<V, D>& a) {
  return small<12>(xi(a));
}

// the second half of both additions (RCB alg. 7 steps 21-..): t0, t1 products; t2b = b3 t2; t3, t4 normalised cross
// terms; y3 = b3 (x z cross term)
template <class T0, class T2B, class T3, class T4, class Y3>
BLS_HD G2Q g2q_finish(const T0& t0, const T0& t1, const T2B& t2b, const T3& t3, const T4& t4, const Y3& y3) {
  const auto t0p = small<3>(t0);        // < 6
  const auto z3 = norm(t1 + t2b);
  const auto t1p = norm(t1 - t2b);
  const auto a = t3 * t1p;
  FQ_SEQ();
  const auto b = t4 * y3;
  FQ_SEQ();
  G2Q r;
  r.x = relax<G2S_VX, G2S_DL>(norm(a - b));
  const auto c = t1p * z3;
  FQ_SEQ();
  const auto d = y3 * t0p;
  FQ_SEQ();
  r.y = relax<G2S_VYZ, G2S_DL>(norm(c + d));
  const auto e = z3 * t4;
  FQ_SEQ();
  const auto g = t0p * t3;
  FQ_SEQ();
  r.z = relax<G2S_VYZ, G2S_DL>(norm(e + g));
  return r;
}

// p + (x2, y2), (x2, y2) an affine point of E2 (not the identity), canonical: RCB alg. 8
BLS_HD G2Q g2q_add_aff(const G2Q& p, const Fq2C& x2, const Fq2C& y2) {
  const auto t0 = p.x * x2;
  FQ_SEQ();
  const auto t1 = p.y * y2;
  FQ_SEQ();
  const auto t3 = norm(norm(p.x + p.y) * norm(x2 + y2) - (t0 + t1));
  FQ_SEQ();
  const auto t4 = norm(y2 * p.z + p.y);
  FQ_SEQ();
  const auto y3 = g2s_b3(norm(x2 * p.z + p.x));
  FQ_SEQ();
  return g2q_finish(t0, t1, g2s_b3(p.z), t3, t4, y3);
}

// g2q_add(p, *q) with q a stored partial: RCB alg. 7, ordered so that each of its three cross terms reads the two
// coordinates of q it needs again instead of holding all of q (84 registers) across the formula (seg_reread, as
// g1q_add_mem)
BLS_HD const G2SP* seg2_reread(const G2SP* q) {
#ifdef __HIP_DEVICE_COMPILE__
  asm volatile("" : "+v"(q));
#endif
  return q;
}
BLS_HD G2Q g2q_add_mem(const G2Q& p, const G2SP* q) {
  typedef Fq2B<2, fqb_detail::MASK> N2;
  N2 t0, t1, t2;
  {
    const Fq2C qx = fq2b_canon(q->x), qy = fq2b_canon(q->y);
    t0 = p.x * qx;
    FQ_SEQ();
    t1 = p.y * qy;
    FQ_SEQ();
  }
  q = seg2_reread(q);
  const auto t3 = [&] {
    const Fq2C qx = fq2b_canon(q->x), qy = fq2b_canon(q->y);
    return norm(norm(p.x + p.y) * norm(qx + qy) - (t0 + t1));
  }();
  FQ_SEQ();
  q = seg2_reread(q);
  {
    const Fq2C qz = fq2b_canon(q->z);
    t2 = p.z * qz;
    FQ_SEQ();
  }
  q = seg2_reread(q);
  const auto t4 = [&] {
    const Fq2C qy = fq2b_canon(q->y), qz = fq2b_canon(q->z);
    return norm(norm(p.y + p.z) * norm(qy + qz) - (t1 + t2));
  }();
  FQ_SEQ();
  q = seg2_reread(q);
  const auto y3 = [&] {
    const Fq2C qx = fq2b_canon(q->x), qz = fq2b_canon(q->z);
    return g2s_b3(norm(norm(p.x + p.z) * norm(qx + qz) - (t0 + t2)));
  }();
  FQ_SEQ();
  return g2q_finish(t0, t1, g2s_b3(t2), t3, t4, y3);
}

// level 0: one run of members.  An item outside the mask is skipped unread; an included member that failed its
// decode (ok 0) marks the run bad; the identity (.inf) is a member and adds nothing.
BLS_HD G2Q seg2_fold_items(const SegRun& r, const uint32_t* items, const int* ok, const uint8_t* include,
                           const G2A* a, uint32_t& flags) {
  G2Q acc = g2q_identity();
  flags = 0;
#pragma unroll 1
  for (uint32_t k = 0; k < r.cnt; ++k) {
    const uint32_t i = items[r.src + k];
    if (include && !include[i]) continue;
    flags |= G2S_SOME;
    if (!ok[i]) {
      flags |= G2S_BAD;
      continue;
    }
    const G2A& m = a[i];
    if (m.inf) continue;
    acc = g2q_add_aff(acc, fq2b_canon(m.x), fq2b_canon(m.y));
  }
  return acc;
}

BLS_HD G2Q seg2_fold_partials(const SegRun& r, const G2SP* prev, uint32_t& flags) {
  G2Q acc = g2q_identity();
  flags = 0;
#pragma unroll 1
  for (uint32_t k = 0; k < r.cnt; ++k) {
    const G2SP* q = prev + r.src + k;
    flags |= q->flags;
    acc = g2q_add_mem(acc, q);
  }
  return acc;
}

// canonical projective result with its flags: a group's sum, or a partial for the next level
BLS_HD void seg2_store(const SegRun& r, const G2Q& acc, uint32_t flags, G2SP* tmp, G2SP* gsum) {
  G2SP* o = (r.dst & SEG_FINAL) ? gsum + (r.dst & ~SEG_FINAL) : tmp + r.dst;
  o->x = fq2b_pack(acc.x);
  o->y = fq2b_pack(acc.y);
  o->z = fq2b_pack(acc.z);
  o->flags = flags;
}

}  // namespace bls
