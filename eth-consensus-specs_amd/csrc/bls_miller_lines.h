// G2 side of the split Miller loop (k_miller_lines2 in bls_miller_lane.hip, and the line waves of k_miller_fused
// in bls_miller_pair.hip): T's doubling / addition steps and the P-independent parts of the line coefficients,
// each step's line record written to L (word w at L[w * n]).
//
// T = (X, Y, Z) is in HOMOGENEOUS projective coordinates (x = X / Z, y = Y / Z) on y^2 = x^3 + b', b' = 4 xi, so
// the three line coefficients fall out of the step with no rescaling (Costello-Lange-Naehrig):
//   doubling   J = X^2, B = Y^2, C = Z^2, S = (Y + Z)^2      E = 3 b' C = 12 xi C, F = 3 E, H = S - B - C = 2 Y Z
//              X3 = 2 (X Y)(B - F),  Y3 = (B + F)^2 - 12 E^2,  Z3 = 4 B H      (4 x the textbook form: no halvings)
//              line (l0, l2, l3) = (B - E, 3 J, H) = Z^2 (y^2 - 3 b', 3 x^2, 2 y)
//   addition   theta = Y - y_Q Z, lambda = X - x_Q Z, C = theta^2, D = lambda^2, E = lambda D, F = Z C, G = X D,
//   (Q affine) H = E + F - 2 G;  X3 = lambda H,  Y3 = theta (G - H) - E Y,  Z3 = Z E
//              line (l0, l2, l3) = (theta x_Q - lambda y_Q, theta, lambda)
// The line at P is l0 + l2 (-x_P) v + l3 y_P v w: the tangent 2y y_P - 3x^2 x_P + (y^2 - 3b') resp. the chord
// lambda (y_P - y_Q) - theta (x_P - x_Q), times a non-zero Fp2 element that the final exponentiation removes.
// A doubling is 6 squarings + 3 products in Fp2 (the Jacobian step it replaced: 7 + 4, two of the products only
// rescaling the line), an addition 2 + 11.
//
// The formulas are written once (ln_* below, host and device) and called by both layouts:
//   Line2   TWO lanes per pair.  A doubling runs five product slots, the lanes 2k / 2k+1 taking one operand
//           pair each and exchanging results by DPP:
//             squarings   lane 0: J, B, (B + F)^2          lane 1: C, S, E^2
//             products    lane 0: X Y                      lane 1: B H
//             X Y (B - F) lane 0: its real part            lane 1: its imaginary part (one dot product each)
//           An addition runs six slots and one split product in the same way (Line2::add).
//   Line1   ONE lane per pair (k_miller_fused<2>'s line wave): every product on the lane.
// T stays in the bound-typed digit form for the whole loop (declared Fq2B<LN_TV, LN_TD>; every step is relaxed to
// it, so its bounds are checked by induction at compile time): no product unpacks or repacks, additions are
// digit-wise.
//
// Exceptional inputs.  The steps are straight-line arithmetic and never branch on T.  T = O (Z = 0) stays O: a
// doubling gives Z3 = 4 B H = 0, an addition Z3 = Z E = 0.  T = Q in an addition gives theta = lambda = 0, T = -Q
// lambda = 0: the record is (0, 0, 0) resp. (theta x_Q, theta, 0) and T becomes O (Z3 = Z lambda^3 = 0).  Neither
// occurs for Q of order r: the loop's running multiples [k] Q, 1 <= k <= |x| < r, are never O or +-Q when an
// addition meets them.  For Q outside G2 the result is some well-defined Fp12 value of no meaning; the callers
// decide membership separately.
#pragma once
#include "bls_fqb.h"
#include "bls_kernels.h"

namespace bls {
namespace mlines {

// products one after another (interleaved, their digit columns spilled ~140 VGPRs); nothing to order on the host
#if defined(__HIP_DEVICE_COMPILE__)
#define LN_SEQ() __builtin_amdgcn_sched_barrier(0)
#else
#define LN_SEQ() ((void)0)
#endif
constexpr uint64_t LN_TV = 1024, LN_TD = 0x20000000ull + 64;  // loop-carried bound of T's coordinates
using TF = Fq2B<LN_TV, LN_TD>;
using QF = Fq2B<1, fqb_detail::MASK>;
using LF = Fq2B<ML_LV, ML_LD>;  // a record word

// ---- the step formulas (host and device) ----------------------------------------------------------------------
// doubling, from the squarings B = Y^2, C = Z^2, S = (Y + Z)^2, J = X^2.  Bounds in units of p: a square is < 4,
// xi C < 9, so E < 108, F < 324, B + F < 328, B - F < 329, B - E < 113 and Y3 < 53 -- far inside the products'
// operand limit (V1 V2 <= R / p ~ 2^25.3), the record's ML_LV and T's declared LN_TV.
template <class TC>
BLS_HD auto ln_E(const TC& C) {  // E = 3 b' C = 12 xi C
  return small<12>(xi(C));
}
template <class TS, class TB, class TC>
BLS_HD auto ln_H(const TS& S, const TB& B, const TC& C) {  // H = 2 Y Z: the line's l3, and Z3 = 4 B H
  return norm(S - (B + C));
}
template <class TB, class TE>
BLS_HD auto ln_l0(const TB& B, const TE& E) {  // l0 = B - E = Z^2 (y^2 - 3 b')
  return norm(B - E);
}
template <class TJ>
BLS_HD auto ln_l2(const TJ& J) {  // l2 = 3 J = Z^2 3 x^2
  return small<3>(J);
}
template <class TB, class TE>
BLS_HD auto ln_BpF(const TB& B, const TE& E) {
  return norm(B + small<3>(E));
}
template <class TB, class TE>
BLS_HD auto ln_BmF(const TB& B, const TE& E) {
  return norm(B - small<3>(E));
}
// T = 2T from the step's products: XF = X Y (B - F), G2 = (B + F)^2, E2 = E^2, BH = B H
template <class T1, class T2, class T3, class T4>
BLS_HD void ln_dbl_out(TF& X, TF& Y, TF& Z, const T1& XF, const T2& G2, const T3& E2, const T4& BH) {
  X = relax<LN_TV, LN_TD>(small<2>(XF));
  Y = relax<LN_TV, LN_TD>(norm(G2 - small<12>(E2)));
  Z = relax<LN_TV, LN_TD>(small<4>(BH));
}

// the whole doubling on one lane: T = 2T; emit(l0, l2, l3) takes the record's words as soon as they exist (held
// to the end of the step they would cost 84 registers through its five remaining products)
template <class Emit>
BLS_HD void ln_dbl(TF& X, TF& Y, TF& Z, Emit&& emit) {
  const auto J = sqr(X);
  LN_SEQ();
  const auto B = sqr(Y);
  LN_SEQ();
  const auto C = sqr(Z);
  LN_SEQ();
  const auto S = sqr(norm(Y + Z));
  LN_SEQ();
  const auto E = ln_E(C);
  const auto H = ln_H(S, B, C);
  emit(relax<ML_LV, ML_LD>(ln_l0(B, E)), relax<ML_LV, ML_LD>(ln_l2(J)), relax<ML_LV, ML_LD>(H));
  LN_SEQ();
  const auto XY = X * Y;
  LN_SEQ();
  const auto XF = XY * ln_BmF(B, E);
  LN_SEQ();
  const auto G2 = sqr(ln_BpF(B, E));
  LN_SEQ();
  const auto E2 = sqr(E);
  LN_SEQ();
  const auto BH = B * H;
  LN_SEQ();
  ln_dbl_out(X, Y, Z, XF, G2, E2, BH);
}

// the addition's sums: theta = Y - y_Q Z (lambda = X - x_Q Z), H = E + F - 2 G, and differences of two products
template <class TY, class TP>
BLS_HD auto ln_diff(const TY& a, const TP& b) {
  return norm(a - b);
}
template <class TE, class TF_, class TG>
BLS_HD auto ln_add_H(const TE& E, const TF_& F, const TG& G) {
  return norm((E + F) - small<2>(G));
}

// the mixed addition T = T + Q (Q affine), the record (theta x_Q - lambda y_Q, theta, lambda) in l0, l2, l3
BLS_HD void ln_add(TF& X, TF& Y, TF& Z, const QF& qx, const QF& qy, LF& l0, LF& l2, LF& l3) {
  const auto yz = qy * Z;
  LN_SEQ();
  const auto xz = qx * Z;
  LN_SEQ();
  const auto th = ln_diff(Y, yz);
  const auto lm = ln_diff(X, xz);
  const auto C = sqr(th);
  LN_SEQ();
  const auto D = sqr(lm);
  LN_SEQ();
  const auto E = lm * D;
  LN_SEQ();
  const auto F = Z * C;
  LN_SEQ();
  const auto G = X * D;
  LN_SEQ();
  const auto H = ln_add_H(E, F, G);
  const auto x3 = lm * H;
  LN_SEQ();
  const auto y3 = ln_diff(th * ln_diff(G, H), E * Y);
  LN_SEQ();
  const auto z3 = Z * E;
  LN_SEQ();
  l0 = relax<ML_LV, ML_LD>(ln_diff(th * qx, lm * qy));
  LN_SEQ();
  l2 = relax<ML_LV, ML_LD>(th);
  l3 = relax<ML_LV, ML_LD>(lm);
  X = relax<LN_TV, LN_TD>(x3);
  Y = relax<LN_TV, LN_TD>(y3);
  Z = relax<LN_TV, LN_TD>(z3);
}

// ---- the kernels' side ----------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t dpp_bc(uint32_t v, bool odd) {  // lane 2k's value (odd = false) or lane 2k+1's
  return odd ? (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xF5, 0xF, 0xF, false)   // quad_perm [1,1,3,3]
             : (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xA0, 0xF, 0xF, false);  // quad_perm [0,0,2,2]
}
template <bool ODD, uint64_t V, uint64_t D>
__device__ __forceinline__ FqB<V, D> bcq(const FqB<V, D>& a) {
  FqB<V, D> r;
#pragma unroll
  for (int i = 0; i < 14; i++) r.x.d[i] = dpp_bc(a.x.d[i], ODD);
  return r;
}
template <bool ODD, uint64_t V, uint64_t D>
__device__ __forceinline__ Fq2B<V, D> bcp(const Fq2B<V, D>& a) {
  return {bcq<ODD>(a.c0), bcq<ODD>(a.c1)};
}
// a b with the lane pair taking one coefficient each -- lane 0: a0 b0 - a1 b1, lane 1: a0 b1 + a1 b0, one dot
// product per lane (the Fq2B product runs both) -- and both lanes receiving both
template <uint64_t V1, uint64_t D1, uint64_t V2, uint64_t D2>
__device__ __forceinline__ Fq2B<2, fqb_detail::MASK> mul_pair(bool hi, const Fq2B<V1, D1>& a, const Fq2B<V2, D2>& b) {
  const auto nb = norm(neg(b.c1));
  const FqN c = dot2(a.c0, sel(hi, b.c1, b.c0), a.c1, sel(hi, b.c0, nb));
  return {bcq<false>(c), bcq<true>(c)};
}
__device__ __forceinline__ void ml_store_q(uint32_t* L, size_t n, int w0, const LF& a) {
  uint32_t* const Lw = L + (size_t)w0 * n;  // a per-lane row base, so the row offsets are uniform
#pragma unroll
  for (int j = 0; j < 14; ++j) {
    Lw[(size_t)j * n] = a.c0.x.d[j];
    Lw[(size_t)(14 + j) * n] = a.c1.x.d[j];
  }
}
// Q's affine coordinates wait in qlds ([word][lane], 56 x 64 words) for the five addition steps (held in
// registers across the 63 doublings they pushed the kernel into spills)
__device__ __forceinline__ void q_park(const QF& qx, const QF& qy, uint32_t* qlds, int lane) {
  const uint32_t* w = reinterpret_cast<const uint32_t*>(&qx);
  const uint32_t* w2 = reinterpret_cast<const uint32_t*>(&qy);
#pragma unroll
  for (int k = 0; k < 28; k++) {
    qlds[k * 64 + lane] = w[k];
    qlds[(28 + k) * 64 + lane] = w2[k];
  }
}
__device__ __forceinline__ void q_fetch(QF& qx, QF& qy, const uint32_t* qlds, int lane) {
  uint32_t* w = reinterpret_cast<uint32_t*>(&qx);
  uint32_t* w2 = reinterpret_cast<uint32_t*>(&qy);
#pragma unroll
  for (int k = 0; k < 28; k++) {
    w[k] = qlds[k * 64 + lane];
    w2[k] = qlds[(28 + k) * 64 + lane];
  }
}

// The line's P factors (k_miller_fused's line waves apply them, so the accumulation reads l0, l2, l3 ready to
// multiply): l2 (-x_P), l3 y_P.  nx = -x_P as K - x_P.
struct PFac {
  FqC y;
  decltype(FqC{} - FqC{}) nx;
  __device__ __forceinline__ void init(const G1A& p) {
    const FqC zero{fq_zero()};
    y = fqb_canon(p.y);
    nx = zero - fqb_canon(p.x);
  }
};
using FqN2 = Fq2B<2, fqb_detail::MASK>;
template <uint64_t V, uint64_t D, uint64_t VS, uint64_t DS>
__device__ __forceinline__ LF scale(const Fq2B<V, D>& a, const FqB<VS, DS>& s) {
  return relax<ML_LV, ML_LD>(FqN2{a.c0 * s, a.c1 * s});
}

// T of one pair on lanes (2k, 2k+1)
// SC: the records carry l2, l3 with their P factors applied (PFac); otherwise (l0, l2, l3) as the formulas give them
template <bool SC = false>
struct Line2 {
  TF X, Y, Z;
  bool hi;
  PFac pf;  // SC only

  __device__ __forceinline__ void init(const G2A& q, bool hi_, uint32_t* qlds, int lane) {
    hi = hi_;
    const QF qx = fq2b_canon(q.x), qy = fq2b_canon(q.y);
    q_park(qx, qy, qlds, lane);
    const FqC one = fqb_canon(FP_ONE), zero{fq_zero()};
    X = relax<LN_TV, LN_TD>(qx);
    Y = relax<LN_TV, LN_TD>(qy);
    Z = relax<LN_TV, LN_TD>(QF{one, zero});
  }

  // doubling step: T = 2T, the record (B - E, 3 J, H) at L
  __device__ __forceinline__ void dbl(uint32_t* L, size_t n) {
    const auto s0 = sqr(sel(hi, Z, X));                          // lane 0: J;  lane 1: C
    LN_SEQ();
    const auto s1 = sqr(sel(hi, norm(Y + Z), Y));                // lane 0: B;  lane 1: S
    LN_SEQ();
    const auto B = bcp<false>(s1);
    const auto C = bcp<true>(s0);
    const auto S = bcp<true>(s1);
    const auto E = ln_E(C);
    const auto H = ln_H(S, B, C);
    // the record: lane 0 holds J (l2), lane 1 stores l0; l3 = H goes with lane 1's P factor y_P in the SC form
    if constexpr (SC) {
      ml_store_q(L, n, hi ? 56 : 28, scale(sel(hi, H, ln_l2(s0)), sel(hi, pf.y, pf.nx)));
      LN_SEQ();
      if (hi) ml_store_q(L, n, 0, relax<ML_LV, ML_LD>(ln_l0(B, E)));
    } else {
      ml_store_q(L, n, hi ? 0 : 28, relax<ML_LV, ML_LD>(sel(hi, ln_l0(B, E), ln_l2(s0))));
      LN_SEQ();
      if (hi) ml_store_q(L, n, 56, relax<ML_LV, ML_LD>(H));
    }
    LN_SEQ();
    const auto r0 = sqr(sel(hi, E, ln_BpF(B, E)));               // lane 0: (B + F)^2;  lane 1: E^2
    LN_SEQ();
    const auto r1 = sel(hi, B, X) * sel(hi, H, Y);               // lane 0: X Y;  lane 1: B H
    LN_SEQ();
    const auto XF = mul_pair(hi, bcp<false>(r1), ln_BmF(B, E));  // X Y (B - F), half on each lane
    LN_SEQ();
    ln_dbl_out(X, Y, Z, XF, bcp<false>(r0), bcp<true>(r0), bcp<true>(r1));
  }

  // addition step (T + Q, Q affine), the record (theta x_Q - lambda y_Q, theta, lambda) at L: six product slots
  // and one split product, each lane one operand pair
  //   lane 0: y_Q Z, theta^2, lambda D, Z C, Z E, lambda H          lane 1: x_Q Z, lambda^2, X D, theta x_Q,
  //   theta (G - H): the lanes one coefficient each                         lambda y_Q, E Y
  __device__ __forceinline__ void add(uint32_t* L, size_t n, const uint32_t* qlds, int lane) {
    QF qx, qy;
    q_fetch(qx, qy, qlds, lane);
    const auto a = sel(hi, qx, qy) * Z;                          // lane 0: y_Q Z;  lane 1: x_Q Z
    LN_SEQ();
    const auto th = ln_diff(Y, bcp<false>(a));
    const auto lm = ln_diff(X, bcp<true>(a));
    const auto b = sqr(sel(hi, lm, th));                         // lane 0: C = theta^2;  lane 1: D = lambda^2
    LN_SEQ();
    const auto c = sel(hi, X, lm) * bcp<true>(b);                // lane 0: E = lambda D;  lane 1: G = X D
    LN_SEQ();
    const auto E = bcp<false>(c);
    const auto d = sel(hi, th, Z) * sel(hi, qx, bcp<false>(b));  // lane 0: F = Z C;  lane 1: theta x_Q
    LN_SEQ();
    const auto e = sel(hi, lm, Z) * sel(hi, qy, E);              // lane 0: Z3 = Z E;  lane 1: lambda y_Q
    LN_SEQ();
    const LF l0 = relax<ML_LV, ML_LD>(ln_diff(d, e));            // lane 1's
    if constexpr (SC) {  // lane 0: l2 = theta (-x_P); lane 1: l0 and l3 = lambda y_P
      ml_store_q(L, n, hi ? 56 : 28, scale(sel(hi, lm, th), sel(hi, pf.y, pf.nx)));
      LN_SEQ();
      if (hi) ml_store_q(L, n, 0, l0);
    } else {
      ml_store_q(L, n, hi ? 0 : 28, sel(hi, l0, relax<ML_LV, ML_LD>(th)));
      LN_SEQ();
      if (hi) ml_store_q(L, n, 56, relax<ML_LV, ML_LD>(lm));
    }
    LN_SEQ();
    const auto G = bcp<true>(c);
    const auto H = ln_add_H(E, bcp<false>(d), G);
    const auto f = sel(hi, E, lm) * sel(hi, Y, H);               // lane 0: X3 = lambda H;  lane 1: E Y
    LN_SEQ();
    const auto g = mul_pair(hi, th, ln_diff(G, H));              // theta (G - H), half on each lane
    LN_SEQ();
    X = relax<LN_TV, LN_TD>(bcp<false>(f));
    Y = relax<LN_TV, LN_TD>(ln_diff(g, bcp<true>(f)));
    Z = relax<LN_TV, LN_TD>(bcp<false>(e));
  }
};

// The same steps with ONE lane per pair (k_miller_fused's line wave: 64 pairs per wave, so one wave keeps up with
// the two f-accumulation waves of a workgroup): every product of the step on the lane, no DPP exchange and no
// selects; the same formulas, bounds and record words as Line2.
template <bool SC = false>
struct Line1 {
  TF X, Y, Z;
  PFac pf;  // SC only

  __device__ __forceinline__ void init(const G2A& q, uint32_t* qlds, int lane) {
    const QF qx = fq2b_canon(q.x), qy = fq2b_canon(q.y);
    q_park(qx, qy, qlds, lane);
    const FqC one = fqb_canon(FP_ONE), zero{fq_zero()};
    X = relax<LN_TV, LN_TD>(qx);
    Y = relax<LN_TV, LN_TD>(qy);
    Z = relax<LN_TV, LN_TD>(QF{one, zero});
  }

  __device__ __forceinline__ void store(uint32_t* L, size_t n, const LF& l0, const LF& l2, const LF& l3) {
    ml_store_q(L, n, 0, l0);
    if constexpr (SC) {
      ml_store_q(L, n, 28, scale(l2, pf.nx));
      LN_SEQ();
      ml_store_q(L, n, 56, scale(l3, pf.y));
    } else {
      ml_store_q(L, n, 28, l2);
      ml_store_q(L, n, 56, l3);
    }
    LN_SEQ();
  }

  __device__ __forceinline__ void dbl(uint32_t* L, size_t n) {
    ln_dbl(X, Y, Z, [&](const LF& l0, const LF& l2, const LF& l3) { store(L, n, l0, l2, l3); });
  }

  __device__ __forceinline__ void add(uint32_t* L, size_t n, const uint32_t* qlds, int lane) {
    QF qx, qy;
    q_fetch(qx, qy, qlds, lane);
    LF l0, l2, l3;
    ln_add(X, Y, Z, qx, qy, l0, l2, l3);
    store(L, n, l0, l2, l3);
  }
};

}  // namespace mlines
}  // namespace bls
