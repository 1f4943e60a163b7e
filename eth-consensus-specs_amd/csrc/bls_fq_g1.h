// Complete projective G1 additions (Renes-Costello-Batina alg. 7 / 8 / 9, a = 0,
// b3 = 12) in the redundant digit form of bls_fq.h, for the registry gather
// (k_fav_gather_q, bls_kernels.hip), the r_i apk_i chain (bls_g1_endo.h) and the
// segmented and workgroup G1 sums; and the sum of two affine points in
// homogeneous coordinates (g1q_add_aff2: 7 digit products, incomplete, x2 != x3),
// which the registry gather forms of every two keys of a lane before one g1q_add.
#pragma once
#include "bls_fqb.h"

namespace bls {

// The accumulator stays in digits between additions (no unpack / repack / final
// subtraction per product), additions and subtractions are digit-wise, and the
// products by 3b = 12 are one pass of 64-bit digit products.
//
// Every output coordinate of the three formulas is a sum or difference of two
// products,
//   X3 = t3 t1' - t4 y3   Y3 = t1' z3 + y3 t0'   Z3 = z3 t4 + t0' t3     (add_aff, add)
//   Y3 = w (t0 + t2) + t2 z8                                            (dbl)
// and each is ONE Montgomery reduction over the shared column sum of both
// products (fq_mul_dot2): 8 / 9 / 7 reductions for the 11 / 12 / 8 digit products
// of a mixed addition / addition / doubling, and no normalisation of the sums.
// The difference is t3 t1' + t4 (K - y3) with K a multiple of p covering y3's
// digits (k_for).
//
// Written in the bound-typed form (bls_fqb.h): every product's value and 28 +
// 14-term columns and every subtraction constant are static_asserts on the
// input contract below, and an operand of a dot product is normalised only
// where the unnormalised one is proved not to fit (a static_assert on
// !dot2_fits for every norm: t3, t4, t0', t1' in the additions, w in the doubling).
//
// Input contract (unchanged): coordinates in L form, digits <= 2^29 + 2^4; an
// accumulator has X < 66p and Y, Z < 4p; either operand of g1q_add may have any
// coordinate up to 66p (bls_g1_endo.h's -Y = 64p - Y); the affine operand of
// g1q_add_aff is in N form (< 2p, 29-bit digits).  Outputs: every coordinate in
// N form except g1q_dbl's X3 = 2 w u (< 4p, digits <= 2^29), so the outputs are
// inputs again and every loop over them closes.
// g1q_add_aff2 takes two affine points in N form and returns N form: an operand
// of g1q_add.
// The host tests (tests/test_hostcheck.py::test_fq_gather_formulas,
// tests/test_g1dot_cpu.py, tests/test_g1pair_cpu.py) run these formulas with the
// 128-bit column checks of bls_fq.h.
struct G1Q {
  Fq x, y, z;
};

namespace g1q_detail {
constexpr uint64_t LD = fqb_detail::MASK + 17;  // 2^29 + 2^4
using AccX = FqB<66, LD>;                       // an accumulator's X, or any coordinate of a g1q_add operand
using AccYZ = FqB<4, LD>;                       // an accumulator's Y, Z
// an output is an input again: the induction every caller's loop closes by
template <class T>
BLS_HD Fq out(const T& a) {
  return relax<AccYZ::val, AccYZ::dig>(a).x;
}
}  // namespace g1q_detail

// complete mixed addition (RCB alg. 8): p an accumulator, (x2, y2) affine in N form
BLS_HD G1Q g1q_add_aff(const G1Q& p, const Fq& x2_, const Fq& y2_) {
  using namespace g1q_detail;
  const AccX X1{p.x};
  const AccYZ Y1{p.y}, Z1{p.z};
  const FqN x2{x2_}, y2{y2_};
  const FqN t0 = X1 * x2;
  const FqN t1 = Y1 * y2;
  const auto t3r = (x2 + y2) * (X1 + Y1) - (t0 + t1);
  const auto t3 = norm(t3r);
  const auto t4r = y2 * Z1 + Y1;
  const auto t4 = norm(t4r);
  const auto y3 = small<12>(x2 * Z1 + X1);
  const auto t0r = t0 + t0 + t0;
  const auto t0p = norm(t0r);
  const auto t2 = small<12>(Z1);
  const auto z3 = t1 + t2;  // unnormalised: its partners t1', t4 are
  const auto t1r = t1 - t2;
  const auto t1p = norm(t1r);
  const auto ny3 = neg(y3);  // unnormalised: its partner t4 is
  using T3 = decltype(t3);
  using T4 = decltype(t4);
  using T1 = decltype(t1p);
  static_assert(!dot2_fits<decltype(t3r), T1, T4, decltype(ny3)>(), "t3 needs no normalisation in X3");
  static_assert(!dot2_fits<T3, decltype(t1r), T4, decltype(ny3)>(), "t1' needs no normalisation in X3");
  static_assert(!dot2_fits<T3, T1, decltype(t4r), decltype(ny3)>(), "t4 needs no normalisation in X3");
  static_assert(!dot2_fits<T1, decltype(z3), decltype(y3), decltype(t0r)>(), "t0' needs no normalisation in Y3");
  G1Q r;
  r.y = out(dot2(t1p, z3, y3, t0p));
  r.z = out(dot2(z3, t4, t0p, t3));
  r.x = out(dot2(t3, t1p, t4, ny3));
  return r;
}

// complete projective addition (RCB alg. 7) of two L-form points, every coordinate below 66p
BLS_HD G1Q g1q_add(const G1Q& p, const G1Q& q) {
  using namespace g1q_detail;
  const AccX X1{p.x}, Y1{p.y}, Z1{p.z}, X2{q.x}, Y2{q.y}, Z2{q.z};
  const FqN t0 = X1 * X2, t1 = Y1 * Y2, t2 = Z1 * Z2;
  const auto t3r = (X1 + Y1) * (X2 + Y2) - (t0 + t1);
  const auto t3 = norm(t3r);
  const auto t4r = (Y1 + Z1) * (Y2 + Z2) - (t1 + t2);
  const auto t4 = norm(t4r);
  const auto y3 = small<12>((X1 + Z1) * (X2 + Z2) - (t0 + t2));
  const auto t0r = t0 + t0 + t0;
  const auto t0p = norm(t0r);
  const auto t2p = small<12>(t2);
  const auto z3 = t1 + t2p;  // unnormalised: its partners t1', t4 are
  const auto t1r = t1 - t2p;
  const auto t1p = norm(t1r);
  const auto ny3 = neg(y3);  // unnormalised: its partner t4 is
  using T3 = decltype(t3);
  using T4 = decltype(t4);
  using T1 = decltype(t1p);
  static_assert(!dot2_fits<decltype(t3r), T1, T4, decltype(ny3)>(), "t3 needs no normalisation in X3");
  static_assert(!dot2_fits<T3, T1, decltype(t4r), decltype(ny3)>(), "t4 needs no normalisation in X3");
  static_assert(!dot2_fits<T3, decltype(t1r), T4, decltype(ny3)>(), "t1' needs no normalisation in X3");
  static_assert(!dot2_fits<T1, decltype(z3), decltype(y3), decltype(t0r)>(), "t0' needs no normalisation in Y3");
  G1Q r;
  r.y = out(dot2(t1p, z3, y3, t0p));
  r.z = out(dot2(z3, t4, t0p, t3));
  r.x = out(dot2(t3, t1p, t4, ny3));
  return r;
}

// whether the plain product a b fits its columns with these bounds
template <class A, class B>
constexpr bool mul_fits() {
  return fqb_detail::columns_fit(A::dig, fqb_detail::top(A::val), B::dig, fqb_detail::top(B::val));
}

// sum of two affine points (x2, y2), (x3, y3) in N form with x2 != x3, in homogeneous coordinates without an
// inversion (the chord through both, denominators cleared by H^3):
//   H = x3 - x2,  R = y3 - y2,  HH = H^2,  HHH = H HH,  V = x2 HH,  W = R^2 - HHH - 2 V
//   X = H W,  Y = R (V - W) - y2 HHH = R (V - W) + HHH (K - y2),  Z = HHH
// two squarings, five digit products (Y is one dot2) and six reductions, against the 22 products and 16
// reductions of two mixed additions; the registry gather adds the result to its accumulator with g1q_add.
// INCOMPLETE: for x2 == x3 the result is (0 : -R^3 : 0) -- the identity -- when y3 == -y2 and (0 : 0 : 0), not
// a point, when the two points are equal.  The caller guards x2 != x3 (k_fav_gather_q: such a pair takes two
// g1q_add_aff).  Outputs in N form: operands of g1q_add.
BLS_HD G1Q g1q_add_aff2(const Fq& x2_, const Fq& y2_, const Fq& x3_, const Fq& y3_) {
  using namespace g1q_detail;
  const FqN x2{x2_}, y2{y2_}, x3{x3_}, y3{y3_};
  const auto Hr = x3 - x2;
  const auto Rr = y3 - y2;
  const auto H = norm(Hr);
  const auto R = norm(Rr);
  const FqN HH = sqr(H);
  const FqN HHH = H * HH;
  const FqN V = x2 * HH;
  const auto Wr = sqr(R) - (HHH + V + V);
  const auto W = norm(Wr);
  const auto VWr = V - W;
  const auto VW = norm(VWr);
  const auto ny2 = neg(y2);  // unnormalised: its partner HHH is
  static_assert(!mul_fits<decltype(Hr), decltype(Hr)>(), "H needs no normalisation in H^2");
  static_assert(!mul_fits<decltype(Rr), decltype(Rr)>(), "R needs no normalisation in R^2");
  static_assert(!mul_fits<decltype(H), decltype(Wr)>(), "W needs no normalisation in X");
  static_assert(!dot2_fits<decltype(R), decltype(VWr), FqN, decltype(ny2)>(), "V - W needs no normalisation in Y");
  G1Q r;
  r.x = out(H * W);
  r.y = out(dot2(R, VW, HHH, ny2));
  r.z = out(HHH);
  return r;
}

// complete doubling (RCB alg. 9) of an L-form point (every coordinate below 66p); X3 < 4p (digits <= 2^29),
// Y3, Z3 in N form
BLS_HD G1Q g1q_dbl(const G1Q& p) {
  using namespace g1q_detail;
  const AccX X1{p.x}, Y1{p.y}, Z1{p.z};
  const FqN t0 = Y1 * Y1;
  const FqN t1 = Y1 * Z1;
  const auto t2 = small<12>(Z1 * Z1);  // 3b Z^2, < 24p
  const FqN u = X1 * Y1;
  const auto z8 = small<8>(t0);
  const auto wr = t0 - small<3>(t2);  // t0 - 3 t2
  const auto w = norm(wr);
  static_assert(!dot2_fits<decltype(wr), decltype(t0 + t2), decltype(t2), decltype(z8)>(),
                "w needs no normalisation in Y3");
  G1Q r;
  r.z = out(t1 * z8);
  r.y = out(dot2(w, t0 + t2, t2, z8));  // no other operand needs normalising
  r.x = out(small<2>(w * u));
  return r;
}

}  // namespace bls
