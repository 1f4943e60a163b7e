// Complete projective G1 additions (Renes-Costello-Batina alg. 7 / 8 / 9, a = 0,
// b3 = 12) in the redundant digit form of bls_fq.h, for the registry gather
// (k_fav_gather_q, bls_kernels.hip), the r_i apk_i chain (bls_g1_endo.h) and the
// segmented and workgroup G1 sums.
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
// The host tests (tests/test_hostcheck.py::test_fq_gather_formulas,
// tests/test_g1dot_cpu.py) run these formulas with the 128-bit column checks of
// bls_fq.h.
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
