// The Fp12 steps of the four-lane f accumulation (k_miller_acc4q, k_miller_fused: bls_miller_pair.hip) as dot
// products with ONE Montgomery reduction per output Fp coefficient (fq_mul_dot6, bls_fq.h), lane by lane.
//
// Lane (h, q) owns the half `own` of f = a + b w (h = 0: a, h = 1: b) and forms one Fp component of each of its
// three output Fp2 coefficients: the real part on q = 0, the imaginary part on q = 1.  An Fp6 coefficient that is a
// sum of three Fp2 products u_t y_t is, per component,
//   Re = sum u_t.c0 y_t.c0 + u_t.c1 (-y_t.c1)      Im = sum u_t.c0 y_t.c1 + u_t.c1 y_t.c0
// so with the y operand prepared per lane as (ya, yb) = q ? (y.c1, y.c0) : (y.c0, K - y.c1) both are
// sum u_t.c0 ya_t + u_t.c1 yb_t: one dot6, the same instruction stream on both q, no select on the u side.
// xi y = (y.c0 - y.c1, y.c0 + y.c1) is prepared the same way, so the xi of v^3 = xi costs additions on the y side
// and no product.  A prepared operand is normalised where its digits (a negation's borrowed digits, a sum) would
// not fit dot6's columns; the bound types decide that at compile time (ACC_YD, and dot6's static_assert proves
// the fit).
//
// The functions here hold everything a lane computes between exchanges; the exchanges themselves come in through
// `Ex` (DPP moves on the device, plain copies in the host harness tests/hostcheck_accdot) and the joins of the two
// q lanes' components are the caller's.
#pragma once
#include "bls_fqb.h"

namespace bls {
namespace accdot {

#if defined(__HIP_DEVICE_COMPILE__)
// the three dot products of a step run one after another (interleaved they hold three column sets live)
#define ACC_SEQ() __builtin_amdgcn_sched_barrier(0)
#else
#define ACC_SEQ() ((void)0)
#endif

using N2 = Fq2B<2, fqb_detail::MASK>;
using N6 = Fq6B<2, fqb_detail::MASK>;

// digits a prepared y operand may keep without normalisation (L form)
constexpr uint64_t ACC_YD = 0x20000000ull + 64;
template <uint64_t V, uint64_t D>
BLS_HD auto fit(const FqB<V, D>& a) {
  if constexpr (D > ACC_YD)
    return norm(a);
  else
    return a;
}

// a prepared y operand: (a, b) = q ? (y.c1, y.c0) : (y.c0, -y.c1)
template <class A, class B>
struct YP {
  A a;
  B b;
};
template <class A, class B>
BLS_HD YP<A, B> yp(const A& a, const B& b) {
  return {a, b};
}
template <uint64_t V, uint64_t D>
BLS_HD auto prep(const Fq2B<V, D>& y, bool q) {
  return yp(fit(sel(q, y.c1, y.c0)), fit(sel(q, y.c0, neg(y.c1))));
}
// the same for xi y = (y.c0 - y.c1) + (y.c0 + y.c1) i
template <uint64_t V, uint64_t D>
BLS_HD auto prep_xi(const Fq2B<V, D>& y, bool q) {
  const auto d = y.c0 + neg(y.c1);
  const auto s = y.c0 + y.c1;
  return yp(fit(sel(q, s, d)), fit(sel(q, d, neg(s))));
}
template <class A1, class B1, class A2, class B2>
BLS_HD auto sel(bool c, const YP<A1, B1>& x, const YP<A2, B2>& y) {
  return yp(sel(c, x.a, y.a), sel(c, x.b, y.b));
}

// this lane's component of u0 y0 + u1 y1 + u2 y2: the u.c0 ya products share dot6's first accumulator with the
// reduction products, the u.c1 yb products have the second
template <uint64_t V0, uint64_t D0, class P0, uint64_t V1, uint64_t D1, class P1, uint64_t V2, uint64_t D2, class P2>
BLS_HD FqN dot3(const Fq2B<V0, D0>& u0, const P0& p0, const Fq2B<V1, D1>& u1, const P1& p1, const Fq2B<V2, D2>& u2,
                const P2& p2) {
  return dot6(u0.c0, p0.a, u1.c0, p1.a, u2.c0, p2.a, u0.c1, p0.b, u1.c1, p1.b, u2.c1, p2.b);
}

template <int I, uint64_t V, uint64_t D>
BLS_HD const Fq2B<V, D>& coef(const Fq6B<V, D>& a) {
  if constexpr (I == 0)
    return a.c0;
  else if constexpr (I == 1)
    return a.c1;
  else
    return a.c2;
}

// own *= line, L = (l0, l2, 0) + (0, l3, 0) w.  With X = h ? o : v o (o the other half: X = a on the h = 1 lanes,
// (xi b2, b0, b1) on h = 0) both halves are own (l0, l2, 0) + X (0, l3, 0):
//   r0 = own0 l0 + own2 (xi l2) + X2 (xi l3)
//   r1 = own0 l2 + own1 l0      + X0 l3        (h = 0: X0 l3 = b2 (xi l3))
//   r2 = own1 l2 + own2 l0      + X1 l3
// r[k]: this lane's component of r_k, N form.  ex.other<A, B>(own, h) is the coefficient the h partner sends: its c_A
// if the partner is an h = 1 lane, its c_B if it is an h = 0 lane -- fetched one at a time, right before its product.
template <class Ex, uint64_t V, uint64_t D, uint64_t VL, uint64_t DL, uint64_t VM, uint64_t DM>
BLS_HD void line_lane(const Fq6B<V, D>& own, bool h, bool q, const Fq2B<VL, DL>& l0, const Fq2B<VM, DM>& l2,
                      const Fq2B<VM, DM>& l3, const Ex& ex, FqN (&r)[3]) {
  const auto p0 = prep(l0, q);
  const auto x3 = prep_xi(l3, q);
  r[0] = dot3(own.c0, p0, own.c2, prep_xi(l2, q), ex.template other<1, 2>(own, h), x3);
  ACC_SEQ();
  const auto p2 = prep(l2, q);
  const auto p3 = prep(l3, q);
  r[1] = dot3(own.c0, p2, own.c1, p0, ex.template other<2, 0>(own, h), sel(h, p3, x3));
  ACC_SEQ();
  r[2] = dot3(own.c1, p2, own.c2, p0, ex.template other<0, 1>(own, h), p3);
  ACC_SEQ();
}

// The Fp12 squaring (a + b w)^2 = (a^2 + v b^2) + 2 a b w from one Fp6 product per half: X Y with
//   h = 0: X = a + b, Y = a + v b   (X Y - a b - v a b = a^2 + v b^2)        h = 1: X = a, Y = b
// as the schoolbook sums c0 = X0 Y0 + X1 (xi Y2) + X2 (xi Y1), c1 = X0 Y1 + X1 Y0 + X2 (xi Y2),
// c2 = X0 Y2 + X1 Y1 + X2 Y0.  r[k]: this lane's component of c_k.  ex.half(own): the other half.
template <class Ex, uint64_t V, uint64_t D>
BLS_HD void sqr_lane(const Fq6B<V, D>& own, bool h, bool q, const Ex& ex, FqN (&r)[3]) {
  const auto o = ex.half(own);
  const auto X = norm(sel(h, o, own + o));
  const auto Y = norm(sel(h, own, own + f6v(o)));
  const auto p0 = prep(Y.c0, q);
  const auto x2 = prep_xi(Y.c2, q);
  r[0] = dot3(X.c0, p0, X.c1, x2, X.c2, prep_xi(Y.c1, q));
  ACC_SEQ();
  const auto p1 = prep(Y.c1, q);
  r[1] = dot3(X.c0, p1, X.c1, p0, X.c2, x2);
  ACC_SEQ();
  r[2] = dot3(X.c0, prep(Y.c2, q), X.c1, p1, X.c2, p0);
  ACC_SEQ();
}
// the squaring's last step, from this half's product P and the h = 1 lanes' t = a b
BLS_HD auto sqr_fin(const N6& P, const N6& t, bool h) { return norm(sel(h, P + P, (P - t) - f6v(t))); }

}  // namespace accdot

// loop-carried bound of the digit-form f halves in k_miller_acc4q and k_miller_fused: a line product leaves N form, a
// squaring sqr_fin's sum of N-form values, whatever the bound going in
using AccSqrOut = decltype(accdot::sqr_fin(accdot::N6{}, accdot::N6{}, false).c0.c0);
constexpr uint64_t ML_QF_V = AccSqrOut::val, ML_QF_D = AccSqrOut::dig;
static_assert(ML_QF_V == 11 && ML_QF_D == 0x20000000ull + 5, "the bound DESIGN 4.3 and tests/test_accdot_cpu.py state");

}  // namespace bls
