// TEST HARNESS ONLY: host build of the Miller loop's G2 line steps (bls_miller_lines.h: ln_dbl / ln_add) and of the
// mixed Jacobian addition of the signature subgroup chain (bls_fq_g2.h: j2q_add_aff, j2q_mul_xabs_aff) with the
// digit form's 128-bit column, value and subtraction-precondition checks compiled in (BLS_FQ_CHECK), for
// tests/test_mlines_cpu.py.
#define BLS_FQ_CHECK 1
#define BLS_HD __host__ __device__ inline  // no forced inlining in this (host-only, checked) unit
#include "bls_ops.h"
#include "bls_miller_lines.h"
#include "bls_fq_g2.h"
#include <string.h>
using namespace bls;
using namespace bls::mlines;

static Fp in_fp(const uint8_t* b) { return fp_to_mont(raw_from_be48(b)); }
static void out_fp(uint8_t* b, const Fp& a) { raw_to_be48(fp_from_mont(a), b); }
template <uint64_t V, uint64_t D>
static void out_fq2(uint8_t* b, const Fq2B<V, D>& a) {
  const Fp2 v = fq2b_pack(a);
  out_fp(b, v.c0);
  out_fp(b + 48, v.c1);
}

// The 68 steps of the loop over |x| on Q = (x, y) (q = x.c0 || x.c1 || y.c0 || y.c1, 48 B big-endian each).  Step
// k writes 577 bytes at out + 577 k: kind (0 doubling, 1 addition), T after the step as X || Y || Z and the step's
// record l0 || l2 || l3 (96 B each, c0 || c1).  Returns the number of steps.
extern "C" int hc_ml_steps(const uint8_t* q, uint8_t* out) {
  const Fp2 x{in_fp(q), in_fp(q + 48)}, y{in_fp(q + 96), in_fp(q + 144)};
  const QF qx = fq2b_canon(x), qy = fq2b_canon(y);
  const FqC one = fqb_canon(FP_ONE), zero{fq_zero()};
  TF X = relax<LN_TV, LN_TD>(qx), Y = relax<LN_TV, LN_TD>(qy), Z = relax<LN_TV, LN_TD>(QF{one, zero});
  int k = 0;
  auto put = [&](int kind, const LF& l0, const LF& l2, const LF& l3) {
    uint8_t* o = out + 577 * (size_t)k++;
    o[0] = (uint8_t)kind;
    out_fq2(o + 1, X);
    out_fq2(o + 97, Y);
    out_fq2(o + 193, Z);
    out_fq2(o + 289, l0);
    out_fq2(o + 385, l2);
    out_fq2(o + 481, l3);
  };
  for (int b = 62; b >= 0; --b) {
    LF l0, l2, l3;
    ln_dbl(X, Y, Z, [&](const LF& a0, const LF& a2, const LF& a3) { l0 = a0, l2 = a2, l3 = a3; });
    put(0, l0, l2, l3);
    if ((X_ABS >> b) & 1ull) {
      ln_add(X, Y, Z, qx, qy, l0, l2, l3);
      put(1, l0, l2, l3);
    }
  }
  return k;
}

static Fq2 in_fq2(const uint8_t* b) { return fq2_unpack(Fp2{in_fp(b), in_fp(b + 48)}); }
static void out_j2q(uint8_t* o, const J2Q& m) {
  const Fp2 X = fq2_pack(m.x), Y = fq2_pack(m.y), Z = fq2_pack(m.z);
  out_fp(o, X.c0), out_fp(o + 48, X.c1), out_fp(o + 96, Y.c0), out_fp(o + 144, Y.c1), out_fp(o + 192, Z.c0),
      out_fp(o + 240, Z.c1);
}

// [|x|] (x, y) through the chain with mixed additions (q = x.c0 || x.c1 || y.c0 || y.c1): out = Jacobian X || Y ||
// Z (96 B each); returns exc
extern "C" int hc_sig_xabs(const uint8_t* q, uint8_t* out) {
  bool exc = false;
  out_j2q(out, j2q_mul_xabs_aff(in_fq2(q), in_fq2(q + 96), exc));
  return exc ? 1 : 0;
}

// one mixed addition (X, Y, Z) + (x, y): p = X || Y || Z, q = x || y; out as above; returns exc
extern "C" int hc_madd(const uint8_t* p, const uint8_t* q, uint8_t* out) {
  bool exc = false;
  const J2Q P{in_fq2(p), in_fq2(p + 96), in_fq2(p + 192)};
  out_j2q(out, j2q_add_aff(P, in_fq2(q), in_fq2(q + 96), exc));
  return exc ? 1 : 0;
}
