// TEST HARNESS ONLY: host build of the six-term dot product (bls_fq.h fq_mul_dot6) and of the f accumulation's lane
// functions on it (bls_acc_dot.h: line_lane, sqr_lane, sqr_fin) with the digit form's 128-bit column checks (both
// accumulators), value checks and subtraction preconditions compiled in (BLS_FQ_CHECK): a stand-alone program that
// tests/test_accdot_cpu.py talks to through a pipe.  Everything travels as raw digit vectors (14 u32), so the test
// controls the redundant form of every operand and can feed an output back as the next input.
//
// The four lanes (h, q) of one f are run one after another; the exchanges the kernels make with DPP moves are plain
// copies here: a lane reads its h partner's half from the caller's arrays, and the two q lanes' components are put
// together after both have run.
#ifndef BLS_FQ_CHECK
#define BLS_FQ_CHECK 1
#endif
#define BLS_HD __host__ __device__ inline  // no forced inlining in this (host-only, checked) unit
#include "bls_ops.h"
#include "bls_kernels.h"
#include "bls_acc_dot.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
using namespace bls;

using F6 = Fq6B<ML_QF_V, ML_QF_D>;       // the loop-carried half of f
using L0 = Fq2B<ML_LV, ML_LD>;           // a line record's l0
using accdot::N2;
using accdot::N6;

// the h partner's half, held by the caller
struct CopyEx {
  const F6& partner;
  template <int A, int B>
  Fq2B<ML_QF_V, ML_QF_D> other(const F6&, bool h) const {
    return sel(!h, accdot::coef<A>(partner), accdot::coef<B>(partner));  // what the partner (an !h lane) sends
  }
  F6 half(const F6&) const { return partner; }
};

// an input must be inside the bound its type declares: the compile-time proofs start from there
template <uint64_t V, uint64_t D>
static FqB<V, D> in_fq(const uint32_t* d) {
  FqB<V, D> r;
  memcpy(r.x.d, d, 56);
  for (int i = 0; i < 13; ++i)
    if (r.x.d[i] > D) abort();
  if (fq_check_top(r.x) >= (double)V * 13.0020899) abort();
  return r;
}
template <uint64_t V, uint64_t D>
static Fq2B<V, D> in_fq2(const uint32_t* d) {
  return {in_fq<V, D>(d), in_fq<V, D>(d + 14)};
}
static F6 in_f6(const uint32_t* d) {
  return {in_fq2<ML_QF_V, ML_QF_D>(d), in_fq2<ML_QF_V, ML_QF_D>(d + 28), in_fq2<ML_QF_V, ML_QF_D>(d + 56)};
}
template <uint64_t V, uint64_t D>
static void out_f6(const Fq6B<V, D>& f, uint32_t* d) {
  static_assert(V <= ML_QF_V && D <= ML_QF_D, "a step's output must fit the loop-carried bound");
  const Fq2B<V, D>* c[3] = {&f.c0, &f.c1, &f.c2};
  for (int k = 0; k < 3; ++k) {
    memcpy(d + 28 * k, c[k]->c0.x.d, 56);
    memcpy(d + 28 * k + 14, c[k]->c1.x.d, 56);
  }
}
static N6 join(const FqN (&r0)[3], const FqN (&r1)[3]) {  // the q = 0 / q = 1 lanes' components
  return {{r0[0], r1[0]}, {r0[1], r1[1]}, {r0[2], r1[2]}};
}

// One request: op (u32) and 252 u32 of operands; one reply: 168 u32.
//   op 0: fq_mul_dot6(x0, y0, ..., x5, y5), operands in that order (12 x 14); reply: the 14 digits
//   op 1: f *= line: a (84), b (84), l0 (28), l2 (28), l3 (28); reply: the new a (84), b (84)
//   op 2: f = f^2:   a (84), b (84); reply: the new a, b
// Requests are served from stdin until it closes, so a test can feed a reply back; a failed check aborts the program
// (assert), which the test sees as a missing reply.
int main() {
  static uint32_t req[1 + 252], rep[168];
  while (fread(req, sizeof req, 1, stdin) == 1) {
    const uint32_t* in = req + 1;
    memset(rep, 0, sizeof rep);
    if (req[0] == 0) {
      Fq v[12];
      for (int t = 0; t < 12; ++t) memcpy(v[t].d, in + 14 * t, 56);
      const Fq r = fq_mul_dot6(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10], v[11]);
      memcpy(rep, r.d, 56);
    } else {
      const F6 half[2] = {in_f6(in), in_f6(in + 84)};  // a, b
      N6 P[2];
      if (req[0] == 1) {
        const L0 l0 = in_fq2<ML_LV, ML_LD>(in + 168);
        const N2 l2 = in_fq2<2, fqb_detail::MASK>(in + 196), l3 = in_fq2<2, fqb_detail::MASK>(in + 224);
        for (int h = 0; h < 2; ++h) {
          FqN r[2][3];
          for (int q = 0; q < 2; ++q) accdot::line_lane(half[h], h != 0, q != 0, l0, l2, l3, CopyEx{half[1 - h]}, r[q]);
          P[h] = join(r[0], r[1]);
        }
        out_f6(P[0], rep);
        out_f6(P[1], rep + 84);
      } else {
        for (int h = 0; h < 2; ++h) {
          FqN r[2][3];
          for (int q = 0; q < 2; ++q) accdot::sqr_lane(half[h], h != 0, q != 0, CopyEx{half[1 - h]}, r[q]);
          P[h] = join(r[0], r[1]);
        }
        out_f6(accdot::sqr_fin(P[0], P[1], false), rep);  // t = a b: the h = 1 lanes' product
        out_f6(accdot::sqr_fin(P[1], P[1], true), rep + 84);
      }
    }
    if (fwrite(rep, sizeof rep, 1, stdout) != 1 || fflush(stdout)) return 1;
  }
  return 0;
}
