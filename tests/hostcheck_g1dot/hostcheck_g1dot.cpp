// TEST HARNESS ONLY: host build of the complete G1 formulas (bls_fq_g1.h) and the endomorphism chain on them
// (bls_g1_endo.h) with the digit form's 128-bit column, value and subtraction-precondition checks compiled in
// (BLS_FQ_CHECK): a stand-alone program that tests/test_g1dot_cpu.py talks to through a pipe.  Points go in and
// out as raw digit vectors (3 x 14 u32), so the test controls the redundant form of every operand and can feed an
// output back as the next input.
#ifndef BLS_FQ_CHECK
#define BLS_FQ_CHECK 1
#endif
#define BLS_HD __host__ __device__ inline  // no forced inlining in this (host-only, checked) unit
#include "bls_ops.h"
#include "bls_g1_endo.h"
#include <stdio.h>
#include <string.h>
using namespace bls;

// The formulas as they stood before every output coordinate became one dot product: one Montgomery reduction per
// product, the two products of a coordinate combined after both were reduced.  Kept here so that the test can
// show the packed coordinates did not change.
namespace before {
static G1Q g1q_add_aff(const G1Q& p, const Fq& x2, const Fq& y2) {
  const Fq t0 = fq_mul(p.x, x2);
  const Fq t1 = fq_mul(p.y, y2);
  const Fq t3 = fq_norm(fq_sub2(fq_mul(fq_add(x2, y2), fq_add(p.x, p.y)), fq_add(t0, t1)));
  const Fq t4 = fq_add(fq_mul(y2, p.z), p.y);
  const Fq y3 = fq_mul_small(fq_add(fq_mul(x2, p.z), p.x), 12);
  const Fq t0p = fq_add(fq_add(t0, t0), t0);
  const Fq t2 = fq_mul_small(p.z, 12);
  const Fq z3 = fq_norm(fq_add(t1, t2));
  const Fq t1p = fq_sub(t1, t2);
  G1Q r;
  r.x = fq_norm(fq_sub(fq_mul(t3, t1p), fq_mul(t4, y3)));
  r.y = fq_norm(fq_add(fq_mul(t1p, z3), fq_mul(y3, t0p)));
  r.z = fq_norm(fq_add(fq_mul(z3, t4), fq_mul(t0p, t3)));
  return r;
}
static G1Q g1q_add(const G1Q& p, const G1Q& q) {
  const Fq t0 = fq_mul(p.x, q.x), t1 = fq_mul(p.y, q.y), t2 = fq_mul(p.z, q.z);
  const Fq t3 = fq_norm(fq_sub2(fq_mul(fq_add(p.x, p.y), fq_add(q.x, q.y)), fq_add(t0, t1)));
  const Fq t4 = fq_norm(fq_sub2(fq_mul(fq_add(p.y, p.z), fq_add(q.y, q.z)), fq_add(t1, t2)));
  const Fq y3 = fq_mul_small(fq_sub2(fq_mul(fq_add(p.x, p.z), fq_add(q.x, q.z)), fq_add(t0, t2)), 12);
  const Fq t0p = fq_add(fq_add(t0, t0), t0);
  const Fq t2p = fq_mul_small(t2, 12);
  const Fq z3 = fq_norm(fq_add(t1, t2p));
  const Fq t1p = fq_sub(t1, t2p);
  G1Q r;
  r.x = fq_norm(fq_sub(fq_mul(t3, t1p), fq_mul(t4, y3)));
  r.y = fq_norm(fq_add(fq_mul(t1p, z3), fq_mul(y3, t0p)));
  r.z = fq_norm(fq_add(fq_mul(z3, t4), fq_mul(t0p, t3)));
  return r;
}
static G1Q g1q_dbl(const G1Q& p) {
  const Fq t0 = fq_mul(p.y, p.y);
  const Fq t1 = fq_mul(p.y, p.z);
  const Fq t2 = fq_mul_small(fq_mul(p.z, p.z), 12);
  const Fq u = fq_mul(p.x, p.y);
  const Fq z8 = fq_mul_small(t0, 8);
  const Fq x3a = fq_mul(t2, z8);
  G1Q r;
  r.z = fq_mul(t1, z8);
  const Fq w = fq_norm(fq_sub2(t0, fq_mul_small(t2, 3)));
  r.y = fq_norm(fq_add(fq_mul(w, fq_add(t0, t2)), x3a));
  r.x = fq_mul_small(fq_mul(w, u), 2);
  return r;
}
}  // namespace before

static G1Q in_pt(const uint32_t* d) {
  G1Q p;
  memcpy(p.x.d, d, 56);
  memcpy(p.y.d, d + 14, 56);
  memcpy(p.z.d, d + 28, 56);
  return p;
}
// digits (3 x 14 u32) and the canonical packed coordinates (fq_pack: 3 x 12 u32 Montgomery limbs)
static void out_pt(const G1Q& r, uint32_t* digits, uint32_t* packed) {
  memcpy(digits, r.x.d, 56);
  memcpy(digits + 14, r.y.d, 56);
  memcpy(digits + 28, r.z.d, 56);
  const Fp c[3] = {fq_pack(r.x), fq_pack(r.y), fq_pack(r.z)};
  for (int k = 0; k < 3; ++k) memcpy(packed + 12 * k, c[k].l, 48);
}

// One request: op, old, a, b (4 x u32), p (42 u32), q (42 u32); one reply: digits (42 u32), packed (36 u32).
//   op 0: g1q_add_aff(p, q.x, q.y); 1: g1q_add(p, q); 2: g1q_dbl(p); 3: g1q_mul_endo(p, a, b) = a p + b phi(p)
//   old != 0 (ops 0 .. 2): the formulas of namespace before
// Requests are served from stdin until it closes, so a test can feed a reply back; a failed check aborts the
// program (assert), which the test sees as a missing reply.
int main() {
  uint32_t req[4 + 84], rep[42 + 36];
  while (fread(req, sizeof req, 1, stdin) == 1) {
    const uint32_t op = req[0];
    const bool old = req[1] != 0;
    const G1Q P = in_pt(req + 4), Q = in_pt(req + 46);
    G1Q r;
    if (op == 0)
      r = old ? before::g1q_add_aff(P, Q.x, Q.y) : g1q_add_aff(P, Q.x, Q.y);
    else if (op == 1)
      r = old ? before::g1q_add(P, Q) : g1q_add(P, Q);
    else if (op == 2)
      r = old ? before::g1q_dbl(P) : g1q_dbl(P);
    else
      r = g1q_mul_endo(P, req[2], req[3]);
    out_pt(r, rep, rep + 42);
    if (fwrite(rep, sizeof rep, 1, stdout) != 1 || fflush(stdout)) return 1;
  }
  return 0;
}
