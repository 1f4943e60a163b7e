// TEST HARNESS ONLY: host build of the pair sum of the registry gather (bls_fq_g1.h: g1q_add_aff2) and of the
// gather's loop step on it, with the digit form's 128-bit column, value and subtraction-precondition checks
// compiled in (BLS_FQ_CHECK): a stand-alone program that tests/test_g1pair_cpu.py talks to through a pipe.  Points
// go in and out as raw digit vectors (3 x 14 u32), so the test controls the redundant form of every operand and can
// feed an output back as the next input.
#ifndef BLS_FQ_CHECK
#define BLS_FQ_CHECK 1
#endif
#define BLS_HD __host__ __device__ inline  // no forced inlining in this (host-only, checked) unit
#include "bls_ops.h"
#include "bls_fq_g1.h"
#include <stdio.h>
#include <string.h>
using namespace bls;

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

// k_fav_gather_q's step on a pair of registry keys a, b (canonical, as fq_unpack of a record leaves them): the pair
// sum and one complete addition, or -- the guard -- two complete mixed additions when the canonical x limbs are equal
// (a repeated key, a key beside its negation).  *fast = which path ran.
static G1Q gather_step(const G1Q& acc, const G1Q& a, const G1Q& b, uint32_t* fast) {
  const Fp xa = fq_pack(a.x), xb = fq_pack(b.x);
  *fast = fp_eq(xa, xb) ? 0u : 1u;
  if (*fast) return g1q_add(acc, g1q_add_aff2(a.x, a.y, b.x, b.y));
  return g1q_add_aff(g1q_add_aff(acc, a.x, a.y), b.x, b.y);
}

// One request: op and three pad words (4 x u32), p, q, s (42 u32 each); one reply: digits (42 u32), packed (36 u32),
// fast (1 u32).
//   op 0: g1q_add_aff2(p.x, p.y, q.x, q.y); 1: g1q_add(p, q); 2: g1q_add_aff(p, q.x, q.y);
//   3: gather_step(p, q, s) (q, s affine: their z is ignored); 4: g1q_add_aff(g1q_add_aff(p, q.x, q.y), s.x, s.y)
// Requests are served from stdin until it closes, so a test can feed a reply back; a failed check aborts the
// program (assert), which the test sees as a missing reply.
int main() {
  uint32_t req[4 + 126], rep[42 + 36 + 1];
  while (fread(req, sizeof req, 1, stdin) == 1) {
    const uint32_t op = req[0];
    const G1Q P = in_pt(req + 4), Q = in_pt(req + 46), S = in_pt(req + 88);
    G1Q r;
    uint32_t fast = 0;
    if (op == 0)
      r = g1q_add_aff2(P.x, P.y, Q.x, Q.y);
    else if (op == 1)
      r = g1q_add(P, Q);
    else if (op == 2)
      r = g1q_add_aff(P, Q.x, Q.y);
    else if (op == 3)
      r = gather_step(P, Q, S, &fast);
    else
      r = g1q_add_aff(g1q_add_aff(P, Q.x, Q.y), S.x, S.y);
    out_pt(r, rep, rep + 42);
    rep[78] = fast;
    if (fwrite(rep, sizeof rep, 1, stdout) != 1 || fflush(stdout)) return 1;
  }
  return 0;
}
