// TEST HARNESS ONLY: host build of csrc/bls_fr.h and csrc/bls_kzg_blob.h.  tests/test_fr_cpu.py drives the
// extern "C" functions through ctypes, and runs the same cases through the stand-alone program (HC_FR_MAIN, built
// with -fsanitize=address,undefined) from a vector file it writes.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "bls_kzg_blob.h"

using namespace bls;

enum { OP_ADD, OP_SUB, OP_NEG, OP_MUL, OP_SQR, OP_INV, OP_POW, OP_REDUCE, OP_FROM };

static const std::vector<Fr>& domain() {
  static std::vector<Fr> dom;
  if (dom.empty()) {
    dom.resize(KZB_N);
    for (uint32_t i = 0; i < KZB_N; ++i) dom[i] = kzb_domain_entry(i);
  }
  return dom;
}

extern "C" {

// out32 = op(a, b, e) on canonical 32-byte operands; returns -1 if an operand is not below r.  OP_REDUCE takes any
// 256-bit a; OP_FROM returns fr_from_be32's verdict on any 256-bit a, with the decoded value (zero if rejected)
int hc_fr_op(int op, const uint8_t* a32, const uint8_t* b32, uint32_t e, uint8_t* out32) {
  Fr a = fr_zero(), b = fr_zero(), r = fr_zero();
  if (op == OP_REDUCE) {
    fr_to_be32(fr_from_be32_reduce(a32), out32);
    return 1;
  }
  if (op == OP_FROM) {
    const bool ok = fr_from_be32(r, a32);
    fr_to_be32(r, out32);
    return ok ? 1 : 0;
  }
  if (!fr_from_be32(a, a32) || !fr_from_be32(b, b32)) return -1;
  switch (op) {
    case OP_ADD: r = fr_add(a, b); break;
    case OP_SUB: r = fr_sub(a, b); break;
    case OP_NEG: r = fr_neg(a); break;
    case OP_MUL: r = fr_mul(a, b); break;
    case OP_SQR: r = fr_sqr(a); break;
    case OP_INV: r = fr_inv(a); break;
    case OP_POW: r = fr_pow_u32(a, e); break;
    default: return -2;
  }
  fr_to_be32(r, out32);
  return 1;
}

// the header's constants as integers: r, R mod r, R^2 mod r (limbs as they stand), omega and 1 / 4096 (taken out
// of Montgomery form), then -1 / r mod 2^32 in the last four bytes of a sixth 32-byte string
void hc_fr_constants(uint8_t* out192) {
  fr_raw_to_be32(fr_modulus(), out192);
  fr_raw_to_be32(fr_one(), out192 + 32);
  fr_raw_to_be32(Fr{{FR_R2_LIMBS}}, out192 + 64);
  fr_to_be32(fr_omega(), out192 + 96);
  fr_to_be32(fr_inv_4096(), out192 + 128);
  Fr n = fr_zero();
  n.l[0] = FR_NINV;
  fr_raw_to_be32(n, out192 + 160);
}

uint32_t hc_kzb_shape(int what) { return what == 0 ? KZB_N : what == 1 ? KZB_LANES : KZB_RUN; }

void hc_kzb_domain(uint8_t* out) {
  const std::vector<Fr>& dom = domain();
  for (uint32_t i = 0; i < KZB_N; ++i) fr_to_be32(dom[i], out + 32 * i);
}

// One blob evaluated and divided as the kernels do it, lane by lane: y32 = p(z), q32 = the 4,096 quotient scalars,
// *hit = the domain index z equals or -1.  Returns 1, or 0 if an element is not below r, -1 if z is not.
int hc_kzb_blob(const uint8_t* blob, const uint8_t* z32, uint8_t* y32, uint8_t* q32, int* hit) {
  const std::vector<Fr>& dom = domain();
  std::vector<Fr> f(KZB_N), pre(KZB_N);
  int ok = 1;
  for (uint32_t i = 0; i < KZB_N; ++i)
    if (!fr_from_be32(f[i], blob + 32 * i)) ok = 0;
  Fr z;
  if (!fr_from_be32(z, z32)) return -1;
  Fr total = fr_zero();
  int h = -1;
  for (uint32_t t = 0; t < KZB_LANES; ++t) {
    const KzbLane r = kzb_eval_lane(dom.data(), f.data(), z, t, pre.data());
    total = fr_add(total, r.sum);
    if (r.hit >= 0) h = r.hit;
  }
  const Fr y = kzb_eval_finish(total, z, f.data(), h);
  fr_to_be32(y, y32);
  *hit = h;
  total = fr_zero();
  for (uint32_t t = 0; t < KZB_LANES; ++t) total = fr_add(total, kzb_quot_lane(dom.data(), f.data(), z, y, h, t, q32, pre.data()));
  if (h >= 0) kzb_quot_finish(total, z, h, q32);
  return ok;
}

}  // extern "C"

#ifdef HC_FR_MAIN
// Vector file: u32 count of operation cases, each {u32 op, u32 e, a[32], b[32], i32 want_rc, want[32]}; the domain
// (4,096 x 32 bytes); u32 count of blob cases, each {blob[131072], z[32], i32 want_rc, i32 want_hit, y[32],
// q[131072]}.  Exit status 0 iff everything matches.
static bool rd(FILE* fh, void* p, size_t n) { return fread(p, 1, n, fh) == n; }

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* fh = fopen(argv[1], "rb");
  if (!fh) return 2;
  int bad = 0;
  uint32_t n = 0;
  if (!rd(fh, &n, 4)) return 2;
  for (uint32_t c = 0; c < n; ++c) {
    uint32_t op, e;
    int32_t want_rc;
    uint8_t a[32], b[32], want[32], got[32];
    if (!rd(fh, &op, 4) || !rd(fh, &e, 4) || !rd(fh, a, 32) || !rd(fh, b, 32) || !rd(fh, &want_rc, 4) ||
        !rd(fh, want, 32))
      return 2;
    const int rc = hc_fr_op((int)op, a, b, e, got);
    if (rc != want_rc || memcmp(got, want, 32)) {
      printf("operation case %u (op %u): mismatch\n", c, op);
      bad++;
    }
  }
  std::vector<uint8_t> dom(32 * KZB_N), got_dom(32 * KZB_N);
  if (!rd(fh, dom.data(), dom.size())) return 2;
  hc_kzb_domain(got_dom.data());
  if (dom != got_dom) {
    printf("domain table: mismatch\n");
    bad++;
  }
  if (!rd(fh, &n, 4)) return 2;
  std::vector<uint8_t> blob(32 * KZB_N), q(32 * KZB_N), got_q(32 * KZB_N);
  for (uint32_t c = 0; c < n; ++c) {
    uint8_t z[32], y[32], got_y[32];
    int32_t want_rc, want_hit;
    if (!rd(fh, blob.data(), blob.size()) || !rd(fh, z, 32) || !rd(fh, &want_rc, 4) || !rd(fh, &want_hit, 4) ||
        !rd(fh, y, 32) || !rd(fh, q.data(), q.size()))
      return 2;
    int hit = -2;
    const int rc = hc_kzb_blob(blob.data(), z, got_y, got_q.data(), &hit);
    if (rc != want_rc || hit != want_hit || memcmp(y, got_y, 32) || q != got_q) {
      printf("blob case %u: mismatch (rc %d hit %d)\n", c, rc, hit);
      bad++;
    }
  }
  fclose(fh);
  printf("hostcheck_fr: %d mismatches\n", bad);
  return bad ? 1 : 0;
}
#endif
