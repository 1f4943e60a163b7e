// TEST HARNESS ONLY: host build of the G1 endomorphism chain (bls_g1_endo.h) with the digit form's 128-bit column,
// value and subtraction-precondition checks compiled in (BLS_FQ_CHECK), for tests/test_endo_cpu.py.
#define BLS_FQ_CHECK 1
#define BLS_HD __host__ __device__ inline  // no forced inlining in this (host-only, checked) unit
#include "bls_ops.h"
#include "bls_g1_endo.h"
#include <string.h>
using namespace bls;

static Fp in_fp(const uint8_t* b) { return fp_to_mont(raw_from_be48(b)); }
static void out_fp(uint8_t* b, const Fp& a) { raw_to_be48(fp_from_mont(a), b); }

// a A + b phi(A) by g1q_mul_endo; p = projective X || Y || Z (48 B big-endian each, canonical), as k_sig_lane2
// passes its apk_i; out = affine x || y, or 96 zero bytes for the identity
extern "C" void hc_endo_mul(const uint8_t* p, uint32_t a, uint32_t b, uint8_t* o) {
  const G1Q A{fq_unpack(in_fp(p)), fq_unpack(in_fp(p + 48)), fq_unpack(in_fp(p + 96))};
  const G1Q R = g1q_mul_endo(A, a, b);
  const Fp X = fq_pack(R.x), Y = fq_pack(R.y), Z = fq_pack(R.z);
  if (fp_is_zero(Z)) {
    memset(o, 0, 96);
    return;
  }
  const Fp zi = fp_inv(Z);
  out_fp(o, fp_mul(X, zi));
  out_fp(o + 48, fp_mul(Y, zi));
}

// FP_BETA, canonical big-endian
extern "C" void hc_endo_beta(uint8_t* o) { out_fp(o, FP_BETA); }
