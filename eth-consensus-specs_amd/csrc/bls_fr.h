// The scalar field F_r of BLS12-381 (r = 0x73eda753...00000001, 255 bits) for device and host: the arithmetic under
// the KZG blob functions (bls_kzg_blob.h) and the cell functions' transform (bls_fr_ntt.h).
//
// A value is a canonical residue (< r) in Montgomery form with R = 2^256, eight 32-bit little-endian limbs.  Products
// are CIOS with 64-bit multiply-adds: a column t + a b + c of 32-bit operands is at most 2^64 - 1, so ordinary
// carries suffice, and with r < 2^255 the running value stays below 2 r < 2^256 (no ninth limb survives a round).
// Every loop has constant bounds and is unrolled: no array here is indexed at run time.
#pragma once
#include <stdint.h>

#include "bls_field_types.h"
#include "bls_fr_constants.h"

namespace bls {

struct alignas(16) Fr {
  uint32_t l[8];
};

BLS_HD Fr fr_zero() { return Fr{{0, 0, 0, 0, 0, 0, 0, 0}}; }
BLS_HD Fr fr_one() { return Fr{{FR_ONE_LIMBS}}; }
BLS_HD Fr fr_modulus() { return Fr{{FR_MOD_LIMBS}}; }
BLS_HD Fr fr_omega() { return Fr{{FR_OMEGA_LIMBS}}; }
BLS_HD Fr fr_inv_4096() { return Fr{{FR_INV_4096_LIMBS}}; }

BLS_HD bool fr_is_zero(const Fr& a) {
  uint32_t v = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) v |= a.l[i];
  return v == 0;
}

BLS_HD bool fr_eq(const Fr& a, const Fr& b) {
  uint32_t v = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) v |= a.l[i] ^ b.l[i];
  return v == 0;
}

// a - b over the integers; returns the borrow (1 iff a < b)
BLS_HD uint32_t fr_raw_sub(Fr& out, const Fr& a, const Fr& b) {
  uint64_t br = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint64_t d = (uint64_t)a.l[i] - b.l[i] - br;
    out.l[i] = (uint32_t)d;
    br = (d >> 32) & 1u;
  }
  return (uint32_t)br;
}

// a + b over the integers; returns the carry
BLS_HD uint32_t fr_raw_add(Fr& out, const Fr& a, const Fr& b) {
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    c += (uint64_t)a.l[i] + b.l[i];
    out.l[i] = (uint32_t)c;
    c >>= 32;
  }
  return (uint32_t)c;
}

// v if v < r, else v - r (v < 2 r)
BLS_HD Fr fr_reduce_once(const Fr& v) {
  Fr d;
  const uint32_t br = fr_raw_sub(d, v, fr_modulus());
  Fr o;
#pragma unroll
  for (int i = 0; i < 8; ++i) o.l[i] = br ? v.l[i] : d.l[i];
  return o;
}

BLS_HD Fr fr_add(const Fr& a, const Fr& b) {
  Fr s;
  fr_raw_add(s, a, b);  // < 2 r < 2^256: no carry out
  return fr_reduce_once(s);
}

BLS_HD Fr fr_sub(const Fr& a, const Fr& b) {
  Fr d, e;
  const uint32_t br = fr_raw_sub(d, a, b);
  fr_raw_add(e, d, fr_modulus());
  Fr o;
#pragma unroll
  for (int i = 0; i < 8; ++i) o.l[i] = br ? e.l[i] : d.l[i];
  return o;
}

BLS_HD Fr fr_neg(const Fr& a) { return fr_sub(fr_zero(), a); }

// Montgomery product a b / R mod r (CIOS)
BLS_HD Fr fr_mul(const Fr& a, const Fr& b) {
  const Fr m = fr_modulus();
  uint32_t t[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    uint64_t c = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      c += (uint64_t)t[j] + (uint64_t)a.l[j] * b.l[i];
      t[j] = (uint32_t)c;
      c >>= 32;
    }
    c += t[8];
    t[8] = (uint32_t)c;
    const uint32_t t9 = (uint32_t)(c >> 32);
    const uint32_t q = t[0] * FR_NINV;
    c = ((uint64_t)t[0] + (uint64_t)q * m.l[0]) >> 32;
#pragma unroll
    for (int j = 1; j < 8; ++j) {
      c += (uint64_t)t[j] + (uint64_t)q * m.l[j];
      t[j - 1] = (uint32_t)c;
      c >>= 32;
    }
    c += t[8];
    t[7] = (uint32_t)c;
    t[8] = t9 + (uint32_t)(c >> 32);
  }
  Fr v;
#pragma unroll
  for (int i = 0; i < 8; ++i) v.l[i] = t[i];
  return fr_reduce_once(v);  // t < 2 r, so t[8] = 0
}

BLS_HD Fr fr_sqr(const Fr& a) { return fr_mul(a, a); }

BLS_HD Fr fr_to_mont(const Fr& a) { return fr_mul(a, Fr{{FR_R2_LIMBS}}); }
BLS_HD Fr fr_from_mont(const Fr& a) { return fr_mul(a, Fr{{1, 0, 0, 0, 0, 0, 0, 0}}); }

// a^e, e a 32-bit integer (a^0 = 1)
BLS_HD Fr fr_pow_u32(const Fr& a, uint32_t e) {
  Fr r = fr_one();
#pragma unroll 1
  for (int b = 31; b >= 0; --b) {
    r = fr_sqr(r);
    if ((e >> b) & 1u) r = fr_mul(r, a);
  }
  return r;
}

// 1 / a by Fermat (a^(r - 2)): 256 squarings and 127 products; fr_inv(0) = 0
BLS_HD Fr fr_inv(const Fr& a) {
  const Fr e = Fr{{FR_MOD_M2_LIMBS}};
  Fr r = fr_one();
#pragma unroll
  for (int w = 7; w >= 0; --w) {
    const uint32_t ew = e.l[w];
#pragma unroll 1
    for (int b = 31; b >= 0; --b) {
      r = fr_sqr(r);
      if ((ew >> b) & 1u) r = fr_mul(r, a);
    }
  }
  return r;
}

// the integer of 32 big-endian bytes as raw limbs
BLS_HD Fr fr_raw_from_be32(const uint8_t* in) {
  Fr v;
#pragma unroll
  for (int w = 0; w < 8; ++w) {
    const uint8_t* b = in + 28 - 4 * w;
    v.l[w] = ((uint32_t)b[0] << 24) | ((uint32_t)b[1] << 16) | ((uint32_t)b[2] << 8) | b[3];
  }
  return v;
}

BLS_HD void fr_raw_to_be32(const Fr& v, uint8_t* out) {
#pragma unroll
  for (int w = 0; w < 8; ++w) {
    uint8_t* b = out + 28 - 4 * w;
    b[0] = (uint8_t)(v.l[w] >> 24), b[1] = (uint8_t)(v.l[w] >> 16), b[2] = (uint8_t)(v.l[w] >> 8), b[3] = (uint8_t)v.l[w];
  }
}

// out = the integer of 32 big-endian bytes in Montgomery form; returns whether it is < r (out = 0 when it is not)
BLS_HD bool fr_from_be32(Fr& out, const uint8_t* in) {
  const Fr v = fr_raw_from_be32(in);
  Fr d;
  const bool ok = fr_raw_sub(d, v, fr_modulus()) != 0;
  out = ok ? fr_to_mont(v) : fr_zero();
  return ok;
}

// any integer below 2^256, reduced mod r (hashes, full-width scalars): 2^256 < 3 r
BLS_HD Fr fr_from_be32_reduce(const uint8_t* in) {
  const Fr v = fr_raw_from_be32(in);
  return fr_to_mont(fr_reduce_once(fr_reduce_once(v)));
}

// the canonical residue as 32 big-endian bytes
BLS_HD void fr_to_be32(const Fr& a, uint8_t* out) { fr_raw_to_be32(fr_from_mont(a), out); }

}  // namespace bls
