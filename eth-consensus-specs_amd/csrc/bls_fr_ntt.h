// The number-theoretic transform over F_r (bls_fr.h) for device and host: the index and twiddle maps, the butterfly,
// the sub-transform and the four-step transform under the cell functions of specs/fulu/polynomial-commitments-
// sampling.md (kernels: bls_kzg_cells.hip; C ABI: bls_capi_kzg_cells.hip), and the recovery's vanishing polynomial.
//
// Sizes: 8,192 = the extended blob (128 cells of 64 elements), 4,096 = the blob.  w = 7^((r - 1) / 8192) generates the
// extended domain; every twiddle is an entry of one table W[i] = w^i, i < 8,192 (w_L^j = W[j 8192 / L], and the
// inverse transform's w_L^-j = W[(8192 - j 8192 / L) mod 8192]).
//
// A transform of N = N1 x 64 points (N1 = 64 or 128) is four-step: with n = 64 n1 + c and k = k1 + N1 k2,
//   X[k] = sum_c w_64^(c k2) ( w_N^(c k1) sum_n1 x[64 n1 + c] w_N1^(n1 k1) )
// pass 1 does the 64 inner transforms of length N1 (one per column c) and the twiddle product and leaves
// t[64 k1 + c]; pass 2 does the N1 outer transforms of length 64 (one per row k1).  The bit reversals of the spec's
// orders are folded into pass 1's load (NTT_SRC_BRP) and pass 2's store (NTT_DST_BRP); pass 1's load also pads with
// zeros from `limit` on.  A sub-transform is radix-2 decimation in time on a buffer loaded in bit-reversed order.
//
// Every piece takes (lane, nl): it does the elements lane, lane + nl, ... of its loop.  A wave calls it with its 64
// lanes and a barrier between the pieces; the array versions below call the same pieces with (0, 1), so the host
// build checks exactly what the kernels run (tests/hostcheck_cells).  All loops stay rolled and a lane holds three
// field elements at a time.
#pragma once
#include "bls_fr.h"

namespace bls {

constexpr uint32_t NTT_EXT = 8192;    // FIELD_ELEMENTS_PER_EXT_BLOB
constexpr uint32_t NTT_BLOB = 4096;   // FIELD_ELEMENTS_PER_BLOB
constexpr uint32_t NTT_CELL = 64;     // FIELD_ELEMENTS_PER_CELL
constexpr uint32_t NTT_CELLS = 128;   // CELLS_PER_EXT_BLOB
constexpr uint32_t NTT_SUB_MAX = 128; // the longest sub-transform: a buffer's entries

enum : uint32_t { NTT_INV = 1, NTT_SRC_BRP = 2, NTT_DST_BRP = 4 };

BLS_HD Fr fr_omega_8192() { return Fr{{FR_OMEGA_8192_LIMBS}}; }
BLS_HD Fr fr_inv_64() { return Fr{{FR_INV_64_LIMBS}}; }
BLS_HD Fr fr_inv_8192() { return Fr{{FR_INV_8192_LIMBS}}; }
BLS_HD Fr fr_seven() { return Fr{{FR_SEVEN_LIMBS}}; }
BLS_HD Fr fr_inv_seven() { return Fr{{FR_INV_SEVEN_LIMBS}}; }

// the low `bits` bits of i reversed (1 <= bits <= 32)
BLS_HD uint32_t brp_bits(uint32_t i, uint32_t bits) {
  uint32_t v = i;
  v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
  v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
  v = ((v >> 4) & 0x0f0f0f0fu) | ((v & 0x0f0f0f0fu) << 4);
  v = ((v >> 8) & 0x00ff00ffu) | ((v & 0x00ff00ffu) << 8);
  v = (v >> 16) | (v << 16);
  return v >> (32 - bits);
}
BLS_HD uint32_t brp6(uint32_t i) { return brp_bits(i, 6); }
BLS_HD uint32_t brp7(uint32_t i) { return brp_bits(i, 7); }
BLS_HD uint32_t brp12(uint32_t i) { return brp_bits(i, 12); }
BLS_HD uint32_t brp13(uint32_t i) { return brp_bits(i, 13); }

// W[i] = w^i; P7[i] = 7^i; P7I[i] = 7^-i (i < 8,192): one table of 3 x 8,192 entries, built once per context
BLS_HD Fr ntt_table_entry(uint32_t i) {
  const uint32_t e = i & (NTT_EXT - 1);
  const Fr base = i < NTT_EXT ? fr_omega_8192() : i < 2 * NTT_EXT ? fr_seven() : fr_inv_seven();
  return fr_pow_u32(base, e);
}

// w^idx, or w^-idx for the inverse transform
BLS_HD Fr ntt_tw(const Fr* W, uint32_t idx, bool inv) {
  const uint32_t i = idx & (NTT_EXT - 1);
  return W[inv ? (NTT_EXT - i) & (NTT_EXT - 1) : i];
}

BLS_HD void ntt_butterfly(Fr& a, Fr& b, const Fr& w) {
  const Fr t = fr_mul(b, w);
  b = fr_sub(a, t);
  a = fr_add(a, t);
}

// stage s (1 .. logl) of a sub-transform of 2^logl points on buf (bit-reversed order before stage 1, natural order
// after stage logl): butterfly t pairs i0 = (t >> (s - 1)) 2^s + j and i0 + 2^(s - 1), j = t mod 2^(s - 1), with
// w_(2^s)^j
BLS_HD void ntt_sub_stage(Fr* buf, uint32_t logl, uint32_t s, const Fr* W, bool inv, uint32_t lane, uint32_t nl) {
  const uint32_t half = 1u << (s - 1);
#pragma unroll 1
  for (uint32_t t = lane; t < (1u << (logl - 1)); t += nl) {
    const uint32_t j = t & (half - 1), i0 = ((t >> (s - 1)) << s) + j, i1 = i0 + half;
    Fr a = buf[i0], b = buf[i1];
    ntt_butterfly(a, b, ntt_tw(W, j << (13 - s), inv));
    buf[i0] = a;
    buf[i1] = b;
  }
}

// ---- the four-step maps (n = 2^logn = 2^(logn - 6) x 64) ------------------------------------------------------
// pass 1, column c: element e of the inner transform is x[64 e + c] (zero from `limit` on), at buffer slot brp(e)
BLS_HD void ntt_p1_load(const Fr* src, Fr* buf, uint32_t logn, uint32_t flags, uint32_t limit, uint32_t c,
                        uint32_t lane, uint32_t nl) {
  const uint32_t logn1 = logn - 6;
#pragma unroll 1
  for (uint32_t e = lane; e < (1u << logn1); e += nl) {
    const uint32_t n = (e << 6) + c;
    Fr v = fr_zero();
    if (n < limit) v = src[(flags & NTT_SRC_BRP) ? brp_bits(n, logn) : n];
    buf[brp_bits(e, logn1)] = v;
  }
}
// ... its output k1 times w_n^(c k1) goes to t[64 k1 + c]
BLS_HD void ntt_p1_store(const Fr* buf, Fr* tmp, uint32_t logn, uint32_t flags, const Fr* W, uint32_t c, uint32_t lane,
                         uint32_t nl) {
#pragma unroll 1
  for (uint32_t k1 = lane; k1 < (1u << (logn - 6)); k1 += nl)
    tmp[(k1 << 6) + c] = fr_mul(buf[k1], ntt_tw(W, (c * k1) << (13 - logn), (flags & NTT_INV) != 0));
}
// pass 2, row k1: element c of the outer transform is t[64 k1 + c], at buffer slot brp6(c)
BLS_HD void ntt_p2_load(const Fr* tmp, Fr* buf, uint32_t k1, uint32_t lane, uint32_t nl) {
#pragma unroll 1
  for (uint32_t c = lane; c < 64; c += nl) buf[brp6(c)] = tmp[(k1 << 6) + c];
}
// ... its output k2 is X[k1 + n1 k2] (times 1 / n for the inverse), stored in natural or bit-reversed order
BLS_HD void ntt_p2_store(const Fr* buf, Fr* dst, uint32_t logn, uint32_t flags, uint32_t k1, uint32_t lane,
                         uint32_t nl) {
  const Fr scale = logn == 13 ? fr_inv_8192() : fr_inv_4096();
#pragma unroll 1
  for (uint32_t k2 = lane; k2 < 64; k2 += nl) {
    const uint32_t k = k1 + (k2 << (logn - 6));
    Fr v = buf[k2];
    if (flags & NTT_INV) v = fr_mul(v, scale);
    dst[(flags & NTT_DST_BRP) ? brp_bits(k, logn) : k] = v;
  }
}

// ---- array versions: the same pieces, one lane ----------------------------------------------------------------
// x: 2^logl points (logl <= 7) in bit-reversed order -> the transform in natural order, unscaled
BLS_HD void ntt_sub_array(Fr* x, uint32_t logl, const Fr* W, bool inv) {
#pragma unroll 1
  for (uint32_t s = 1; s <= logl; ++s) ntt_sub_stage(x, logl, s, W, inv, 0, 1);
}

// dst = the transform of src's 2^logn points (logn 12 or 13); tmp: 2^logn entries; dst may be src
BLS_HD void ntt_four_step_array(const Fr* src, Fr* tmp, Fr* dst, uint32_t logn, uint32_t flags, uint32_t limit,
                                const Fr* W) {
  Fr buf[NTT_SUB_MAX];
  const bool inv = (flags & NTT_INV) != 0;
#pragma unroll 1
  for (uint32_t c = 0; c < 64; ++c) {
    ntt_p1_load(src, buf, logn, flags, limit, c, 0, 1);
    ntt_sub_array(buf, logn - 6, W, inv);
    ntt_p1_store(buf, tmp, logn, flags, W, c, 0, 1);
  }
#pragma unroll 1
  for (uint32_t k1 = 0; k1 < (1u << (logn - 6)); ++k1) {
    ntt_p2_load(tmp, buf, k1, 0, 1);
    ntt_sub_array(buf, 6, W, inv);
    ntt_p2_store(buf, dst, logn, flags, k1, 0, 1);
  }
}

// ---- verification: a cell's interpolation polynomial ------------------------------------------------------------
// Cell k's element j is the value at h_k g^brp6(j), h_k = w^brp7(k), g = w^128, so the cell as it stands is the
// sub-transform's bit-reversed input, and the interpolant's coefficients are
//   c_m = h_k^-m / 64 sum_j e_j g^(-m brp6(j)):  the inverse 64-point sub-transform, then this scaling
BLS_HD void cells_interp_scale(Fr* buf, uint32_t k, const Fr* W, uint32_t lane, uint32_t nl) {
  const uint32_t hk = brp7(k & (NTT_CELLS - 1));
#pragma unroll 1
  for (uint32_t m = lane; m < NTT_CELL; m += nl)
    buf[m] = fr_mul(fr_mul(buf[m], fr_inv_64()), ntt_tw(W, hk * m, true));
}
BLS_HD void cells_interp_array(Fr* x, uint32_t k, const Fr* W) {
  ntt_sub_array(x, 6, W, true);
  cells_interp_scale(x, k, W, 0, 1);
}
// h_k^64 = w_128^brp7(k): one of 128 values
BLS_HD Fr cells_shift_pow64(const Fr* W, uint32_t k) { return W[brp7(k & (NTT_CELLS - 1)) << 6]; }

// ---- recovery: the vanishing polynomial ------------------------------------------------------------------------
// S(X) = prod over the missing cells k of (X - w_128^brp7(k)): coef[0 .. deg], deg <= 128 (coef holds 129 entries);
// the spec's vanishing polynomial of the extended domain is Z(X) = S(X^64)
BLS_HD uint32_t cells_vanishing(const uint8_t* present, const Fr* W, Fr* coef) {
  uint32_t deg = 0;
  coef[0] = fr_one();
#pragma unroll 1
  for (uint32_t k = 0; k < NTT_CELLS; ++k) {
    if (present[k]) continue;
    const Fr root = W[brp7(k) << 6];
    coef[deg + 1] = coef[deg];
#pragma unroll 1
    for (uint32_t i = deg; i > 0; --i) coef[i] = fr_sub(coef[i - 1], fr_mul(coef[i], root));
    coef[0] = fr_neg(fr_mul(coef[0], root));
    ++deg;
  }
  return deg;
}

BLS_HD Fr cells_poly_eval(const Fr* coef, uint32_t deg, const Fr& x) {
  Fr acc = coef[deg];
#pragma unroll 1
  for (uint32_t i = deg; i > 0; --i) acc = fr_add(fr_mul(acc, x), coef[i - 1]);
  return acc;
}

// Z on the domain and on the coset 7 x domain takes 128 values each, since Z(X) = S(X^64):
//   Z(w^n) = S(w_128^(n mod 128)),   Z(7 w^n) = S(7^64 w_128^(n mod 128))
BLS_HD Fr cells_vanish_domain(const Fr* coef, uint32_t deg, const Fr* W, uint32_t m) {
  return cells_poly_eval(coef, deg, W[(m & 127u) << 6]);
}
BLS_HD Fr cells_vanish_coset(const Fr* coef, uint32_t deg, const Fr* W, uint32_t m) {
  return cells_poly_eval(coef, deg, fr_mul(fr_pow_u32(fr_seven(), 64), W[(m & 127u) << 6]));
}


// the recovery's pointwise steps: entry i of a blob's 8,192 (taken from the spec's bit-reversed order when brp is
// set) times mul[i & mask] -- the vanishing polynomial's 128 values or inverses, or the 8,192 powers 7^(+-i)
BLS_HD Fr cells_pointwise(const Fr* src, uint32_t i, bool brp, const Fr* mul, uint32_t mask) {
  return fr_mul(src[brp ? brp13(i) : i], mul[i & mask]);
}

}  // namespace bls
