// The radix-2 transform over G1 for device and host, X[k] = sum_i [w_n^(i k)] x[i] for n = 2^logn <= 4,096 points, and
// the scalar rows of the Fulu cell proofs (kernels: bls_g1_fft.hip; C ABI: bls_capi_kzg_cells.hip).
//
// Schedule: natural-order input, bit-reversed output, in place, one stage per launch.  Stage s (0 .. logn - 1) sees
// the buffer as 2^s blocks of 2 half = n / 2^s entries; block m holds its polynomial modulo X^(2 half) - z^2 and
// splits it modulo X^half - z and X^half + z, z = w_n^(brp_s(m) n / 2^(s + 1)):
//   t = [z] b,   (a, b) <- (a + t, a - t)     for the pairs (i0, i0 + half) of the block
// After the last stage entry i is the value at w_n^brp(i), which is X[brp(i)].  A block's butterflies share one
// twiddle, so the lanes of a wave skip or run the chain together while half >= 64; block 0 of
// every stage has z = 1 and runs no chain (all of stage 0, half of stage 1, ...).  z is an entry of the F_r
// transform's table, W[brp_s(m) 2^(12 - s)] whatever n is (bls_fr_ntt.h: w_n = W[8192 / n]), taken out of Montgomery
// form as eight 32-bit limbs; the inverse transform takes W[8192 - e] and a last pass multiplies by 1 / n.
//
// Points between the stages are canonical projective (G1P, the identity (0 : 1 : 0) allowed anywhere); the chain
// and the two additions are the complete formulas of bls_fq_g1.h on the digit form, under its contract.  The chain
// is bls_g1_endo.h's joint double-and-add at 128 steps: the lane splits its twiddle as z = a + b L, L = x^2 - 1 the
// eigenvalue of the endomorphism's square, by one shift-and-subtract division (g1fft_glv_split), and every step
// doubles and adds one of b, [L] b, b + [L] b by selects -- half the doublings of the plain chain (g1fft_mul, which
// the host check's direct sums keep).  The butterfly adds an unpacked canonical a and the chain's result, whose
// -Y = 64p - Y is bls_g1_endo.h's.
//
// Every piece takes (lane, lanes): it does the elements lane, lane + lanes, ... of its loop.  The kernels call it
// with one lane per element, the host build (tests/hostcheck_g1fft) with (0, 1).
#pragma once
#include "bls_fr_ntt.h"
#include "bls_g1_msm.h"

namespace bls {

constexpr uint32_t G1FFT_LOG_MAX = 12;  // n <= 4,096: every twiddle is an entry of W's first half
constexpr uint32_t CELLPROOF_ROWS = NTT_CELLS / 2 - 1;           // h_0 .. h_62 (h_63 is the identity)
constexpr uint32_t CELLPROOF_ROW_N = NTT_BLOB - NTT_CELL;        // monomial entries 0 .. 4,031
constexpr uint32_t CELLPROOF_FFT_LOG = 7;                        // the 128-point transform of (h_0 .. h_62, O ...)

// ---- index maps ------------------------------------------------------------------------------------------------
// butterfly t (< n / 2) of stage s: its block m and its pair (i0, i1 = i0 + half)
BLS_HD void g1fft_pair(uint32_t logn, uint32_t s, uint32_t t, uint32_t& m, uint32_t& i0, uint32_t& i1) {
  const uint32_t lh = logn - 1 - s;  // log2 of half
  m = t >> lh;
  i0 = (m << (lh + 1)) + (t & ((1u << lh) - 1u));
  i1 = i0 + (1u << lh);
}

// where W holds block m's twiddle of stage s; 0 means z = 1
BLS_HD uint32_t g1fft_tw_index(uint32_t s, uint32_t m, bool inv) {
  const uint32_t e = s ? brp_bits(m, s) << (G1FFT_LOG_MAX - s) : 0u;
  return inv ? (NTT_EXT - e) & (NTT_EXT - 1) : e;
}

// where entry i of the buffer goes after the last stage: X's index for natural order, else i itself
BLS_HD uint32_t g1fft_out_index(uint32_t logn, uint32_t i, bool natural) { return natural ? brp_bits(i, logn) : i; }

// ---- the butterfly ---------------------------------------------------------------------------------------------
BLS_HD G1P g1fft_identity() { return G1P{fp_zero(), FP_ONE, fp_zero()}; }
BLS_HD G1P g1fft_from_aff(const G1A& a) { return a.inf ? g1fft_identity() : G1P{a.x, a.y, FP_ONE}; }

// [k] p for k < 2^255 (eight little-endian limbs): 255 doublings, an addition per set bit.  The plain chain: the
// host check's direct sums run it, the kernels run g1fft_mul_glv below
BLS_HD G1Q g1fft_mul(const G1Q& p, const uint32_t k[8]) {
  G1Q r = g1q_identity();
#pragma unroll 1
  for (int i = 254; i >= 0; --i) {
    r = g1q_dbl(r);
    if ((k[i >> 5] >> (i & 31)) & 1u) r = g1q_add(r, p);
  }
  return r;
}

// k = a + b L for k < r, with L = x^2 - 1 (x the curve parameter; L^2 + L + 1 = r): b = k div L, a = k mod L, both
// non-negative and below 2^128 (b <= L + 1).  A 256-step shift-and-subtract on five-limb remainders; k, a and b are
// shifted through, so nothing is indexed at run time.
BLS_HD void g1fft_glv_split(const uint32_t k[8], uint32_t a[4], uint32_t b[4]) {
  const uint32_t L[5] = {0xffffffffu, 0x00000000u, 0x0001a402u, 0xac45a401u, 0u};
  uint32_t kk[8], rem[5] = {0, 0, 0, 0, 0}, q[4] = {0, 0, 0, 0};
#pragma unroll
  for (int w = 0; w < 8; ++w) kk[w] = k[w];
#pragma unroll 1
  for (int i = 0; i < 256; ++i) {
    const uint32_t bit = kk[7] >> 31;
#pragma unroll
    for (int w = 7; w > 0; --w) kk[w] = (kk[w] << 1) | (kk[w - 1] >> 31);
    kk[0] <<= 1;
#pragma unroll
    for (int w = 4; w > 0; --w) rem[w] = (rem[w] << 1) | (rem[w - 1] >> 31);
    rem[0] = (rem[0] << 1) | bit;
    uint32_t t[5], borrow = 0;
#pragma unroll
    for (int w = 0; w < 5; ++w) {
      const uint64_t d = (uint64_t)rem[w] - L[w] - borrow;
      t[w] = (uint32_t)d;
      borrow = (uint32_t)(d >> 63);
    }
    const bool ge = borrow == 0;
#pragma unroll
    for (int w = 0; w < 5; ++w) rem[w] = ge ? t[w] : rem[w];
#pragma unroll
    for (int w = 3; w > 0; --w) q[w] = (q[w] << 1) | (q[w - 1] >> 31);
    q[0] = (q[0] << 1) | (ge ? 1u : 0u);
  }
#pragma unroll
  for (int w = 0; w < 4; ++w) a[w] = rem[w], b[w] = q[w];
}

// [k] A for k < r through the endomorphism, bls_g1_endo.h's joint chain at 128 steps: phi(x, y) = (beta x, y) is
// [lambda] with lambda = -x^2 = L^2 mod r, so [L] A = phi^2(A) = (beta^2 X : Y : Z) and, 1 + L + L^2 being 0,
// A + [L] A = -phi(A) = (beta X : -Y : Z); [k] A = a A + b [L] A.  A: unpacked canonical coordinates; the bounds of
// the table operand are g1q_mul_endo's, and the addition is computed at every step and chosen by selects.
BLS_HD G1Q g1fft_mul_glv(const G1Q& A, const uint32_t k[8]) {
  uint32_t a[4], b[4];
  g1fft_glv_split(k, a, b);
  const Fq beta = fq_unpack(FP_BETA);
  const Fq x1 = fq_mul(A.x, beta);
  const Fq x2 = fq_mul(x1, beta);
  const Fq yn = fq_norm(fq_sub(fq_zero(), A.y));
  G1Q R = g1q_identity();
#pragma unroll 1
  for (int i = 0; i < 128; ++i) {
    R = g1q_dbl(R);
    const uint32_t d = (a[3] >> 31) | ((b[3] >> 31) << 1);
#pragma unroll
    for (int w = 3; w > 0; --w) {
      a[w] = (a[w] << 1) | (a[w - 1] >> 31);
      b[w] = (b[w] << 1) | (b[w - 1] >> 31);
    }
    a[0] <<= 1;
    b[0] <<= 1;
    const G1Q T{fq_select(d == 3u, x1, fq_select(d == 2u, x2, A.x)), fq_select(d == 3u, yn, A.y), A.z};
    const G1Q S = g1q_add(R, T);
    R = G1Q{fq_select(d != 0u, S.x, R.x), fq_select(d != 0u, S.y, R.y), fq_select(d != 0u, S.z, R.z)};
  }
  return R;
}

// t = [k] b (b itself when unit, or when b is the identity); (a, b) <- (a + t, a - t)
BLS_HD void g1fft_butterfly(G1P& a, G1P& b, const uint32_t k[8], bool unit) {
  const G1Q A = g1m_unpack(a);
  G1Q T = g1m_unpack(b);
  if (!unit && !fp_is_zero(b.z)) T = g1fft_mul_glv(T, k);
  const G1Q Tn{T.x, fq_norm(fq_sub(fq_zero(), T.y)), T.z};
  a = g1m_pack(g1q_add(A, T));
  b = g1m_pack(g1q_add(A, Tn));
}

// stage s of B transforms of 2^logn points each, vector v at buf + (v << logn)
BLS_HD void g1fft_stage(G1P* buf, uint32_t logn, uint32_t s, size_t B, const Fr* W, bool inv, size_t lane,
                        size_t lanes) {
  const size_t total = B << (logn - 1);
#pragma unroll 1
  for (size_t g = lane; g < total; g += lanes) {
    G1P* x = buf + ((g >> (logn - 1)) << logn);
    uint32_t m, i0, i1;
    g1fft_pair(logn, s, (uint32_t)(g & ((1u << (logn - 1)) - 1u)), m, i0, i1);
    const uint32_t e = g1fft_tw_index(s, m, inv);
    const Fr k = fr_from_mont(W[e]);
    G1P a = x[i0], b = x[i1];
    g1fft_butterfly(a, b, k.l, e == 0);
    x[i0] = a;
    x[i1] = b;
  }
}

// the inverse transform's last pass: every entry times 1 / n
BLS_HD void g1fft_scale(G1P* buf, uint32_t logn, size_t B, size_t lane, size_t lanes) {
  const Fr k = fr_from_mont(fr_inv(fr_to_mont(Fr{{1u << logn, 0, 0, 0, 0, 0, 0, 0}})));
#pragma unroll 1
  for (size_t g = lane; g < (B << logn); g += lanes) {
    if (fp_is_zero(buf[g].z)) continue;
    buf[g] = g1m_pack(g1fft_mul_glv(g1m_unpack(buf[g]), k.l));
  }
}

// the whole transform on one lane: x natural order in, natural or bit-reversed order out (tmp: n entries)
BLS_HD void g1fft_array(G1P* x, G1P* tmp, uint32_t logn, bool inv, bool natural, const Fr* W) {
#pragma unroll 1
  for (uint32_t s = 0; s < logn; ++s) g1fft_stage(x, logn, s, 1, W, inv, 0, 1);
  if (inv) g1fft_scale(x, logn, 1, 0, 1);
#pragma unroll 1
  for (uint32_t i = 0; i < (1u << logn); ++i) tmp[g1fft_out_index(logn, i, natural)] = x[i];
#pragma unroll 1
  for (uint32_t i = 0; i < (1u << logn); ++i) x[i] = tmp[i];
}

// ---- cell proofs -------------------------------------------------------------------------------------------------
// The proof of cell k commits to (p - I_k) / (X^64 - a_k), a_k = w_128^brp7(k).  X^n / (X^64 - a) has the polynomial
// part sum_m a^m X^(n - 64 (m + 1)), so with p = sum f_i X^i
//   pi_k = sum_{m < 64} [a_k^m] h_m,   h_m = sum_{i < 4096 - 64 (m + 1)} f_{i + 64 (m + 1)} [tau^i] G1   (h_63 = O)
// The h_m are rows of the table MSM over the monomial entries 0 .. 4,031: row m is the coefficient vector shifted
// down by 64 (m + 1) and zero above; the pi_k in the spec's order are the bit-reversed-order output of the forward
// 128-point transform of (h_0 .. h_62, O, ..., O).
BLS_HD Fr cellproof_row_entry(const Fr* coef, uint32_t m, uint32_t i) {
  const uint32_t j = i + NTT_CELL * (m + 1);
  return j < NTT_BLOB ? coef[j] : fr_zero();
}

}  // namespace bls
