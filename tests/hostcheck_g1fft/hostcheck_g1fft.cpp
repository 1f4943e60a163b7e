// TEST HARNESS ONLY: host build of csrc/bls_g1_fft.h.  tests/test_g1fft_host_cpu.py drives the extern "C" functions
// through ctypes, and runs the same cases through the stand-alone program (HC_G1FFT_MAIN, built with
// -fsanitize=address,undefined) from a vector file it writes.
#ifndef BLS_HD
#define BLS_HD __host__ __device__ inline  // no forced inlining in this host-only unit
#endif
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "bls_ops.h"
#include "bls_g1_fft.h"

using namespace bls;

static const Fr* tables() {
  static std::vector<Fr> tab;
  if (tab.empty()) {
    tab.resize(NTT_EXT);
    for (uint32_t i = 0; i < NTT_EXT; ++i) tab[i] = ntt_table_entry(i);
  }
  return tab.data();
}

static bool load(std::vector<G1P>& v, const uint8_t* in48, size_t n) {
  v.resize(n);
  for (size_t i = 0; i < n; ++i) {
    G1A a{fp_zero(), fp_zero(), true};
    const int d = g1_decompress(a, in48 + 48 * i);
    if (d != DEC_OK && d != DEC_INFINITY) return false;
    if (d == DEC_INFINITY) a = G1A{fp_zero(), fp_zero(), true};
    v[i] = g1fft_from_aff(a);
  }
  return true;
}
static void store(const std::vector<G1P>& v, uint8_t* out48) {
  for (size_t i = 0; i < v.size(); ++i) {
    G1A a{fp_zero(), fp_zero(), true};
    if (!fp_is_zero(v[i].z)) {
      const Fp zi = fp_inv(v[i].z);
      a = G1A{fp_mul(v[i].x, zi), fp_mul(v[i].y, zi), false};
    }
    g1_compress(out48 + 48 * i, a);
  }
}

extern "C" {

uint32_t hc_g1fft_maps_len(uint32_t logn) { return 5u * logn << (logn - 1); }
// per stage and butterfly: block, i0, i1, the twiddle's forward and inverse table index
void hc_g1fft_maps(uint32_t logn, uint32_t* out) {
  for (uint32_t s = 0; s < logn; ++s)
    for (uint32_t t = 0; t < (1u << (logn - 1)); ++t) {
      uint32_t m, i0, i1;
      g1fft_pair(logn, s, t, m, i0, i1);
      *out++ = m, *out++ = i0, *out++ = i1;
      *out++ = g1fft_tw_index(s, m, false);
      *out++ = g1fft_tw_index(s, m, true);
    }
}
// where the buffer's entries go: natural order, then as they stand
void hc_g1fft_out_index(uint32_t logn, uint32_t* out) {
  for (uint32_t i = 0; i < (1u << logn); ++i) *out++ = g1fft_out_index(logn, i, true);
  for (uint32_t i = 0; i < (1u << logn); ++i) *out++ = g1fft_out_index(logn, i, false);
}
// every (stage, block)'s twiddle as the chain reads it: out of Montgomery form, 32 big-endian bytes
void hc_g1fft_twiddles(uint32_t logn, uint32_t inv, uint8_t* out32) {
  for (uint32_t s = 0; s < logn; ++s)
    for (uint32_t m = 0; m < (1u << s); ++m, out32 += 32)
      fr_raw_to_be32(fr_from_mont(tables()[g1fft_tw_index(s, m, inv != 0)]), out32);
}

// the transform of 2^logn compressed points (natural order in; natural or bit-reversed order out); -1: an encoding
int hc_g1fft(uint32_t logn, uint32_t inv, uint32_t natural, const uint8_t* in48, uint8_t* out48) {
  if (logn < 1 || logn > G1FFT_LOG_MAX) return -2;
  std::vector<G1P> x, tmp((size_t)1 << logn);
  if (!load(x, in48, (size_t)1 << logn)) return -1;
  g1fft_array(x.data(), tmp.data(), logn, inv != 0, natural != 0, tables());
  store(x, out48);
  return 1;
}

// out[k] = sum_i [w_n^(i k)] in[i] in natural order, every term its own chain and every sum a complete addition
int hc_g1fft_direct(uint32_t logn, const uint8_t* in48, uint8_t* out48) {
  if (logn < 1 || logn > G1FFT_LOG_MAX) return -2;
  const uint32_t n = 1u << logn;
  std::vector<G1P> x, out(n);
  if (!load(x, in48, n)) return -1;
  for (uint32_t k = 0; k < n; ++k) {
    G1Q acc = g1q_identity();
    for (uint32_t i = 0; i < n; ++i) {
      if (fp_is_zero(x[i].z)) continue;
      const Fr e = fr_from_mont(tables()[((i * k) & (n - 1)) << (13 - logn)]);
      acc = g1q_add(g1m_unpack(g1m_pack(acc)), g1fft_mul(g1m_unpack(x[i]), e.l));
    }
    out[k] = g1m_pack(acc);
  }
  store(out, out48);
  return 1;
}

// k = a + b L: a, b as 16 big-endian bytes each
void hc_g1fft_split(const uint8_t* k32, uint8_t* a16, uint8_t* b16) {
  const Fr k = fr_raw_from_be32(k32);
  uint32_t a[4], b[4];
  g1fft_glv_split(k.l, a, b);
  for (int i = 0; i < 16; ++i) {
    a16[i] = (uint8_t)(a[3 - i / 4] >> (8 * (3 - i % 4)));
    b16[i] = (uint8_t)(b[3 - i / 4] >> (8 * (3 - i % 4)));
  }
}

// [k] P by the plain chain (glv = 0) or through the endomorphism (glv = 1); -1: an encoding
int hc_g1fft_mul(uint32_t glv, const uint8_t* p48, const uint8_t* k32, uint8_t* out48) {
  std::vector<G1P> x;
  if (!load(x, p48, 1)) return -1;
  const Fr k = fr_raw_from_be32(k32);
  const G1Q r = glv ? g1fft_mul_glv(g1m_unpack(x[0]), k.l) : g1fft_mul(g1m_unpack(x[0]), k.l);
  x[0] = g1m_pack(r);
  store(x, out48);
  return 1;
}

// row m of the cell proofs' MSM from 4,096 coefficients: 4,032 scalars
int hc_cellproof_row(const uint8_t* coef32, uint32_t m, uint8_t* out32) {
  std::vector<Fr> c(NTT_BLOB);
  for (uint32_t i = 0; i < NTT_BLOB; ++i)
    if (!fr_from_be32(c[i], coef32 + 32 * i)) return -1;
  if (m >= CELLPROOF_ROWS) return -2;
  for (uint32_t i = 0; i < CELLPROOF_ROW_N; ++i) fr_to_be32(cellproof_row_entry(c.data(), m, i), out32 + 32 * i);
  return 1;
}

}  // extern "C"

#ifdef HC_G1FFT_MAIN
// Vector file: u32 count of records, each u32 kind and
//   0  maps       u32 logn, want u32[hc_g1fft_maps_len], want u32[2 n] (the output order)
//   1  twiddles   u32 logn, u32 inv, want[32 (n - 1)]
//   2  transform  u32 logn, u32 inv, u32 natural, in[48 n], want[48 n]
//   3  product    u32 1 (in logn's place), point[48], k[32], want a[16], b[16] (the split), want[48]: both chains
// Exit status 0 iff everything matches.
static bool rd(FILE* fh, void* p, size_t n) { return fread(p, 1, n, fh) == n; }

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* fh = fopen(argv[1], "rb");
  if (!fh) return 2;
  int bad = 0;
  uint32_t count = 0;
  if (!rd(fh, &count, 4)) return 2;
  for (uint32_t c = 0; c < count; ++c) {
    uint32_t kind, logn;
    if (!rd(fh, &kind, 4) || !rd(fh, &logn, 4) || logn < 1 || logn > G1FFT_LOG_MAX) return 2;
    const size_t n = (size_t)1 << logn;
    bool ok = false;
    if (kind == 0) {
      std::vector<uint32_t> want(hc_g1fft_maps_len(logn)), got(want.size()), wo(2 * n), go(2 * n);
      if (!rd(fh, want.data(), 4 * want.size()) || !rd(fh, wo.data(), 4 * wo.size())) return 2;
      hc_g1fft_maps(logn, got.data());
      hc_g1fft_out_index(logn, go.data());
      ok = want == got && wo == go;
    } else if (kind == 1) {
      uint32_t inv;
      std::vector<uint8_t> want(32 * (n - 1)), got(32 * (n - 1));
      if (!rd(fh, &inv, 4) || !rd(fh, want.data(), want.size())) return 2;
      hc_g1fft_twiddles(logn, inv, got.data());
      ok = want == got;
    } else if (kind == 2) {
      uint32_t inv, natural;
      std::vector<uint8_t> in(48 * n), want(48 * n), got(48 * n);
      if (!rd(fh, &inv, 4) || !rd(fh, &natural, 4) || !rd(fh, in.data(), in.size()) ||
          !rd(fh, want.data(), want.size()))
        return 2;
      ok = hc_g1fft(logn, inv, natural, in.data(), got.data()) == 1 && want == got;
    } else if (kind == 3) {
      uint8_t p[48], k[32], wa[16], wb[16], want[48], ga[16], gb[16], g0[48], g1[48];
      if (!rd(fh, p, 48) || !rd(fh, k, 32) || !rd(fh, wa, 16) || !rd(fh, wb, 16) || !rd(fh, want, 48)) return 2;
      hc_g1fft_split(k, ga, gb);
      ok = hc_g1fft_mul(0, p, k, g0) == 1 && hc_g1fft_mul(1, p, k, g1) == 1 && !memcmp(ga, wa, 16) &&
           !memcmp(gb, wb, 16) && !memcmp(g0, want, 48) && !memcmp(g1, want, 48);
    } else {
      return 2;
    }
    if (!ok) {
      printf("record %u (kind %u): mismatch\n", c, kind);
      bad++;
    }
  }
  fclose(fh);
  printf("hostcheck_g1fft: %d mismatches\n", bad);
  return bad ? 1 : 0;
}
#endif
