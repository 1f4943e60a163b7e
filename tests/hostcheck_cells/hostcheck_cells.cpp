// TEST HARNESS ONLY: host build of csrc/bls_fr_ntt.h.  tests/test_cells_host_cpu.py drives the extern "C" functions
// through ctypes, and runs the same cases through the stand-alone program (HC_CELLS_MAIN, built with
// -fsanitize=address,undefined) from a vector file it writes.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "bls_fr_ntt.h"

using namespace bls;

static const Fr* tables() {
  static std::vector<Fr> tab;
  if (tab.empty()) {
    tab.resize(3 * NTT_EXT);
    for (uint32_t i = 0; i < 3 * NTT_EXT; ++i) tab[i] = ntt_table_entry(i);
  }
  return tab.data();
}

// one instance of each inlined piece: the header's functions are force-inlined, and this file calls them often
#define HC_NOINLINE __attribute__((noinline))
static HC_NOINLINE void four_step(const Fr* src, Fr* tmp, Fr* dst, uint32_t logn, uint32_t flags, uint32_t limit) {
  ntt_four_step_array(src, tmp, dst, logn, flags, limit, tables());
}
static HC_NOINLINE void pointwise(const Fr* src, Fr* dst, uint32_t n, bool brp, const Fr* mul, uint32_t mask) {
  for (uint32_t i = 0; i < n; ++i) dst[i] = cells_pointwise(src, i, brp, mul, mask);
}
// zd[m] = Z(w^m), zci[m] = 1 / Z(7 w^m), m < 128; c: 129 entries; returns the degree
static HC_NOINLINE uint32_t vanish(const uint8_t* present, Fr* c, Fr* zd, Fr* zci) {
  const uint32_t deg = cells_vanishing(present, tables(), c);
  for (uint32_t m = 0; m < NTT_CELLS; ++m) {
    zd[m] = cells_vanish_domain(c, deg, tables(), m);
    zci[m] = fr_inv(cells_vanish_coset(c, deg, tables(), m));
  }
  return deg;
}

static bool load(std::vector<Fr>& v, const uint8_t* in, size_t n) {
  v.resize(n);
  for (size_t i = 0; i < n; ++i)
    if (!fr_from_be32(v[i], in + 32 * i)) return false;
  return true;
}
static void store(const std::vector<Fr>& v, uint8_t* out) {
  for (size_t i = 0; i < v.size(); ++i) fr_to_be32(v[i], out + 32 * i);
}

extern "C" {

uint32_t hc_cells_maps_len() { return 64 + 128 + 4096 + 8192; }
// brp6 over 0 .. 63, then brp7, brp12, brp13 over their ranges
void hc_cells_maps(uint32_t* out) {
  for (uint32_t i = 0; i < 64; ++i) *out++ = brp6(i);
  for (uint32_t i = 0; i < 128; ++i) *out++ = brp7(i);
  for (uint32_t i = 0; i < 4096; ++i) *out++ = brp12(i);
  for (uint32_t i = 0; i < 8192; ++i) *out++ = brp13(i);
}

// the constants as integers: w, 1 / 64, 1 / 8192, 7, 1 / 7; then w^8191, 7^8191, 7^-8191 from the tables
void hc_cells_constants(uint8_t* out256) {
  const Fr* tab = tables();
  fr_to_be32(fr_omega_8192(), out256);
  fr_to_be32(fr_inv_64(), out256 + 32);
  fr_to_be32(fr_inv_8192(), out256 + 64);
  fr_to_be32(fr_seven(), out256 + 96);
  fr_to_be32(fr_inv_seven(), out256 + 128);
  fr_to_be32(tab[NTT_EXT - 1], out256 + 160);
  fr_to_be32(tab[2 * NTT_EXT - 1], out256 + 192);
  fr_to_be32(tab[3 * NTT_EXT - 1], out256 + 224);
}

// out = the transform of 2^logl points given in natural order (logl 6 or 7), the inverse scaled by 1 / 2^logl only
// for logl = 6; -1 if an input is not below r
int hc_ntt_sub(uint32_t logl, uint32_t inv, const uint8_t* in, uint8_t* out) {
  if (logl != 6 && logl != 7) return -2;
  const uint32_t n = 1u << logl;
  std::vector<Fr> x, buf(n);
  if (!load(x, in, n)) return -1;
  for (uint32_t i = 0; i < n; ++i) buf[brp_bits(i, logl)] = x[i];
  ntt_sub_array(buf.data(), logl, tables(), inv != 0);
  if (inv && logl == 6)
    for (uint32_t i = 0; i < n; ++i) buf[i] = fr_mul(buf[i], fr_inv_64());
  store(buf, out);
  return 1;
}

// the four-step transform of 2^logn points (logn 12 or 13) with the flags and the limit of bls_fr_ntt.h
int hc_ntt(uint32_t logn, uint32_t flags, uint32_t limit, const uint8_t* in, uint8_t* out) {
  if (logn != 12 && logn != 13) return -2;
  const uint32_t n = 1u << logn;
  std::vector<Fr> x, tmp(n), dst(n);
  if (!load(x, in, n)) return -1;
  four_step(x.data(), tmp.data(), dst.data(), logn, flags, limit);
  store(dst, out);
  return 1;
}

// the 64 coefficients of cell k's interpolation polynomial
int hc_cells_interp(uint32_t k, const uint8_t* cell, uint8_t* out) {
  std::vector<Fr> x;
  if (k >= NTT_CELLS) return -2;
  if (!load(x, cell, NTT_CELL)) return -1;
  cells_interp_array(x.data(), k, tables());
  store(x, out);
  return 1;
}

void hc_cells_shift_pow64(uint32_t k, uint8_t* out32) { fr_to_be32(cells_shift_pow64(tables(), k), out32); }

// the vanishing polynomial of the cells with present[k] = 0: its degree, its 129 coefficients (zero above the
// degree), its values Z(w^m) and the inverses 1 / Z(7 w^m), m < 128
int hc_cells_vanish(const uint8_t* present, uint8_t* coef, uint8_t* zd, uint8_t* zci) {
  std::vector<Fr> c(NTT_CELLS + 1, fr_zero()), d(NTT_CELLS), inv(NTT_CELLS);
  const uint32_t deg = vanish(present, c.data(), d.data(), inv.data());
  for (uint32_t i = deg + 1; i <= NTT_CELLS; ++i) c[i] = fr_zero();
  store(c, coef);
  store(d, zd);
  store(inv, zci);
  return (int)deg;
}

// The recovery as bls_kzg_recover_cells composes it, on one blob: ext_rbo = the 8,192 elements in the spec's order
// with zeros for the missing cells; out = the recovered polynomial's 4,096 coefficients
int hc_cells_recover(const uint8_t* present, const uint8_t* ext_rbo, uint8_t* out_coef) {
  const Fr *W = tables(), *P7 = W + NTT_EXT, *P7I = W + 2 * NTT_EXT;
  std::vector<Fr> x, y(NTT_EXT), t(NTT_EXT), c(NTT_CELLS + 1), zd(NTT_CELLS), zci(NTT_CELLS), coef(NTT_BLOB);
  if (!load(x, ext_rbo, NTT_EXT)) return -1;
  vanish(present, c.data(), zd.data(), zci.data());
  pointwise(x.data(), y.data(), NTT_EXT, true, zd.data(), NTT_CELLS - 1);
  four_step(y.data(), t.data(), y.data(), 13, NTT_INV, NTT_EXT);
  pointwise(y.data(), y.data(), NTT_EXT, false, P7, NTT_EXT - 1);
  four_step(y.data(), t.data(), y.data(), 13, 0, NTT_EXT);
  pointwise(y.data(), y.data(), NTT_EXT, false, zci.data(), NTT_CELLS - 1);
  four_step(y.data(), t.data(), y.data(), 13, NTT_INV, NTT_EXT);
  pointwise(y.data(), coef.data(), NTT_BLOB, false, P7I, NTT_EXT - 1);
  store(coef, out_coef);
  return 1;
}

}  // extern "C"

#ifdef HC_CELLS_MAIN
// Vector file: u32 count of records, each u32 kind and
//   0  maps          want u32[12480]
//   1  sub           u32 logl, u32 inv, in[32 n], want[32 n]
//   2  four-step     u32 logn, u32 flags, u32 limit, in[32 n], want[32 n]
//   3  interpolation u32 k, cell[2048], want[2048]
//   4  vanishing     present[128], i32 want_deg, want coef[129 x 32], zd[128 x 32], zci[128 x 32]
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
    uint32_t kind;
    if (!rd(fh, &kind, 4)) return 2;
    bool ok = false;
    if (kind == 0) {
      std::vector<uint32_t> want(hc_cells_maps_len()), got(hc_cells_maps_len());
      if (!rd(fh, want.data(), 4 * want.size())) return 2;
      hc_cells_maps(got.data());
      ok = want == got;
    } else if (kind == 1 || kind == 2) {
      uint32_t lg, a, limit = 0;
      if (!rd(fh, &lg, 4) || !rd(fh, &a, 4) || (kind == 2 && !rd(fh, &limit, 4)) || lg > 13) return 2;
      const size_t n = (size_t)32 << lg;
      std::vector<uint8_t> in(n), want(n), got(n);
      if (!rd(fh, in.data(), n) || !rd(fh, want.data(), n)) return 2;
      const int rc = kind == 1 ? hc_ntt_sub(lg, a, in.data(), got.data()) : hc_ntt(lg, a, limit, in.data(), got.data());
      ok = rc == 1 && want == got;
    } else if (kind == 3) {
      uint32_t k;
      std::vector<uint8_t> in(2048), want(2048), got(2048);
      if (!rd(fh, &k, 4) || !rd(fh, in.data(), 2048) || !rd(fh, want.data(), 2048)) return 2;
      ok = hc_cells_interp(k, in.data(), got.data()) == 1 && want == got;
    } else if (kind == 4) {
      uint8_t present[128];
      int32_t want_deg;
      std::vector<uint8_t> wc(129 * 32), wd(128 * 32), wi(128 * 32), gc(129 * 32), gd(128 * 32), gi(128 * 32);
      if (!rd(fh, present, 128) || !rd(fh, &want_deg, 4) || !rd(fh, wc.data(), wc.size()) ||
          !rd(fh, wd.data(), wd.size()) || !rd(fh, wi.data(), wi.size()))
        return 2;
      ok = hc_cells_vanish(present, gc.data(), gd.data(), gi.data()) == want_deg && wc == gc && wd == gd && wi == gi;
    } else {
      return 2;
    }
    if (!ok) {
      printf("record %u (kind %u): mismatch\n", c, kind);
      bad++;
    }
  }
  fclose(fh);
  printf("hostcheck_cells: %d mismatches\n", bad);
  return bad ? 1 : 0;
}
#endif
