// TEST HARNESS ONLY: host build of the per-lane pieces of the bucket MSM over a call's own points
// (bls_g1_var_msm.h: the (row, window, digit) slots and the window chain, with the run folds, bit sums and Horner of
// bls_g1_msm.h that its kernels share with the resident table) with the digit form's 128-bit column, value and
// subtraction-precondition checks compiled in (BLS_FQ_CHECK), for tests/test_g1_var_msm_cpu.py.
#define BLS_FQ_CHECK 1
#define BLS_HD __host__ __device__ inline  // no forced inlining in this (host-only, checked) unit
#include "bls_ops.h"
#include "bls_g1_var_msm.h"
#include <string.h>
#include <vector>
using namespace bls;

static Fp in_fp(const uint8_t* b) { return fp_to_mont(raw_from_be48(b)); }
static void out_fp(uint8_t* b, const Fp& a) { raw_to_be48(fp_from_mont(a), b); }
static RegKey record(const Fp& x, const Fp& y) {
  RegKey e{x, y, {0, 0, 0, 0, 0, 0, 0, 0}};
  e.x.l[11] |= REG_VALID;
  return e;
}
static G1P in_g1p(const uint8_t* m) { return G1P{in_fp(m), in_fp(m + 48), in_fp(m + 96)}; }
static void out_g1p(uint8_t* b, const G1P& o) {
  out_fp(b, o.x);
  out_fp(b + 48, o.y);
  out_fp(b + 96, o.z);
}

extern "C" uint32_t hc_g1vm_k() { return G1M_K; }

// the slots the sort's lane of (row v, scalar k32) visits, in order; returns their number
extern "C" uint32_t hc_g1vm_slots(const uint8_t* k32, uint32_t v, uint32_t* out32) {
  uint32_t k[8], c = 0;
  memcpy(k, k32, 32);
  g1vm_each_slot(k, v, [&](uint32_t slot) { out32[c++] = slot; });
  return c;
}

// One step of the window chain from an accumulator given as raw digits (3 x 14 u32), so that the test sets every
// digit and value at its declared bound: eight g1q_dbl, then g1q_add with the canonical window sum mem
// (x || y || z, 48 B big-endian each).  out: the result's digits, then its three canonical values.
extern "C" void hc_g1vm_step(const uint32_t* acc42, const uint8_t* mem, uint32_t* out_digits, uint8_t* out_be144) {
  G1Q r;
  memcpy(r.x.d, acc42, 56);
  memcpy(r.y.d, acc42 + 14, 56);
  memcpy(r.z.d, acc42 + 28, 56);
  for (int i = 0; i < 8; ++i) r = g1q_dbl(r);
  r = g1q_add(r, g1m_unpack(in_g1p(mem)));
  memcpy(out_digits, r.x.d, 56);
  memcpy(out_digits + 14, r.y.d, 56);
  memcpy(out_digits + 28, r.z.d, 56);
  out_g1p(out_be144, g1m_pack(r));
}

// g1vm_combine over 32 canonical window sums (144 B each); returns the window it started from
extern "C" int hc_g1vm_combine(const uint8_t* w_be, uint8_t* out_be144) {
  G1P W[G1M_WINDOWS];
  for (int w = 0; w < G1M_WINDOWS; ++w) W[w] = in_g1p(w_be + 144 * w);
  out_g1p(out_be144, g1m_pack(g1vm_combine(W)));
  return g1vm_top_window(W);
}

// The whole MSM as the device runs it, one "lane" at a time: the points' records, the sort into the slots of
// g1vm_each_slot, every level of the bucket folds (as many levels as the launcher runs for buckets of at most n
// entries), the 64 lanes and the tree of each bit sum and Horner per (row, window), then the window chain per row.
// pts: n points x || y (48 B big-endian each); state: 1 point, 2 identity; k32: B x n scalars.
// out: B affine sums x || y, 96 zero bytes for the identity.  info: {levels, bucket entries, runs of level 0}.
// Returns 0; -3: a bucket was left with more than one partial.
extern "C" int hc_g1vm_msm(const uint8_t* pts, const uint8_t* state, size_t n, const uint8_t* k32, size_t B,
                           uint8_t* out, uint32_t* info) {
  std::vector<RegKey> rec(n ? n : 1, RegKey{fp_zero(), fp_zero(), {0, 0, 0, 0, 0, 0, 0, 0}});
  for (size_t i = 0; i < n; ++i)
    if (state[i] == G1T_POINT) rec[i] = record(in_fp(pts + 96 * i), in_fp(pts + 96 * i + 48));
  int levels = 0;
  for (size_t m = n;;) {
    m = (m + G1M_K - 1) / G1M_K;
    ++levels;
    if (m <= 1) break;
  }
  info[0] = (uint32_t)levels;
  info[1] = info[2] = 0;
  const size_t N = B * G1M_WINDOWS * G1M_SLOTS;
  std::vector<std::vector<uint32_t>> lists(N);
  for (size_t v = 0; v < B; ++v)
    for (size_t i = 0; i < n; ++i) {
      if (state[i] != G1T_POINT) continue;
      uint32_t k[8];
      memcpy(k, k32 + 32 * (v * n + i), 32);
      g1vm_each_slot(k, (uint32_t)v, [&](uint32_t slot) { lists[slot].push_back((uint32_t)i); });
    }
  // off / sums as the device leaves them after the last level
  std::vector<uint32_t> off(N + 1, 0);
  std::vector<G1P> sums;
  for (size_t s_ = 0; s_ < N; ++s_) {
    const std::vector<uint32_t>& l = lists[s_];
    info[1] += (uint32_t)l.size();
    std::vector<G1P> part;
    for (size_t s = 0; s < l.size(); s += G1M_K) {
      const uint32_t c = (uint32_t)(l.size() - s < G1M_K ? l.size() - s : G1M_K);
      part.push_back(g1m_pack(g1m_fold_records(rec.data(), l.data() + s, c)));
    }
    info[2] += (uint32_t)part.size();
    for (int lv = 1; lv < levels; ++lv) {
      std::vector<G1P> next;
      for (size_t s = 0; s < part.size(); s += G1M_K) {
        const uint32_t c = (uint32_t)(part.size() - s < G1M_K ? part.size() - s : G1M_K);
        next.push_back(g1m_pack(g1m_fold_partials(part.data() + s, c)));
      }
      part.swap(next);
    }
    if (part.size() > 1) return -3;
    off[s_] = (uint32_t)sums.size();
    if (!part.empty()) sums.push_back(part[0]);
    off[s_ + 1] = (uint32_t)sums.size();
  }
  if (sums.empty()) sums.push_back(G1P{fp_zero(), FP_ONE, fp_zero()});
  for (size_t v = 0; v < B; ++v) {
    G1P W[G1M_WINDOWS];
    for (int w = 0; w < G1M_WINDOWS; ++w) {
      const uint32_t g = (uint32_t)(v * G1M_WINDOWS + w);
      G1P U[8];
      for (int b = 0; b < 8; ++b) {
        G1Q sh[64];
        for (uint32_t j = 0; j < 64; ++j) sh[j] = g1m_bit_lane(off.data(), sums.data(), g, b, j);
        for (uint32_t s = 32; s > 0; s >>= 1)
          for (uint32_t j = 0; j < s; ++j) sh[j] = g1q_add(sh[j], sh[j + s]);
        U[b] = g1m_pack(sh[0]);
      }
      W[w] = g1m_pack(g1m_horner(U));
    }
    const G1P r = g1m_pack(g1vm_combine(W));
    memset(out + 96 * v, 0, 96);
    if (fp_is_zero(r.z)) continue;
    const Fp zi = fp_inv(r.z);
    out_fp(out + 96 * v, fp_mul(r.x, zi));
    out_fp(out + 96 * v + 48, fp_mul(r.y, zi));
  }
  return 0;
}
