// TEST HARNESS ONLY: host build of the resident G1 table's per-lane pieces (bls_g1_msm.h: the digit split, the run
// folds, the bit sums and the window step that the kernels of bls_g1_table.hip run) with the digit form's 128-bit
// column, value and subtraction-precondition checks compiled in (BLS_FQ_CHECK), for tests/test_g1_table_cpu.py.
#define BLS_FQ_CHECK 1
#define BLS_HD __host__ __device__ inline  // no forced inlining in this (host-only, checked) unit
#include "bls_ops.h"
#include "bls_g1_msm.h"
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

extern "C" uint32_t hc_g1m_k() { return G1M_K; }

extern "C" void hc_g1m_digits(const uint8_t* k32, uint8_t* out32) {
  uint32_t k[8];
  memcpy(k, k32, 32);
  for (int w = 0; w < G1M_WINDOWS; ++w) out32[w] = (uint8_t)g1m_digit(k, w);
}

static G1Q in_pt(const uint32_t* d) {
  G1Q p;
  memcpy(p.x.d, d, 56);
  memcpy(p.y.d, d + 14, 56);
  memcpy(p.z.d, d + 28, 56);
  return p;
}

// One step of a per-lane loop from an accumulator given as raw digits (3 x 14 u32), so that the test sets every
// digit and value at its declared bound; mem: the operand as it lies in memory, three canonical values x || y || z
// (48 B big-endian each).  op 0: a run fold's step over a record (x, y); 1: over a partial (g1q_add_mem);
// 2: a Horner step of the reduction, 2 acc + mem; 3: the window step's eight doublings (acc read as canonical
// packed from mem instead).  out: the result's digits, then its three canonical values (36 u32 limbs, plain).
extern "C" void hc_g1m_step(int op, const uint32_t* acc42, const uint8_t* mem, uint32_t* out_digits,
                            uint8_t* out_be144) {
  const G1Q acc = in_pt(acc42);
  const G1P m{in_fp(mem), in_fp(mem + 48), in_fp(mem + 96)};
  G1Q r;
  if (op == 0) {
    const RegKey rec = record(m.x, m.y);
    // the fold's own loop body: unpack of the record, then the mixed addition
    uint4 w[6];
    memcpy(w, &rec, 96);
    Fp x, y;
    g1m_record_xy(w, x, y);
    r = g1q_add_aff(acc, fq_unpack(x), fq_unpack(y));
  } else if (op == 1) {
    r = g1q_add_mem(acc, &m);
  } else if (op == 2) {
    r = g1q_add(g1q_dbl(acc), g1m_unpack(m));
  } else {
    r = g1m_unpack(g1m_window_step(m));
  }
  memcpy(out_digits, r.x.d, 56);
  memcpy(out_digits + 14, r.y.d, 56);
  memcpy(out_digits + 28, r.z.d, 56);
  const G1P o = g1m_pack(r);
  out_fp(out_be144, o.x);
  out_fp(out_be144 + 48, o.y);
  out_fp(out_be144 + 96, o.z);
}

// The whole MSM as the device runs it, one "lane" at a time: the table's records of all 32 windows by the window
// step, the digit sort, every level of the bucket folds (runs of at most G1M_K, as many levels as the launcher
// runs), the 64 lanes and the tree of each bit sum, and Horner.
// pts: ntab entries x || y (48 B big-endian each); state: 0 invalid, 1 point, 2 identity; k32: B x n scalars.
// out: B affine sums x || y, 96 zero bytes for the identity.  info: {levels, bucket entries, runs of level 0}.
// Returns 0; -1: an index out of range; -2: an invalid entry named.
extern "C" int hc_g1m_msm(const uint8_t* pts, const uint8_t* state, size_t ntab, const uint32_t* idx, size_t n,
                          const uint8_t* k32, size_t B, uint8_t* out, uint32_t* info) {
  for (size_t i = 0; i < n; ++i) {
    if (idx[i] >= ntab) return -1;
    if (!state[idx[i]]) return -2;
  }
  const size_t cap = ntab ? ntab : 1;
  std::vector<RegKey> tab(G1M_WINDOWS * cap, RegKey{fp_zero(), fp_zero(), {0, 0, 0, 0, 0, 0, 0, 0}});
  for (size_t i = 0; i < ntab; ++i) {
    if (state[i] != G1T_POINT) continue;
    G1P cur{in_fp(pts + 96 * i), in_fp(pts + 96 * i + 48), FP_ONE};
    tab[i] = record(cur.x, cur.y);
    for (int w = 1; w < G1M_WINDOWS; ++w) {
      cur = g1m_window_step(cur);
      const Fp zi = fp_inv(cur.z);
      tab[w * cap + i] = record(fp_mul(cur.x, zi), fp_mul(cur.y, zi));
    }
  }
  int levels = 0;
  for (size_t m = n * G1M_WINDOWS;;) {
    m = (m + G1M_K - 1) / G1M_K;
    ++levels;
    if (m <= 1) break;
  }
  info[0] = (uint32_t)levels;
  info[1] = info[2] = 0;
  for (size_t v = 0; v < B; ++v) {
    std::vector<std::vector<uint32_t>> lists(G1M_SLOTS);
    for (size_t i = 0; i < n; ++i) {
      if (state[idx[i]] != G1T_POINT) continue;
      uint32_t k[8];
      memcpy(k, k32 + 32 * (v * n + i), 32);
      for (int w = 0; w < G1M_WINDOWS; ++w) {
        const uint32_t d = g1m_digit(k, w);
        if (d) lists[d].push_back((uint32_t)(w * cap + idx[i]));
      }
    }
    // off / sums as the device leaves them after the last level, for this vector alone (v = 0 below)
    std::vector<uint32_t> off(G1M_SLOTS + 1, 0);
    std::vector<G1P> sums;
    for (uint32_t d = 0; d < G1M_SLOTS; ++d) {
      info[1] += (uint32_t)lists[d].size();
      std::vector<G1P> part;
      for (size_t s = 0; s < lists[d].size(); s += G1M_K) {
        const uint32_t c = (uint32_t)(lists[d].size() - s < G1M_K ? lists[d].size() - s : G1M_K);
        part.push_back(g1m_pack(g1m_fold_records(tab.data(), lists[d].data() + s, c)));
      }
      info[2] += (uint32_t)part.size();
      for (int l = 1; l < levels; ++l) {
        std::vector<G1P> next;
        for (size_t s = 0; s < part.size(); s += G1M_K) {
          const uint32_t c = (uint32_t)(part.size() - s < G1M_K ? part.size() - s : G1M_K);
          next.push_back(g1m_pack(g1m_fold_partials(part.data() + s, c)));
        }
        part.swap(next);
      }
      if (part.size() > 1) return -3;
      off[d] = (uint32_t)sums.size();
      if (!part.empty()) sums.push_back(part[0]);
      off[d + 1] = (uint32_t)sums.size();
    }
    if (sums.empty()) sums.push_back(G1P{fp_zero(), FP_ONE, fp_zero()});
    G1P U[8];
    for (int b = 0; b < 8; ++b) {
      G1Q sh[64];
      for (uint32_t j = 0; j < 64; ++j) sh[j] = g1m_bit_lane(off.data(), sums.data(), 0, b, j);
      for (uint32_t s = 32; s > 0; s >>= 1)
        for (uint32_t j = 0; j < s; ++j) sh[j] = g1q_add(sh[j], sh[j + s]);
      U[b] = g1m_pack(sh[0]);
    }
    const G1P r = g1m_pack(g1m_horner(U));
    memset(out + 96 * v, 0, 96);
    if (fp_is_zero(r.z)) continue;
    const Fp zi = fp_inv(r.z);
    out_fp(out + 96 * v, fp_mul(r.x, zi));
    out_fp(out + 96 * v + 48, fp_mul(r.y, zi));
  }
  return 0;
}
