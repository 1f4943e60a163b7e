// Resident G1 table and its bucket MSM (bls_g1_table_*; kernels in bls_g1_table.hip): the per-lane pieces, which the
// kernels and the host check (tests/hostcheck_g1msm, with BLS_FQ_CHECK) both run.
//
// The table keeps, per entry P, the 32 window multiples 2^(8w) P as affine RegKey records (128 B, REG_VALID set on a
// usable non-identity point), window-major: record w * cap + i.  A 256-bit scalar k = sum_w d_w 2^(8w) then gives
// [k] P = sum_w [d_w] (2^(8w) P): an MSM is additions only.  The non-zero digits of a vector's scalars are sorted
// into its 255 buckets (v, d) as record numbers; a bucket's sum S_d is a levelled fold of runs of at most G1M_K
// entries; sum_d d S_d = sum_b 2^b U_b with U_b the sum of the buckets whose digit has bit b.
//
// Bounds (bls_fq_g1.h's accumulator contract; every formula called here is bound-typed or is g1q_add_mem of
// bls_g1_segsum.h, whose bounds are written there):
//   run fold over records   the accumulator starts at the identity in N form and is then an output of g1q_add_aff;
//                           the operand is a record, canonical (< p, N form): k_fav_gather_q's inner loop
//   run fold over partials  seg_fold_partials: outputs of g1q_add_mem, operand a canonical packed partial
//   bit sums, Horner        g1q_add / g1q_dbl on unpacked canonical points and on their own outputs (g1q_dbl's
//                           X3 < 4p is inside g1q_add's 66p)
//   window step             eight g1q_dbl from an unpacked canonical point; each output is an input again
#pragma once
#include "bls_curve.h"
#include "bls_fq_g1.h"
#include "bls_g1_segsum.h"

namespace bls {

constexpr uint32_t G1M_K = 16;       // entries per run
constexpr int G1M_WINDOWS = 32;      // 8-bit windows of a 256-bit scalar
constexpr uint32_t G1M_SLOTS = 256;  // bucket slots per vector: slot d holds digit d, slot 0 stays empty
// an entry's state (the table's side array; REG_VALID of its records is set for G1T_POINT only)
constexpr uint8_t G1T_INVALID = 0, G1T_POINT = 1, G1T_IDENTITY = 2;

// digit w (weight 2^(8w)) of a 256-bit big-endian scalar held as the eight 32-bit words it occupies in memory
BLS_HD uint32_t g1m_digit(const uint32_t k[8], int w) {
  const int j = 31 - w;  // byte j of the big-endian string
  return (k[j >> 2] >> (8 * (j & 3))) & 0xffu;
}

// the j-th (j < 128) digit with bit b set
BLS_HD uint32_t g1m_bit_digit(int b, uint32_t j) { return ((j >> b) << (b + 1)) | (1u << b) | (j & ((1u << b) - 1u)); }

BLS_HD G1P g1m_pack(const G1Q& a) { return G1P{fq_pack(a.x), fq_pack(a.y), fq_pack(a.z)}; }
BLS_HD G1Q g1m_unpack(const G1P& a) { return G1Q{fq_unpack(a.x), fq_unpack(a.y), fq_unpack(a.z)}; }

// (x, y) of a usable record
BLS_HD void g1m_record_xy(const uint4 (&r)[6], Fp& x, Fp& y) {
#pragma unroll
  for (int w = 0; w < 3; ++w) {
    x.l[4 * w] = r[w].x, x.l[4 * w + 1] = r[w].y, x.l[4 * w + 2] = r[w].z, x.l[4 * w + 3] = r[w].w;
    y.l[4 * w] = r[3 + w].x, y.l[4 * w + 1] = r[3 + w].y, y.l[4 * w + 2] = r[3 + w].z, y.l[4 * w + 3] = r[3 + w].w;
  }
  x.l[11] &= ~REG_VALID;
}

// The fold of one run of a bucket's list: cnt <= G1M_K record numbers at lst, every one a usable record (the sort
// drops identity entries and the call refuses invalid ones).  The next record is in flight while this one is added,
// as in k_fav_gather_q; the last step loads the last record again.
BLS_HD G1Q g1m_fold_records(const RegKey* tab, const uint32_t* lst, uint32_t cnt) {
  G1Q acc = g1q_identity();
  if (!cnt) return acc;
  uint4 r[6];
  {
    const uint4* p = reinterpret_cast<const uint4*>(tab + lst[0]);
#pragma unroll
    for (int w = 0; w < 6; ++w) r[w] = p[w];
  }
  uint32_t nxt = cnt > 1 ? lst[1] : lst[0];
#pragma unroll 1
  for (uint32_t k = 0; k < cnt; ++k) {
    uint4 cr[6];
#pragma unroll
    for (int w = 0; w < 6; ++w) cr[w] = r[w];
    const uint4* p = reinterpret_cast<const uint4*>(tab + nxt);
#pragma unroll
    for (int w = 0; w < 6; ++w) r[w] = p[w];
    nxt = k + 2 < cnt ? lst[k + 2] : nxt;
    Fp x, y;
    g1m_record_xy(cr, x, y);
    acc = g1q_add_aff(acc, fq_unpack(x), fq_unpack(y));
  }
  return acc;
}

// the fold of one run of cnt <= G1M_K partials of the level below
BLS_HD G1Q g1m_fold_partials(const G1P* prev, uint32_t cnt) { return seg_fold_partials(SegRun{0, cnt, 0}, prev); }

// Lane j < 64 of the bit sum U_{v,b}: the sums of the buckets of digits g1m_bit_digit(b, j) and (b, j + 64).  After
// the last level a bucket's sum is sums[off[slot]] when off[slot + 1] > off[slot], else the identity.  The 64 lane
// sums are then folded by a tree of g1q_add.
BLS_HD G1Q g1m_bit_lane(const uint32_t* off, const G1P* sums, uint32_t v, int b, uint32_t j) {
  G1Q acc = g1q_identity();
#pragma unroll 1
  for (uint32_t t = 0; t < 2; ++t) {
    const uint32_t slot = v * G1M_SLOTS + g1m_bit_digit(b, j + 64 * t);
    const uint32_t o = off[slot];
    if (off[slot + 1] > o) acc = g1q_add(acc, g1m_unpack(sums[o]));
  }
  return acc;
}

// sum_b 2^b U_b over the eight bit sums of one vector
BLS_HD G1Q g1m_horner(const G1P* U) {
  G1Q r = g1m_unpack(U[7]);
#pragma unroll 1
  for (int b = 6; b >= 0; --b) r = g1q_add(g1q_dbl(r), g1m_unpack(U[b]));
  return r;
}

// the next window multiple of the load: 2^8 P in projective coordinates, canonical
BLS_HD G1P g1m_window_step(const G1P& p) {
  G1Q a = g1m_unpack(p);
#pragma unroll 1
  for (int i = 0; i < 8; ++i) a = g1q_dbl(a);
  return g1m_pack(a);
}

}  // namespace bls
