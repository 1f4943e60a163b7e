// Segmented G1 sum of a shared-message FAV batch: gsum[m] = sum of r_i apk_i over the live items i with
// msg_id[i] == m, so that the batch equation takes one (gsum[m], H(m)) Miller pair per distinct message
// (bilinearity: prod_i e(r_i apk_i, H(m)) = e(sum_i r_i apk_i, H(m))).
//
// Group sizes are as skewed as they can be (all singletons, or one group holding the whole batch), so the sum is
// a levelled fold: the host cuts every group into runs of at most SEG_K consecutive entries, one lane folds one
// run, and the next level folds each group's run partials the same way until every group has one partial --
// ceil(log_K(largest group)) launches of k_g1_seg_fold (bls_segsum.hip), one when every group fits a run.
//
// Part 1 (the plan) is plain C++ with no HIP types; part 2 (the per-lane fold) is the code the kernel and the
// host check (tests/hostcheck_segsum, with BLS_FQ_CHECK) both run.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

namespace bls {

constexpr uint32_t SEG_K = 16;                 // entries per run
constexpr uint32_t SEG_FINAL = 0x80000000u;    // SegRun::dst: the run's sum is its group's (dst & ~SEG_FINAL)

// One lane's work.  Level 0: entries grp_items[src .. src + cnt) (item numbers); above: partials
// prev[src .. src + cnt) of the level below.  dst: the group (| SEG_FINAL) when this run is all that is left of
// it, else the slot of this level's partial array.  cnt == 0 only for an unused table entry (level 0, final).
struct SegRun {
  uint32_t src, cnt, dst;
};

struct SegPlan {
  std::vector<uint32_t> grp_offs;   // M + 1: group m's items are grp_items[grp_offs[m] .. grp_offs[m + 1])
  std::vector<uint32_t> grp_items;  // B item numbers, stable counting sort by msg_id
  std::vector<SegRun> runs;         // every level's runs, level l at runs[level_off[l] .. level_off[l + 1])
  std::vector<uint32_t> level_off;  // levels + 1
  std::vector<uint32_t> level_tmp;  // partials (non-final runs) each level writes
  size_t levels() const { return level_tmp.size(); }
  uint32_t max_tmp() const {
    uint32_t m = 0;
    for (uint32_t t : level_tmp) m = t > m ? t : m;
    return m;
  }
};

// false (plan untouched beyond scratch use) when M == 0 with B > 0, an id is >= M, or B or M does not fit 31 bits
inline bool seg_plan(const uint32_t* msg_id, size_t B, size_t M, SegPlan& p) {
  if ((B && !M) || B >= SEG_FINAL || M >= SEG_FINAL) return false;
  p.grp_offs.assign(M + 1, 0);
  for (size_t i = 0; i < B; ++i) {
    if (msg_id[i] >= M) return false;
    ++p.grp_offs[msg_id[i] + 1];
  }
  for (size_t m = 0; m < M; ++m) p.grp_offs[m + 1] += p.grp_offs[m];
  p.grp_items.resize(B);
  {
    std::vector<uint32_t> at(p.grp_offs.begin(), p.grp_offs.end() - 1);
    for (size_t i = 0; i < B; ++i) p.grp_items[at[msg_id[i]]++] = (uint32_t)i;
  }
  p.runs.clear();
  p.level_off.assign(1, 0);
  p.level_tmp.clear();
  struct Pend {
    uint32_t grp, src, cnt;
  };
  std::vector<Pend> cur, next;
  cur.reserve(M);
  for (size_t m = 0; m < M; ++m) cur.push_back(Pend{(uint32_t)m, p.grp_offs[m], p.grp_offs[m + 1] - p.grp_offs[m]});
  while (!cur.empty()) {
    uint32_t ntmp = 0;
    next.clear();
    for (const Pend& g : cur) {
      if (g.cnt <= SEG_K) {
        p.runs.push_back(SegRun{g.src, g.cnt, g.grp | SEG_FINAL});
        continue;
      }
      const uint32_t first = ntmp;
      for (uint32_t o = 0; o < g.cnt; o += SEG_K)
        p.runs.push_back(SegRun{g.src + o, g.cnt - o < SEG_K ? g.cnt - o : SEG_K, ntmp++});
      next.push_back(Pend{g.grp, first, ntmp - first});
    }
    p.level_off.push_back((uint32_t)p.runs.size());
    p.level_tmp.push_back(ntmp);
    cur.swap(next);
  }
  return true;
}

}  // namespace bls

#ifndef BLS_SEGSUM_PLAN_ONLY
#include "bls_curve.h"
#include "bls_fq_g1.h"

namespace bls {

// The fold of one run, in the redundant digit form with the complete formulas of bls_fq_g1.h, everything in
// registers.  Bounds: the accumulator starts at the identity (0 : 1 : 0) in N form and is from then on an output
// of g1q_add_aff (N form, < 2p) or of g1q_add_mem below (L form: digits <= 2^29 + 2^4; X < 66p, Y, Z < 4p), both
// inside the accumulator contract of bls_fq_g1.h.
//   level 0: the operand is an affine r_i apk_i, canonical (< p, N form) -- exactly k_fav_gather_q's inner loop,
//     whose largest product is (x2 + y2)(X + Y) < 2p x 70p;
//   above: the operand q is a partial stored canonical (fq_pack) and unpacked, X, Y, Z < p in N form, so
//     g1q_add(acc, q) stays inside what k_fav_gather_q's LDS tree does with two L-form accumulators
//     ((p.x + p.y)(q.x + q.y) < 70p x 70p there, < 70p x 2p here; R / p ~ 2^25.3), operand digits <= 2^30 + 2^5
//     on the accumulator's side and <= 2^30 on q's; the subtrahends of fq_sub / fq_sub2 are N-form products or
//     sums of two, as in the gather.
// The host check runs both with the 128-bit column, value and subtraction checks (tests/test_shared_msgs_cpu.py).
BLS_HD G1Q g1q_identity() { return G1Q{fq_zero(), fq_unpack(FP_ONE), fq_zero()}; }

// level 0: status-0 items (rejected before the pairing: their rP is the identity) are skipped
BLS_HD G1Q seg_fold_items(const SegRun& r, const uint32_t* items, const int* status, const G1A* rP) {
  G1Q acc = g1q_identity();
#pragma unroll 1
  for (uint32_t k = 0; k < r.cnt; ++k) {
    const uint32_t i = items[r.src + k];
    if (status[i]) {
      const G1A& a = rP[i];
      acc = g1q_add_aff(acc, fq_unpack(a.x), fq_unpack(a.y));
    }
  }
  return acc;
}

// p + *q with q in memory: the complete addition (RCB alg. 7) in its own statement, one Montgomery reduction per
// product and the two products of a coordinate combined after both are reduced (g1q_add of bls_fq_g1.h forms each
// coordinate with one reduction; the residues are the same), ordered so that each of its three cross terms reads
// the two coordinates of q it needs again instead of holding all of q (42 registers) across the formula -- with
// both operands in registers the kernel needs more than half a SIMD's register file.  On the device the pointer
// passes through an empty asm between the terms, so the reads are issued again (L2 hits).
BLS_HD const G1P* seg_reread(const G1P* q) {
#ifdef __HIP_DEVICE_COMPILE__
  asm volatile("" : "+v"(q));
#endif
  return q;
}
BLS_HD G1Q g1q_add_mem(const G1Q& p, const G1P* q) {
  Fq t0, t1, t2, t3, t4, y3;
  {
    const Fq qx = fq_unpack(q->x), qy = fq_unpack(q->y);
    t0 = fq_mul(p.x, qx);
    t1 = fq_mul(p.y, qy);
    t3 = fq_norm(fq_sub2(fq_mul(fq_add(p.x, p.y), fq_add(qx, qy)), fq_add(t0, t1)));
  }
  q = seg_reread(q);
  {
    const Fq qy = fq_unpack(q->y), qz = fq_unpack(q->z);
    t2 = fq_mul(p.z, qz);
    t4 = fq_norm(fq_sub2(fq_mul(fq_add(p.y, p.z), fq_add(qy, qz)), fq_add(t1, t2)));
  }
  q = seg_reread(q);
  {
    const Fq qx = fq_unpack(q->x), qz = fq_unpack(q->z);
    y3 = fq_mul_small(fq_sub2(fq_mul(fq_add(p.x, p.z), fq_add(qx, qz)), fq_add(t0, t2)), 12);
  }
  const Fq t0p = fq_add(fq_add(t0, t0), t0);
  const Fq t2p = fq_mul_small(t2, 12);
  const Fq z3 = fq_norm(fq_add(t1, t2p));
  const Fq t1p = fq_sub(t1, t2p);
  G1Q r;
  r.x = fq_norm(fq_sub(fq_mul(t3, t1p), fq_mul(t4, y3)));
  r.y = fq_norm(fq_add(fq_mul(t1p, z3), fq_mul(y3, t0p)));
  r.z = fq_norm(fq_add(fq_mul(z3, t4), fq_mul(t0p, t3)));
  return r;
}

BLS_HD G1Q seg_fold_partials(const SegRun& r, const G1P* prev) {
  G1Q acc = g1q_identity();
#pragma unroll 1
  for (uint32_t k = 0; k < r.cnt; ++k) acc = g1q_add_mem(acc, prev + r.src + k);
  return acc;
}

// canonical projective result: a group's sum with ok = (Z != 0) -- an empty, all-rejected or cancelling group is
// the identity, ok 0, a dead Miller pair -- or a partial for the next level
BLS_HD void seg_store(const SegRun& r, const G1Q& acc, G1P* tmp, G1P* gsum, int* ok) {
  const G1P o{fq_pack(acc.x), fq_pack(acc.y), fq_pack(acc.z)};
  if (r.dst & SEG_FINAL) {
    const uint32_t g = r.dst & ~SEG_FINAL;
    gsum[g] = o;
    ok[g] = fp_is_zero(o.z) ? 0 : 1;
  } else {
    tmp[r.dst] = o;
  }
}

}  // namespace bls
#endif
