// S = sum_i r_i sigma_i for the RLC batch check (Pippenger, 8-bit windows).
//
// The 64-bit scalars split into 8 windows; the (item, window) pairs with a
// nonzero digit d are counting-sorted into 8 x 255 buckets (atomic histogram,
// one block-wide prefix scan, atomic scatter).  Eight launches:
//   k_msm_count, k_msm_scan, k_msm_scatter   the sort; the scan also cuts each
//                   bucket into runs of at most K = 16 entries (G2M_KMAX) and
//                   leaves the runs' offsets
//   k_msm_fold0     one lane per run, in the digit form (bls_g2_msm.h): the
//                   accumulator starts as the run's first point, the rest are
//                   complete mixed additions (g2q_add_aff) with the next
//                   point's load in flight; a bucket's entries are cut evenly
//                   (39 -> 13 + 13 + 13; ~96 waves for a C2 batch).  A bucket
//                   of one run is written straight to the bucket sums
//   k_msm_fold1     one lane per bucket: the run partials of a bucket with
//                   more than one run folded into B_{w,d} (g2q_add_mem), the
//                   identity written for a bucket without entries
//                   (Before, the buckets were summed on lane pairs in the
//                   packed form, 8 strided chunks per bucket from the
//                   identity and a 3-level LDS fold: 512 waves, 152 SIMD-ms
//                   per C2 batch against 55 now.  Below MSM_FOLD_MIN =
//                   8,160 items that form stays, k_msm_bucketc with 4, 2 or
//                   1 chunks in place of the two folds: a C3 or C5 batch has
//                   its MSM on stream1's latency chain and gained nothing.)
//   k_msm_usum      U_b = sum_{d : bit k of d} B_{w,d}  (b = 8w + k): one
//                   wave per b, 32 lane pairs adding 4 bucket sums each, then a
//                   5-level LDS tree (a 16-wave wide-arithmetic variant
//                   measured C2 -4 %: profiles/r04o_usum_ab.txt)
//   k_msm_upairs    the 64 pairs (-w_b G1, U_b), U_b affine, w_b the weight
//                   of scalar bit b (2^b below 32, 2^(b - 32) lambda above:
//                   r_i = a + b lambda, bls_g1_endo.h): the Miller loop
//                   of (-G1, S) with S = sum_b w_b U_b is, after the final
//                   exponentiation, the product of e(-w_b G1, U_b) -- so the
//                   U_b join the batch's own pairs (lines + f accumulation)
//                   and the 63-doubling weighted sum S (round 4:
//                   k_msm_weighted_wide, one 16-wave workgroup, ~0.7 ms) and
//                   its one-pair Miller loop (k_miller_wide, ~0.5 ms) leave
//                   the latency chain.  The -w_b G1 are entries of the
//                   bisection's fixed-base comb (bls_bisect.hip).
// ~8 additions per signature instead of a 64-step double-and-add.  (The
// previous form ran one lane pair per bucket -- 64 waves, ~40 dependent
// additions with unprefetched loads -- and 13 tree launches: ~6.8 ms per C2
// batch.)
#include "bls_kernels.h"
#include "bls_fp_inv.h"
#include "bls_pp_lane.h"
#include "bls_g2_msm.h"

namespace bls {

constexpr int MSM_W = 8, MSM_NB = MSM_W * 256;

// cnt[MSM_NB] must be zero on entry.
__global__ void __launch_bounds__(256) k_msm_count(size_t B, const int* status, const int* status2, const uint64_t* rsc,
                                                   uint32_t* cnt) {
  const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= B * MSM_W) return;
  const size_t i = k / MSM_W;
  const int w = (int)(k % MSM_W);
  if (!status[i] || !status2[i]) return;
  const uint32_t d = (uint32_t)(rsc[i] >> (8 * w)) & 0xffu;
  if (d) atomicAdd(&cnt[w * 256 + d], 1u);
}

// off[b] = exclusive prefix of cnt; cur[b] = off[b] (scatter cursor); roff[b] = exclusive prefix of the buckets' run
// counts ceil(cnt[b] / K); one 256-thread block, 8 buckets per thread
__global__ void __launch_bounds__(256) k_msm_scan(const uint32_t* cnt, uint32_t K, uint32_t* off, uint32_t* cur,
                                                  uint32_t* roff) {
  constexpr int PER = MSM_NB / 256;
  __shared__ uint32_t part[256], rpart[256];
  const int t = threadIdx.x;
  uint32_t loc[PER], sum = 0, rsum = 0;
#pragma unroll
  for (int i = 0; i < PER; i++) {
    loc[i] = cnt[t * PER + i];
    sum += loc[i];
    rsum += g2m_nruns(loc[i], K);
  }
  part[t] = sum;
  rpart[t] = rsum;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {  // inclusive Hillis-Steele scan of the per-thread sums
    const uint32_t v = t >= d ? part[t - d] : 0u;
    const uint32_t rv = t >= d ? rpart[t - d] : 0u;
    __syncthreads();
    part[t] += v;
    rpart[t] += rv;
    __syncthreads();
  }
  uint32_t base = part[t] - sum, rbase = rpart[t] - rsum;
#pragma unroll
  for (int i = 0; i < PER; i++) {
    off[t * PER + i] = base;
    cur[t * PER + i] = base;
    roff[t * PER + i] = rbase;
    base += loc[i];
    rbase += g2m_nruns(loc[i], K);
  }
  if (t == 255) {
    off[MSM_NB] = part[255];
    roff[MSM_NB] = rpart[255];
  }
}

__global__ void __launch_bounds__(256) k_msm_scatter(size_t B, const int* status, const int* status2,
                                                     const uint64_t* rsc, uint32_t* cur, uint32_t* lst) {
  const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= B * MSM_W) return;
  const size_t i = k / MSM_W;
  const int w = (int)(k % MSM_W);
  if (!status[i] || !status2[i]) return;
  const uint32_t d = (uint32_t)(rsc[i] >> (8 * w)) & 0xffu;
  if (d) lst[atomicAdd(&cur[w * 256 + d], 1u)] = (uint32_t)i;
}

using P2 = PP<Fp2>;

// ------------------------------------------------------ bucket sums (digit form) --
// Level 0: lane r < roff[MSM_NB] folds run r (bls_g2_msm.h).  Its bucket b is the one with roff[b] <= r < roff[b + 1]
// (bisection; an empty bucket shares its offset with its successor and is never found); the bucket's entries are cut
// evenly over its roff[b + 1] - roff[b] runs.  A bucket of one run has its sum written straight to csum; else the
// run's partial goes to part[r], so a bucket's partials lie together at part[roff[b] ..).  One lane per run, one
// wave per SIMD, no cross-lane operation, no LDS, no private segment.
__global__ void __launch_bounds__(64) k_msm_fold0(const uint32_t* off, const uint32_t* roff, const uint32_t* lst,
                                                  const G2A* sig, G2SP* part, Fp* csum) {
  const uint32_t r = blockIdx.x * 64 + threadIdx.x;
  if (r >= roff[MSM_NB]) return;
  uint32_t lo = 0, hi = MSM_NB;  // roff[lo] <= r < roff[hi]
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (roff[mid] <= r) lo = mid;
    else hi = mid;
  }
  const uint32_t first = off[lo], runs = roff[lo + 1] - roff[lo];
  const G2mRun g = g2m_run(off[lo + 1] - first, runs, r - roff[lo]);
  const G2Q acc = g2m_fold_records(sig, lst + first + g.src, g.cnt);
  g2m_store_run(part + r, csum + (size_t)lo * 6, runs == 1, acc);
}

// Level 1: lane b < MSM_NB finishes bucket b: the identity for a bucket without entries, nothing for a bucket of one
// run (level 0 wrote its sum), else the fold of its run partials.
__global__ void __launch_bounds__(64) k_msm_fold1(const uint32_t* roff, const G2SP* part, Fp* csum) {
  const uint32_t b = blockIdx.x * 64 + threadIdx.x;
  static_assert(MSM_NB % 64 == 0, "k_msm_fold1: whole waves");
  const uint32_t r0 = roff[b], runs = roff[b + 1] - r0;
  if (runs == 1) return;
  Fp* o = csum + (size_t)b * 6;
  if (!runs) {
    g2m_store_identity(o);
    return;
  }
  g2m_store_sum(o, g2m_fold_partials(part + r0, runs));
}

// ----------------------------------------------------------- lane form --
// U and weighted sums on lane pairs (bls_pp_lane.h pp2_*: complete
// projective formulas, each dependency level split between lanes 2k / 2k+1).
namespace {
// a point through LDS or HBM as six packed Fp: lane 0 of a pair writes x, y.c0, lane 1 y.c1, z
__device__ __forceinline__ void p2_store(Fp* o, const P2& p, bool hi) {  // selects, not a branch: no stack copy
  Fp* d = o + (hi ? 3 : 0);
  d[0] = fp_select(hi, p.y.c1, p.x.c0);
  d[1] = fp_select(hi, p.z.c0, p.x.c1);
  d[2] = fp_select(hi, p.z.c1, p.y.c0);
}
__device__ __forceinline__ P2 p2_load(const Fp* in) {
  return P2{Fp2{in[0], in[1]}, Fp2{in[2], in[3]}, Fp2{in[4], in[5]}};
}
}  // namespace

// Bucket sums of a batch below MSM_FOLD_MIN items, on lane pairs in the packed form.  There the MSM sits on
// stream1's latency chain, and the run folds measured no gain (C3 the same, C5 -1 %: profiles/g2msm_ab.txt).
// Measured were 1,024 and 2,048 items on this side and 10,000 and 125,000 on the other; nothing in between.  The
// boundary is where the lane-pair form went to eight chunks, not a measured crossover.  (k_msm_scan's run offsets
// are written here too and not read.)
// chunks per bucket for such a batch of B items: ~B / 255 points per bucket; few enough that a C3- or C5-size batch
// is not mostly fold tree and idle lanes
constexpr size_t MSM_FOLD_MIN = 32 * 255;
static int msm_chunks(size_t B) {
  const size_t per = B / 255;
  return per >= 12 ? 4 : per >= 4 ? 2 : 1;
}

// chunk c of bucket b (lane pair (b, c)): the sum of the bucket's points k = off[b] + c + j C from the identity, the
// chunks then folded by a log2(C)-level LDS tree into csum[b]
template <int MSM_C>
__global__ void __launch_bounds__(64) k_msm_bucketc(const uint32_t* off, const uint32_t* lst, const G2A* sig,
                                                    Fp* csum) {
  const int t = blockIdx.x * 64 + threadIdx.x;
  const int pi = t >> 1;
  const bool hi = (t & 1) != 0;
  // every lane reaches the fold's barriers: the grid covers the MSM_NB * MSM_C lane pairs exactly
  static_assert((2 * MSM_NB * MSM_C) % 64 == 0 && MSM_C <= 32, "k_msm_bucketc: whole waves, chunks within a wave");
  const int b = pi / MSM_C, c = pi % MSM_C;
  P2 R{fp2_zero(), fp2_one(), fp2_zero()};
  const uint32_t end = off[b + 1];
  uint32_t k = off[b] + c;
  // the next point is in flight while this one is added (both lanes of a pair run the same trip count)
  G2A q = sig[k < end ? lst[k] : 0u];
  uint32_t li = k + MSM_C < end ? lst[k + MSM_C] : 0u;
#pragma unroll 1
  for (; k < end; k += MSM_C) {
    const G2A cq = q;
    q = sig[li];
    li = k + 2 * MSM_C < end ? lst[k + 2 * MSM_C] : 0u;
    R = pp2_add_aff(R, cq.x, cq.y, hi);
  }
  __shared__ Fp sm[32 * 6];
  const int lp = threadIdx.x >> 1;  // lane pair in the wave
#pragma unroll 1
  for (int s = MSM_C / 2; s >= 1; s >>= 1) {
    if (c >= s && c < 2 * s) p2_store(sm + 6 * (lp - s), R, hi);
    __syncthreads();
    if (c < s) R = pp2_add(R, p2_load(sm + 6 * lp), hi);
    __syncthreads();
  }
  if (c == 0) p2_store(csum + (size_t)b * 6, R, hi);
}

// U_b for b = blockIdx.x (w = b / 8, bit k = b % 8): one wave of 32 lane pairs; pair j adds the bucket sums of
// the digits d_j, d_{j+32}, d_{j+64}, d_{j+96} (d_i = the i-th digit with bit k set), then a 5-level LDS tree.
// (128 pairs over four waves with a 7-level tree ran one addition shorter but held 4x the waves at barriers:
// 16 % -> 9 % of a C3 epoch's wave time after the bucket fold, profiles/r04n2_c3_timeline.txt.)
constexpr int USUM_PAIRS = 32;
__global__ void __launch_bounds__(64) k_msm_usum(const Fp* csum, Fp* U) {
  __shared__ Fp sm[(USUM_PAIRS / 2) * 6];
  const int b = blockIdx.x, w = b >> 3, kb = b & 7;
  const int j = threadIdx.x >> 1;
  const bool hi = (threadIdx.x & 1) != 0;
  auto bucket = [&](int i) {
    const int d = ((i >> kb) << (kb + 1)) | (1 << kb) | (i & ((1 << kb) - 1));
    return csum + (size_t)(w * 256 + d) * 6;
  };
  P2 R = p2_load(bucket(j));
#pragma unroll 1
  for (int t = 1; t < 128 / USUM_PAIRS; ++t) R = pp2_add(R, p2_load(bucket(j + USUM_PAIRS * t)), hi);
#pragma unroll 1
  for (int s = USUM_PAIRS / 2; s >= 1; s >>= 1) {
    if (j >= s && j < 2 * s) p2_store(sm + 6 * (j - s), R, hi);
    __syncthreads();
    if (j < s) R = pp2_add(R, p2_load(sm + 6 * j), hi);
    __syncthreads();
  }
  if (j == 0) p2_store(U + 6 * b, R, hi);
}

// lane b < 64: pair (-w_b G1, U_b) at P[b], Q[b], ok[b] = 1 (U_b = the identity: Q[b].inf, a skipped pair), w_b
// the weight of scalar bit b: 2^b for b < 32, 2^(b - 32) lambda above (r_i = a + b lambda, bls_g1_endo.h).
// -w_b G1 = comb[256 (b / 8) + 2^(b % 8)] (comb[256 w + d] = d 2^(8 w) (-G1), its phi image for w >= 4).
__global__ void __launch_bounds__(64) k_msm_upairs(const Fp* U, const G1A* comb, G1A* P, G2A* Q, int* ok) {
  const int b = threadIdx.x;
  const Fp* u = U + 6 * b;
  const Fp2 X{u[0], u[1]}, Y{u[2], u[3]}, Z{u[4], u[5]};
  G2A q{fp2_zero(), fp2_zero(), true};
  if (!fp2_is_zero(Z)) {  // homogeneous projective (RCB): x = X / Z, y = Y / Z
    const Fp ni = fp_inv_sg_i(fp_add(fp_sqr_i(Z.c0), fp_sqr_i(Z.c1)));  // 1 / norm(Z)
    const Fp2 zi{fp_mul_i(Z.c0, ni), fp_neg(fp_mul_i(Z.c1, ni))};
    q = G2A{f2mul(X, zi), f2mul(Y, zi), false};
  }
  Q[b] = q;
  P[b] = comb[256 * (b >> 3) + (1 << (b & 7))];
  ok[b] = 1;
}

// Scratch: cnt[MSM_NB] | off[MSM_NB + 1] | cur[MSM_NB] | roff[MSM_NB + 1] (u32), lst[8 B] (u32);
// points (in units of Fd slots): bucket sums [MSM_NB] | U [64] (packed Fp, 6 per point) | run partials (G2SP), one per
// run: at most 8 B / K full runs and one partly filled run per bucket.
namespace {
size_t msm_max_runs(size_t B, uint32_t K) { return MSM_W * B / K + MSM_NB; }
// entries per run: G2M_KMAX for a batch of MSM_FOLD_MIN items or more, 0 (the lane-pair kernel) below; run_len != 0
// (the test hook) asks for the run folds at that length whatever the size
uint32_t msm_run_len(size_t B, uint32_t run_len) {
  if (run_len) return run_len < G2M_KMAX ? run_len : G2M_KMAX;
  return B >= MSM_FOLD_MIN ? G2M_KMAX : 0;
}
}  // namespace
size_t msm_scratch_u32(size_t B) { return (size_t)4 * MSM_NB + 2 + MSM_W * B; }
size_t msm_scratch_fd(size_t B, uint32_t run_len) {
  const uint32_t K = msm_run_len(B, run_len);
  const size_t bytes = (size_t)(MSM_NB + 64) * 6 * sizeof(Fp) + (K ? msm_max_runs(B, K) : 0) * sizeof(G2SP);
  return (bytes + sizeof(Fd) - 1) / sizeof(Fd);
}

hipError_t launch_msm_upairs(hipStream_t st, size_t B, const int* status, const int* status2, const uint64_t* rsc,
                             const G2A* sig, uint32_t* scr, Fd* pts, const G1A* comb, G1A* P, G2A* Q, int* ok,
                             uint32_t run_len) {
  const uint32_t K = msm_run_len(B, run_len);
  uint32_t* cnt = scr;
  uint32_t* off = cnt + MSM_NB;
  uint32_t* cur = off + MSM_NB + 1;
  uint32_t* roff = cur + MSM_NB;
  uint32_t* lst = roff + MSM_NB + 1;
  Fp* csum = reinterpret_cast<Fp*>(pts);
  Fp* U = csum + (size_t)MSM_NB * 6;
  G2SP* part = reinterpret_cast<G2SP*>(U + 64 * 6);
  static_assert(alignof(G2SP) <= alignof(Fp), "the run partials follow the packed points");
  hipError_t e = hipMemsetAsync(cnt, 0, MSM_NB * sizeof(uint32_t), st);
  if (e != hipSuccess) return e;
  const unsigned nb = (unsigned)((B * MSM_W + 255) / 256);
  if (B) {
    hipLaunchKernelGGL(k_msm_count, dim3(nb), dim3(256), 0, st, B, status, status2, rsc, cnt);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_msm_scan, dim3(1), dim3(256), 0, st, cnt, K ? K : G2M_KMAX, off, cur, roff);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (B) {
    hipLaunchKernelGGL(k_msm_scatter, dim3(nb), dim3(256), 0, st, B, status, status2, rsc, cur, lst);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (K) {
    // the grid covers the most runs the batch can have; the lanes past roff[MSM_NB] leave at once
    hipLaunchKernelGGL(k_msm_fold0, dim3((unsigned)((msm_max_runs(B, K) + 63) / 64)), dim3(64), 0, st, off, roff, lst,
                       sig, part, csum);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_msm_fold1, dim3(MSM_NB / 64), dim3(64), 0, st, roff, part, csum);
  } else {
    switch (msm_chunks(B)) {
      case 4: hipLaunchKernelGGL(k_msm_bucketc<4>, dim3(2 * MSM_NB * 4 / 64), dim3(64), 0, st, off, lst, sig, csum); break;
      case 2: hipLaunchKernelGGL(k_msm_bucketc<2>, dim3(2 * MSM_NB * 2 / 64), dim3(64), 0, st, off, lst, sig, csum); break;
      default: hipLaunchKernelGGL(k_msm_bucketc<1>, dim3(2 * MSM_NB / 64), dim3(64), 0, st, off, lst, sig, csum);
    }
  }
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(k_msm_usum, dim3(64), dim3(2 * USUM_PAIRS), 0, st, csum, U);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(k_msm_upairs, dim3(1), dim3(64), 0, st, U, comb, P, Q, ok);
  return hipGetLastError();
}

}  // namespace bls
