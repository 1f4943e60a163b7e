// Kernels of the resident G1 table and its batched bucket MSM (bls_capi_msm.hip; per-lane pieces in bls_g1_msm.h).
//
// Load (launch_g1_table_fill): the decoded points become window-0 records and projective running points; then per
// window w = 1 .. 31: k_g1t_step (eight doublings in digits), launch_g1_affine (one inversion per 8 entries),
// k_g1t_pack (records w * cap + first + i).
//
// MSM (launch_g1_table_msm), out[v] = sum_i [k_{v,i}] T[idx[i]] for v < B, additions only:
//   k_g1m_sort (count) / scan / k_g1m_sort (scatter)   one lane per (v, i) splits the scalar into 32 digits; the non-zero digits
//                   of non-identity entries are counting-sorted into the 256 B bucket slots (v, d) as record numbers
//                   w * cap + idx[i]
//   k_g1m_nruns / scan / k_g1m_fold      one level of the bucket sums: a bucket's items (level 0: list entries, above:
//                   the partials of the level below) are cut into runs of at most G1M_K; one lane folds one run and
//                   finds its bucket by bisecting the run offsets, which a device scan made -- no host plan.  The host
//                   launches ceil(log_K(32 n)) levels over grids sized by the worst case; after the last, every
//                   bucket has at most one partial.  One bucket holding every entry is as parallel as 255 even ones.
//   k_g1m_usum      U_{v,b} = sum of the buckets of v whose digit has bit b: one wave per (v, b), two buckets per
//                   lane, then a 6-level LDS tree (k_msm_usum's scheme)
//   k_g1m_final     sum_b 2^b U_{v,b} by Horner, one lane per vector; launch_g1_affine; k_g1m_compress
// The scan is three kernels over blocks of 1,024 counters, so 256 B slots need no single-block limit.
//
// Variable base (launch_g1_var_msm), out[v] = sum_i [k_{v,i}] P_i over the call's own points, no window multiples:
//   k_g1vm_records  the n points as single-window records
//   k_g1vm_sort (count) / scan / k_g1vm_sort (scatter)   buckets per (row, window, digit): 8,192 B slots
//   the levels, k_g1m_usum and k_g1m_final above over the 32 B slot groups: one window sum W_{v,w} per (row, window)
//   k_g1vm_combine  sum_w 2^(8w) W_{v,w} by Horner from the row's top window, one lane per row; launch_g1_affine;
//                   k_g1m_compress
#include "bls_kernels.h"
#include "bls_g1_var_msm.h"
#include "bls_key_out.h"

namespace bls {

namespace {
inline unsigned nblk(size_t n, unsigned t) { return (unsigned)((n + t - 1) / t); }
constexpr uint32_t SCAN_BLK = 1024;  // counters per scan block: 256 threads x 4
}  // namespace

// ------------------------------------------------------------------------------------------------------- load --
__global__ void __launch_bounds__(256) k_g1t_first(const G1A* a, const int* ok, size_t n, RegKey* rec, uint8_t* stat,
                                                   G1P* cur, int* live, uint8_t* out_ok) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const G1A p = a[i];
  const bool v = ok[i] != 0, pt = v && !p.inf;
  // selects and field-wise stores: no G1P or RegKey temporary (bls_key_out.h has the cost of one)
  G1P* c = cur + i;
  c->x = fp_select(pt, p.x, fp_zero());
  c->y = fp_select(pt, p.y, FP_ONE);  // the identity (0 : 1 : 0) for an unusable entry
  c->z = fp_select(pt, FP_ONE, fp_zero());
  KeyOutRecords{rec, nullptr}.put(i, p, pt ? 1 : 0);
  stat[i] = !v ? G1T_INVALID : p.inf ? G1T_IDENTITY : G1T_POINT;
  live[i] = pt ? 1 : 0;
  out_ok[i] = v ? 1 : 0;
}

__global__ void __launch_bounds__(64) k_g1t_step(size_t n, const int* live, G1P* cur) {
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n || !live[i]) return;
  cur[i] = g1m_window_step(cur[i]);
}

__global__ void __launch_bounds__(256) k_g1t_pack(const G1A* a, const int* live, size_t n, RegKey* rec) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const bool pt = live[i] != 0;
  KeyOutRecords{rec, nullptr}.put(i, a[i], pt ? 1 : 0);
}

hipError_t launch_g1_table_fill(hipStream_t st, const G1A* a, const int* ok, size_t n, RegKey* tab, size_t cap,
                                size_t first, uint8_t* stat, G1P* cur, int* live, G1A* aff, uint8_t* out_ok) {
  if (!n) return hipSuccess;
  hipError_t e;
  hipLaunchKernelGGL(k_g1t_first, dim3(nblk(n, 256)), dim3(256), 0, st, a, ok, n, tab + first, stat + first, cur, live,
                     out_ok);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  for (int w = 1; w < G1M_WINDOWS; ++w) {
    hipLaunchKernelGGL(k_g1t_step, dim3(nblk(n, 64)), dim3(64), 0, st, n, live, cur);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = launch_g1_affine(st, n, live, cur, aff)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_g1t_pack, dim3(nblk(n, 256)), dim3(256), 0, st, aff, live, n, tab + (size_t)w * cap + first);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}

// -------------------------------------------------------------------------------------------------------- sort --
// One lane per (vector, item).  SCATTER = false: cnt[v * 256 + d] += 1 per non-zero digit (cnt zero on entry);
// true: the record numbers go to the buckets' lists through the cursors cur (= the buckets' offsets on entry).
template <bool SCATTER>
__global__ void __launch_bounds__(256) k_g1m_sort(const uint32_t* idx, const uint8_t* stat, uint32_t n, uint32_t B,
                                                  const uint8_t* k32, uint32_t cap, uint32_t* cnt_or_cur,
                                                  uint32_t* lst) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (size_t)n * B) return;
  const uint32_t v = (uint32_t)(t / n), i = (uint32_t)(t % n);
  const uint32_t e = idx[i];
  if (stat[e] != G1T_POINT) return;  // the identity contributes nothing (an invalid entry was refused by the call)
  uint32_t k[8];
  {
    const uint4* p = reinterpret_cast<const uint4*>(k32 + 32 * t);
    const uint4 lo = p[0], hi = p[1];
    k[0] = lo.x, k[1] = lo.y, k[2] = lo.z, k[3] = lo.w, k[4] = hi.x, k[5] = hi.y, k[6] = hi.z, k[7] = hi.w;
  }
  uint32_t* slot = cnt_or_cur + (size_t)v * G1M_SLOTS;
#pragma unroll 1
  for (int w = 0; w < G1M_WINDOWS; ++w) {
    const uint32_t d = g1m_digit(k, w);
    if (!d) continue;
    if (SCATTER) lst[atomicAdd(&slot[d], 1u)] = (uint32_t)w * cap + e;
    else atomicAdd(&slot[d], 1u);
  }
}

// -------------------------------------------------------------------------------------------------------- scan --
// off[0 .. N] = the exclusive prefix sums of cnt[0 .. N) in three kernels: per block of SCAN_BLK counters the local
// prefix and the block's total, the totals' prefix on one block, and the sum of both (cur, nullable: a copy, the
// scatter's cursors).
__global__ void __launch_bounds__(256) k_g1m_scan_blk(const uint32_t* cnt, uint32_t N, uint32_t* off, uint32_t* bsum) {
  __shared__ uint32_t part[256];
  const uint32_t t = threadIdx.x, base = blockIdx.x * SCAN_BLK + 4 * t;
  uint32_t loc[4], sum = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    loc[i] = base + i < N ? cnt[base + i] : 0u;
    sum += loc[i];
  }
  part[t] = sum;
  __syncthreads();
  for (uint32_t d = 1; d < 256; d <<= 1) {  // inclusive Hillis-Steele scan of the per-thread sums
    const uint32_t v = t >= d ? part[t - d] : 0u;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  uint32_t run = part[t] - sum;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    if (base + i < N) off[base + i] = run;
    run += loc[i];
  }
  if (t == 255) bsum[blockIdx.x] = part[255];
}

// bsum[0 .. nb) -> its exclusive prefix, bsum[nb] = the total; one block, 256 totals per round
__global__ void __launch_bounds__(256) k_g1m_scan_top(uint32_t* bsum, uint32_t nb) {
  __shared__ uint32_t part[256];
  const uint32_t t = threadIdx.x;
  uint32_t carry = 0;
  for (uint32_t r = 0; r < nb; r += 256) {
    const uint32_t mine = r + t < nb ? bsum[r + t] : 0u;
    part[t] = mine;
    __syncthreads();
    for (uint32_t d = 1; d < 256; d <<= 1) {
      const uint32_t v = t >= d ? part[t - d] : 0u;
      __syncthreads();
      part[t] += v;
      __syncthreads();
    }
    if (r + t < nb) bsum[r + t] = carry + part[t] - mine;
    carry += part[255];
    __syncthreads();
  }
  if (t == 0) bsum[nb] = carry;
}

__global__ void __launch_bounds__(256) k_g1m_scan_add(uint32_t* off, uint32_t N, const uint32_t* bsum, uint32_t nb,
                                                      uint32_t* cur) {
  const uint32_t e = blockIdx.x * 256 + threadIdx.x;
  if (e < N) {
    const uint32_t o = off[e] + bsum[e / SCAN_BLK];
    off[e] = o;
    if (cur) cur[e] = o;
  }
  if (e == 0) off[N] = bsum[nb];
}

static hipError_t g1m_scan(hipStream_t st, const uint32_t* cnt, uint32_t N, uint32_t* off, uint32_t* bsum,
                           uint32_t* cur) {
  const uint32_t nb = nblk(N, SCAN_BLK);
  hipError_t e;
  hipLaunchKernelGGL(k_g1m_scan_blk, dim3(nb), dim3(256), 0, st, cnt, N, off, bsum);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(k_g1m_scan_top, dim3(1), dim3(256), 0, st, bsum, nb);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(k_g1m_scan_add, dim3(nblk(N, 256)), dim3(256), 0, st, off, N, bsum, nb, cur);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------- bucket sums --
// runs of the next level: cnt[b] = ceil(items of b / G1M_K), items = off[b + 1] - off[b]
__global__ void __launch_bounds__(256) k_g1m_nruns(const uint32_t* off, uint32_t N, uint32_t* cnt) {
  const uint32_t b = blockIdx.x * 256 + threadIdx.x;
  if (b < N) cnt[b] = (off[b + 1] - off[b] + G1M_K - 1) / G1M_K;
}

// One level: lane r < roff[N] folds run r.  Its bucket b is the one with roff[b] <= r < roff[b + 1] (bisection;
// empty buckets share an offset with their successor and are never found); the run is items
// ioff[b] + G1M_K j .. of the bucket, j = r - roff[b].  L0: the items are record numbers in lst; else partials in
// prev.  The run's sum goes to out[r], canonical projective.
template <bool L0>
__global__ void __launch_bounds__(64) k_g1m_fold(const uint32_t* ioff, const uint32_t* roff, uint32_t N,
                                                 const RegKey* tab, const uint32_t* lst, const G1P* prev, G1P* out) {
  const uint32_t r = blockIdx.x * 64 + threadIdx.x;
  if (r >= roff[N]) return;
  uint32_t lo = 0, hi = N;  // roff[lo] <= r < roff[hi]
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (roff[mid] <= r) lo = mid;
    else hi = mid;
  }
  const uint32_t src = ioff[lo] + (r - roff[lo]) * G1M_K;
  const uint32_t left = ioff[lo + 1] - src;
  const uint32_t cnt = left < G1M_K ? left : G1M_K;
  const G1Q acc = L0 ? g1m_fold_records(tab, lst + src, cnt) : g1m_fold_partials(prev + src, cnt);
  out[r] = g1m_pack(acc);
}

// ---------------------------------------------------------------------------------------------------- reduction --
// U[8 v + b] for blockIdx.x = 8 v + b: lane j adds the sums of two buckets whose digit has bit b (g1m_bit_lane), then a
// 6-level LDS tree of complete additions.
__global__ void __launch_bounds__(64) k_g1m_usum(const uint32_t* off, const G1P* sums, G1P* U) {
  __shared__ G1Q sh[64];
  const uint32_t v = blockIdx.x >> 3;
  const int b = (int)(blockIdx.x & 7);
  const uint32_t j = threadIdx.x;
  const G1Q acc = g1m_bit_lane(off, sums, v, b, j);
  sh[j] = acc;
  __syncthreads();
#pragma unroll 1
  for (uint32_t s = 32; s > 0; s >>= 1) {
    if (j < s) sh[j] = g1q_add(sh[j], sh[j + s]);
    __syncthreads();
  }
  if (j == 0) U[blockIdx.x] = g1m_pack(sh[0]);
}

__global__ void __launch_bounds__(64) k_g1m_final(const G1P* U, uint32_t B, G1P* res, int* live) {
  const uint32_t v = blockIdx.x * 64 + threadIdx.x;
  if (v >= B) return;
  const G1P o = g1m_pack(g1m_horner(U + 8 * (size_t)v));
  res[v] = o;
  live[v] = fp_is_zero(o.z) ? 0 : 1;  // the identity: launch_g1_affine's status-0 item
}

__global__ void __launch_bounds__(64) k_g1m_compress(const G1A* a, uint32_t B, uint8_t* out48) {
  const uint32_t v = blockIdx.x * 64 + threadIdx.x;
  if (v < B) g1_compress(out48 + 48 * (size_t)v, a[v]);
}

// ---------------------------------------------------------------------------------------------------- launcher --
G1MsmPlan g1_msm_plan(size_t n, size_t B) {
  G1MsmPlan p{};
  p.slots = (uint32_t)(B * G1M_SLOTS);
  p.entries = n * B * G1M_WINDOWS;
  size_t deepest = n * G1M_WINDOWS, total = p.entries;  // items of the fullest bucket / of all buckets, at most
  do {
    deepest = (deepest + G1M_K - 1) / G1M_K;
    total = (total + G1M_K - 1) / G1M_K + (size_t)255 * B;  // one partly filled run per non-empty bucket
    size_t& part = p.part[p.levels & 1];
    part = total > part ? total : part;
    p.level_runs[p.levels++] = total;
  } while (deepest > 1);
  if (!p.part[1]) p.part[1] = 1;
  // cnt | cur (slots each) | offA | offL0 | offL1 (slots + 1 each) | bsum (blocks + 1) | lst
  p.u32_words = (size_t)5 * p.slots + 3 + nblk(p.slots, SCAN_BLK) + 1 + p.entries;
  return p;
}

// The levelled bucket sums, the bit sums and Horner over G slot groups of 256 slots each (N = 256 G; a group is a
// vector of the table MSM, a (row, window) of the variable-base one): res[g] = sum_d d S_{g,d}, live[g] = res[g] is
// not the identity.  offA: the lists' offsets, lst: their record numbers into tab.
static hipError_t g1m_reduce(hipStream_t st, const G1MsmPlan& p, uint32_t N, uint32_t G, const RegKey* tab,
                             const uint32_t* lst, uint32_t* cnt, const uint32_t* offA, uint32_t* const offL[2],
                             uint32_t* bsum, G1P* const part[2], G1P* U, G1P* res, int* live) {
  hipError_t e;
  // level l cuts the items at ioff (the lists, then the partials of level l - 1) into the runs at roff
  const uint32_t* ioff = offA;
  const G1P* sums = nullptr;
  for (int l = 0; l < p.levels; ++l) {
    uint32_t* roff = offL[l & 1];
    G1P* out = part[l & 1];
    hipLaunchKernelGGL(k_g1m_nruns, dim3(nblk(N, 256)), dim3(256), 0, st, ioff, N, cnt);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = g1m_scan(st, cnt, N, roff, bsum, nullptr)) != hipSuccess) return e;
    const unsigned fb = nblk(p.level_runs[l], 64);
    if (l == 0)
      hipLaunchKernelGGL(k_g1m_fold<true>, dim3(fb), dim3(64), 0, st, ioff, roff, N, tab, lst, nullptr, out);
    else
      hipLaunchKernelGGL(k_g1m_fold<false>, dim3(fb), dim3(64), 0, st, ioff, roff, N, nullptr, nullptr, sums, out);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    ioff = roff;
    sums = out;
  }
  hipLaunchKernelGGL(k_g1m_usum, dim3(8 * G), dim3(64), 0, st, ioff, sums, U);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(k_g1m_final, dim3(nblk(G, 64)), dim3(64), 0, st, U, G, res, live);
  return hipGetLastError();
}

hipError_t launch_g1_table_msm(hipStream_t st, const G1MsmPlan& p, const RegKey* tab, uint32_t cap,
                               const uint8_t* stat, const uint32_t* idx, uint32_t n, uint32_t B, const uint8_t* k32,
                               uint32_t* scr, G1P* partA, G1P* partB, G1P* U, G1P* res, int* live, G1A* aff,
                               uint8_t* out48, const uint32_t** d_entries) {
  const uint32_t N = p.slots;
  uint32_t* cnt = scr;
  uint32_t* cur = cnt + N;
  uint32_t* offA = cur + N;
  uint32_t* offL[2] = {offA + N + 1, offA + 2 * (size_t)N + 2};
  uint32_t* bsum = offA + 3 * (size_t)N + 3;
  uint32_t* lst = bsum + nblk(N, SCAN_BLK) + 1;
  G1P* part[2] = {partA, partB};
  hipError_t e;
  if ((e = hipMemsetAsync(cnt, 0, (size_t)N * sizeof(uint32_t), st)) != hipSuccess) return e;
  const unsigned sb = nblk((size_t)n * B, 256);
  hipLaunchKernelGGL(k_g1m_sort<false>, dim3(sb), dim3(256), 0, st, idx, stat, n, B, k32, cap, cnt, nullptr);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = g1m_scan(st, cnt, N, offA, bsum, cur)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_g1m_sort<true>, dim3(sb), dim3(256), 0, st, idx, stat, n, B, k32, cap, cur, lst);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  *d_entries = offA + N;  // the entries the buckets hold
  if ((e = g1m_reduce(st, p, N, B, tab, lst, cnt, offA, offL, bsum, part, U, res, live)) != hipSuccess) return e;
  if ((e = launch_g1_affine(st, B, live, res, aff)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_g1m_compress, dim3(nblk(B, 64)), dim3(64), 0, st, aff, B, out48);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------- variable base (bls_g1_msm) --
// The call's own points (per-lane pieces in bls_g1_var_msm.h): record i = point i (REG_VALID and live[i] set on a
// usable non-identity point), one window only.
__global__ void __launch_bounds__(256) k_g1vm_records(const G1A* a, const int* ok, uint32_t n, RegKey* rec,
                                                      int* live) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const G1A p = a[i];
  const bool pt = ok[i] != 0 && !p.inf;
  KeyOutRecords{rec, nullptr}.put(i, p, pt ? 1 : 0);
  live[i] = pt ? 1 : 0;
}

// k_g1m_sort's two passes with buckets per (row, window, digit): one lane per (v, i); the non-zero digit d of window w
// goes to slot (v * 32 + w) * 256 + d as record number i.  Points that are not live are dropped.
template <bool SCATTER>
__global__ void __launch_bounds__(256) k_g1vm_sort(const int* live, uint32_t n, uint32_t B, const uint8_t* k32,
                                                   uint32_t* cnt_or_cur, uint32_t* lst) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (size_t)n * B) return;
  const uint32_t v = (uint32_t)(t / n), i = (uint32_t)(t % n);
  if (!live[i]) return;
  uint32_t k[8];
  {
    const uint4* p = reinterpret_cast<const uint4*>(k32 + 32 * t);
    const uint4 lo = p[0], hi = p[1];
    k[0] = lo.x, k[1] = lo.y, k[2] = lo.z, k[3] = lo.w, k[4] = hi.x, k[5] = hi.y, k[6] = hi.z, k[7] = hi.w;
  }
  g1vm_each_slot(k, v, [&](uint32_t slot) {
    if (SCATTER) lst[atomicAdd(&cnt_or_cur[slot], 1u)] = i;
    else atomicAdd(&cnt_or_cur[slot], 1u);
  });
}

// res[v] = sum_w 2^(8w) W[32 v + w], one lane per row (g1vm_combine); live[v] = 0 for the identity
__global__ void __launch_bounds__(64) k_g1vm_combine(const G1P* W, uint32_t B, G1P* res, int* live) {
  const uint32_t v = blockIdx.x * 64 + threadIdx.x;
  if (v >= B) return;
  const G1P o = g1m_pack(g1vm_combine(W + (size_t)G1M_WINDOWS * v));
  res[v] = o;
  live[v] = fp_is_zero(o.z) ? 0 : 1;
}

G1MsmPlan g1_var_msm_plan(size_t n, size_t B) {
  G1MsmPlan p{};
  const size_t groups = B * G1M_WINDOWS;
  p.slots = (uint32_t)(groups * G1M_SLOTS);
  p.entries = n * groups;
  size_t deepest = n, total = p.entries;  // a bucket holds at most every point once
  do {
    deepest = (deepest + G1M_K - 1) / G1M_K;
    // one partly filled run per non-empty bucket, and never more runs than items
    const size_t runs = (total + G1M_K - 1) / G1M_K + (size_t)255 * groups;
    total = runs < total ? runs : total;
    size_t& part = p.part[p.levels & 1];
    part = total > part ? total : part;
    p.level_runs[p.levels++] = total;
  } while (deepest > 1);
  if (!p.part[1]) p.part[1] = 1;
  p.u32_words = (size_t)5 * p.slots + 3 + nblk(p.slots, SCAN_BLK) + 1 + p.entries;
  return p;
}

hipError_t launch_g1_var_msm(hipStream_t st, const G1MsmPlan& p, const G1A* pts, const int* ok, uint32_t n,
                             uint32_t B, const uint8_t* k32, RegKey* rec, int* plive, uint32_t* scr, G1P* partA,
                             G1P* partB, G1P* U, G1P* W, int* wlive, G1P* res, int* live, G1A* aff, uint8_t* out48,
                             const uint32_t** d_entries) {
  const uint32_t N = p.slots, G = B * G1M_WINDOWS;
  uint32_t* cnt = scr;
  uint32_t* cur = cnt + N;
  uint32_t* offA = cur + N;
  uint32_t* offL[2] = {offA + N + 1, offA + 2 * (size_t)N + 2};
  uint32_t* bsum = offA + 3 * (size_t)N + 3;
  uint32_t* lst = bsum + nblk(N, SCAN_BLK) + 1;
  G1P* part[2] = {partA, partB};
  hipError_t e;
  hipLaunchKernelGGL(k_g1vm_records, dim3(nblk(n, 256)), dim3(256), 0, st, pts, ok, n, rec, plive);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = hipMemsetAsync(cnt, 0, (size_t)N * sizeof(uint32_t), st)) != hipSuccess) return e;
  const unsigned sb = nblk((size_t)n * B, 256);
  hipLaunchKernelGGL(k_g1vm_sort<false>, dim3(sb), dim3(256), 0, st, plive, n, B, k32, cnt, nullptr);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = g1m_scan(st, cnt, N, offA, bsum, cur)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_g1vm_sort<true>, dim3(sb), dim3(256), 0, st, plive, n, B, k32, cur, lst);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (d_entries) *d_entries = offA + N;
  if ((e = g1m_reduce(st, p, N, G, rec, lst, cnt, offA, offL, bsum, part, U, W, wlive)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_g1vm_combine, dim3(nblk(B, 64)), dim3(64), 0, st, W, B, res, live);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = launch_g1_affine(st, B, live, res, aff)) != hipSuccess) return e;
  if (!out48) return hipSuccess;
  hipLaunchKernelGGL(k_g1m_compress, dim3(nblk(B, 64)), dim3(64), 0, st, aff, B, out48);
  return hipGetLastError();
}

}  // namespace bls
