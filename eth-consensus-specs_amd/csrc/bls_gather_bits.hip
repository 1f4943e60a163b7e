// Kernels of the committee-bitfield FAV batch (bls_capi.hip fav_prepare with bits; the algorithm is in
// bls_g1_bits.h):
//   k_bits_expand       one wave per item: counts the item's bits, picks direct or complement, and compacts the
//                       wanted members' registry indices into a list with 64-bit ballots and prefix popcounts, so
//                       that the gather's lanes stay balanced whatever the participation is
//   k_fav_gather_bits   k_fav_gather_q's lane schedule over those lists (L lanes per item, software-pipelined record
//                       loads, complete additions); a complement item's lanes negate their partial sums and add
//                       their shares of the committee sums before the same LDS tree.  On the committee table itself
//                       (bls_committees_load) it computes csum[c] and exports cstat[c] apart from the identity check.
#include "bls_kernels.h"
#include "bls_g1_bits.h"

namespace bls {

namespace {

// the executor of bits_expand_item on a wave: lane-private callbacks, cross-lane ballot / reduction
struct WaveExec {
  uint32_t lane;
  template <class F>
  __device__ __forceinline__ uint64_t ballot(F f) {
    return __ballot(f(lane) ? 1 : 0);
  }
  template <class F>
  __device__ __forceinline__ void each(F f) {
    f(lane);
  }
  template <class F>
  __device__ __forceinline__ uint64_t sum(F f) {
    unsigned long long v = f(lane);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
  }
  template <class F>
  __device__ __forceinline__ bool all(F f) {
    return __all(f(lane) ? 1 : 0) != 0;
  }
};

}  // namespace

// The inputs and the list never alias (__restrict__): the loads of a step do not wait for the stores of the one before.
__global__ void __launch_bounds__(64) k_bits_expand(size_t B, int mode, const uint32_t* __restrict__ comm_ids,
                                                    const uint64_t* __restrict__ comm_offs,
                                                    const uint8_t* __restrict__ bits,
                                                    const uint64_t* __restrict__ bit_offs,
                                                    const uint64_t* __restrict__ slot_offs,
                                                    const uint32_t* __restrict__ tab_idx,
                                                    const uint64_t* __restrict__ tab_offs,
                                                    const int* __restrict__ cstat, uint32_t* __restrict__ list,
                                                    BitsItem* __restrict__ items) {
  const size_t b = blockIdx.x;
  if (b >= B) return;
  WaveExec ex{(uint32_t)threadIdx.x};
  const uint64_t co = comm_offs[b], ncomm = comm_offs[b + 1] - co;
  const uint64_t start = slot_offs[b], n = slot_offs[b + 1] - start;
  const BitsItem it = bits_expand_item(ex, mode, comm_ids + co, ncomm, tab_idx, tab_offs, cstat, bits + bit_offs[b], n,
                                       start, list);
  if (threadIdx.x == 0) items[b] = it;
}

// comm_ids / comm_offs / csum: read for complement items only (null on the committee table's own sums).
// members_ok (nullable): 1 iff every listed key was in range and valid -- the committee table's cstat.
template <int L>
__global__ void __launch_bounds__(64) k_fav_gather_bits(const uint32_t* idx, const BitsItem* items, size_t B,
                                                        const RegKey* reg, uint32_t reg_n, const uint32_t* comm_ids,
                                                        const uint64_t* comm_offs, const G1P* csum, G1P* apk,
                                                        int* status, int* members_ok) {
  constexpr int IPW = 64 / L;
  __shared__ G1Q sh[64];
  __shared__ int bad[IPW];
  const int sub = (int)threadIdx.x / L, ln = (int)threadIdx.x % L;
  const size_t b = (size_t)blockIdx.x * IPW + sub;
  const bool mine = b < B;
  if ((int)threadIdx.x < IPW) bad[threadIdx.x] = 0;
  __syncthreads();
  G1Q acc{fq_zero(), fq_unpack(FP_ONE), fq_zero()};  // identity (0 : 1 : 0)
  int mybad = 0;
  uint32_t flags = 0;
  if (mine) {
    const BitsItem it = items[b];
    flags = it.flags;
    const uint64_t lo = it.start, hi = it.start + it.len;
    // k_fav_gather_q's software pipeline: the record of key j + L and the index of key j + 2L are in flight while
    // key j is added (an out-of-range index reads record 0 and is flagged; every load is unconditional)
    uint64_t j = lo + ln;
    uint32_t k1 = j < hi ? idx[j] : 0u;
    const uint32_t* rw = reinterpret_cast<const uint32_t*>(reg + (k1 < reg_n ? k1 : 0u));
    uint4 r[6];
#pragma unroll
    for (int w = 0; w < 6; ++w) r[w] = reinterpret_cast<const uint4*>(rw)[w];
    uint32_t k2 = j + L < hi ? idx[j + L] : 0u;
#pragma unroll 1
    for (; j < hi; j += L) {
      uint4 cr[6];
#pragma unroll
      for (int w = 0; w < 6; ++w) cr[w] = r[w];
      const uint32_t ck = k1;
      k1 = k2;
      const uint4* nr = reinterpret_cast<const uint4*>(reg + (k1 < reg_n ? k1 : 0u));
#pragma unroll
      for (int w = 0; w < 6; ++w) r[w] = nr[w];
      k2 = j + 2 * L < hi ? idx[j + 2 * L] : 0u;
      Fp x, y;
#pragma unroll
      for (int w = 0; w < 3; ++w) {
        reinterpret_cast<uint4*>(x.l)[w] = cr[w];
        reinterpret_cast<uint4*>(y.l)[w] = cr[3 + w];
      }
      if (ck >= reg_n || !(x.l[11] & REG_VALID)) {
        mybad = 1;
      } else {
        x.l[11] &= ~REG_VALID;
        acc = g1q_add_aff(acc, fq_unpack(x), fq_unpack(y));
      }
    }
    if (flags & BITS_F_COMPLEMENT) {
      const uint64_t co = comm_offs[b];
      acc = bits_lane_combine(acc, flags, comm_ids + co, comm_offs[b + 1] - co, csum, (uint32_t)ln, (uint32_t)L);
    }
  }
  if (mybad) atomicOr(&bad[sub], 1);
  sh[threadIdx.x] = acc;
  __syncthreads();
#pragma unroll 1
  for (int s = L / 2; s > 0; s >>= 1) {
    if (ln < s) sh[threadIdx.x] = g1q_add(sh[threadIdx.x], sh[threadIdx.x + s]);
    __syncthreads();
  }
  if (ln == 0 && mine) {  // canonical projective aggregate key; the identity is invalid (KeyValidate of the sum)
    const G1Q& a = sh[threadIdx.x];
    const G1P o{fq_pack(a.x), fq_pack(a.y), fq_pack(a.z)};
    apk[b] = o;
    status[b] = ((flags & BITS_F_SOME) && !(flags & BITS_F_MALFORMED) && !bad[sub] && !fp_is_zero(o.z)) ? 1 : 0;
    if (members_ok) members_ok[b] = bad[sub] ? 0 : 1;
  }
}

hipError_t launch_bits_expand(hipStream_t st, size_t B, int mode, const uint32_t* comm_ids, const uint64_t* comm_offs,
                              const uint8_t* bits, const uint64_t* bit_offs, const uint64_t* slot_offs,
                              const uint32_t* tab_idx, const uint64_t* tab_offs, const int* cstat, uint32_t* list,
                              BitsItem* items) {
  if (!B) return hipSuccess;
  hipLaunchKernelGGL(k_bits_expand, dim3((unsigned)B), dim3(64), 0, st, B, mode, comm_ids, comm_offs, bits, bit_offs,
                     slot_offs, tab_idx, tab_offs, cstat, list, items);
  return hipGetLastError();
}

// lanes per aggregate: 16 from 1,024 aggregates up, else 64 (launch_fav_gather goes on to 4 lanes for full batches
// with its pair-first loop; this kernel keeps one key per step)
hipError_t launch_fav_gather_bits(hipStream_t st, const uint32_t* list, const BitsItem* items, size_t B,
                                  const RegKey* reg, uint32_t reg_n, const uint32_t* comm_ids,
                                  const uint64_t* comm_offs, const G1P* csum, G1P* apk, int* status,
                                  int* members_ok) {
  if (!B) return hipSuccess;
  if (B >= 1024)
    hipLaunchKernelGGL(k_fav_gather_bits<16>, dim3((unsigned)((B + 3) / 4)), dim3(64), 0, st, list, items, B, reg,
                       reg_n, comm_ids, comm_offs, csum, apk, status, members_ok);
  else
    hipLaunchKernelGGL(k_fav_gather_bits<64>, dim3((unsigned)B), dim3(64), 0, st, list, items, B, reg, reg_n,
                       comm_ids, comm_offs, csum, apk, status, members_ok);
  return hipGetLastError();
}

}  // namespace bls
