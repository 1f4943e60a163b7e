// Kernels of the shared-message FAV batch (bls_capi.hip fav_prepare with a grouping):
//   k_g1_seg_fold   one level of the segmented G1 sum (bls_g1_segsum.h): one lane per run, complete additions in
//                   the redundant digit form in registers; no cross-lane operation, no LDS, no private segment
//   k_g2a_gather    the bisection's per-item H: H_item[i] = H[msg_id[i]]
// The M sums go to affine through launch_g1_affine (one inversion per 8) with the fold's ok as status.
// Kernels of grouped signature aggregation (bls_capi.hip bls_aggregate_grouped):
//   k_g2_seg_fold   one level of the segmented G2 sum (bls_g2_segsum.h), the G2 counterpart of k_g1_seg_fold
//   k_g2_seg_finish the G projective sums to compressed signatures and ok, one inversion per 4 groups
#include <utility>

#include "bls_kernels.h"
#include "bls_g1_segsum.h"
#include "bls_g2_segsum.h"
#include "bls_tower_inline.h"
#include "bls_fp_inv.h"

namespace bls {

namespace {
inline unsigned nblk(size_t n, unsigned t) { return (unsigned)((n + t - 1) / t); }
}  // namespace

// L0: the runs read item points (affine r_i apk_i through the sorted item list); else the partials of the level below.
// At least two waves per SIMD (198 / 159 registers, no private segment): it runs beside the one-wave lane kernels,
// as the registry gather does.
template <bool L0>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2)))
k_g1_seg_fold(const SegRun* runs, uint32_t nruns, const uint32_t* items, const int* status, const G1A* rP,
              const G1P* prev, G1P* tmp, G1P* gsum, int* ok) {
  const uint32_t t = blockIdx.x * 64 + threadIdx.x;
  if (t >= nruns) return;
  const SegRun r = runs[t];
  const G1Q acc = L0 ? seg_fold_items(r, items, status, rP) : seg_fold_partials(r, prev);
  seg_store(r, acc, tmp, gsum, ok);
}

__global__ void __launch_bounds__(256) k_g2a_gather(size_t B, const G2A* H, const uint32_t* msg_id, G2A* out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < B) out[i] = H[msg_id[i]];
}

// ------------------------------------------------------------ grouped signature aggregation (bls_aggregate_grouped)
// One level of the segmented G2 sum: one lane per run, the accumulator (84 digits) and one complete addition's
// temporaries in registers -- one wave per SIMD, as every other one-lane G2 kernel here; no cross-lane operation, no
// LDS, no private segment (DESIGN.md 4.8 has the resource table).
template <bool L0>
__global__ void __launch_bounds__(64)
k_g2_seg_fold(const SegRun* runs, uint32_t nruns, const uint32_t* items, const int* ok, const uint8_t* include,
              const G2A* a, const G2SP* prev, G2SP* tmp, G2SP* gsum) {
  const uint32_t t = blockIdx.x * 64 + threadIdx.x;
  if (t >= nruns) return;
  const SegRun r = runs[t];
  uint32_t flags;
  const G2Q acc = L0 ? seg2_fold_items(r, items, ok, include, a, flags) : seg2_fold_partials(r, prev, flags);
  seg2_store(r, acc, flags, tmp, gsum);
}

// The G sums to compressed bytes and ok.  A group is ok when it has an included member and no bad one; its bytes
// are then the compressed affine sum -- c0 00.. when the sum is the identity (Z = 0) -- and 96 zero bytes otherwise.
// Each lane converts FIN_K groups (group w * 64 FIN_K + lane + 64 k) with ONE inversion: 1 / Z = conj(Z) / norm(Z)
// and Montgomery's trick over the FIN_K norms (k_h2c_affine_b's scheme; norm(Z) = 0 only for Z = 0 since -1 is a
// non-residue).  The sign bit is the lexicographic order of y (g2_compress).
constexpr int FIN_K = 4;
template <class F, int... K>
__device__ __forceinline__ void fin_walk_back(F&& f, std::integer_sequence<int, K...>) {
  (f(std::integral_constant<int, (int)sizeof...(K) - 1 - K>{}), ...);
}
template <class F, int... K>
__device__ __forceinline__ void fin_walk(F&& f, std::integer_sequence<int, K...>) {
  (f(std::integral_constant<int, K>{}), ...);
}

__global__ void __launch_bounds__(64) k_g2_seg_finish(size_t G, const G2SP* gsum, uint8_t* out96, uint8_t* out_ok) {
  const size_t base = (size_t)blockIdx.x * 64 * FIN_K + threadIdx.x;
  Fp pre[FIN_K];
  bool live[FIN_K];
  Fp acc = FP_ONE;
  fin_walk([&](auto kc) {
    constexpr int k = decltype(kc)::value;
    const size_t g = base + 64 * k;
    Fp n = FP_ONE;
    live[k] = false;
    if (g < G && gsum[g].flags == G2S_SOME) {
      const Fp2 Z = gsum[g].z;
      const Fp nz = fp_add(fp_sqr_i(Z.c0), fp_sqr_i(Z.c1));
      live[k] = !fp_is_zero(nz);
      if (live[k]) n = nz;
    }
    acc = fp_mul_i(acc, n);
    pre[k] = acc;
  }, std::make_integer_sequence<int, FIN_K>{});
  Fp inv = fp_inv_sg_i(acc);  // 1 / (n_0 ... n_{K-1})
  fin_walk_back([&](auto kc) {
    constexpr int k = decltype(kc)::value;
    const size_t g = base + 64 * k;
    if (g >= G) return;
    const bool okg = gsum[g].flags == G2S_SOME;
    uint8_t* o = out96 + 96 * g;
    if (live[k]) {
      const G2SP s = gsum[g];
      const Fp ni = k ? fp_mul_i(inv, pre[k ? k - 1 : 0]) : inv;  // 1 / norm(Z)
      if (k) inv = fp_mul_i(inv, fp_add(fp_sqr_i(s.z.c0), fp_sqr_i(s.z.c1)));
      const Fp2 zi{fp_mul_i(s.z.c0, ni), fp_neg(fp_mul_i(s.z.c1, ni))};
      g2_compress(o, G2A{f2mul(s.x, zi), f2mul(s.y, zi), false});
    } else {
      for (int b = 0; b < 96; ++b) o[b] = 0;
      if (okg) o[0] = 0xc0;
    }
    out_ok[g] = okg ? 1 : 0;
  }, std::make_integer_sequence<int, FIN_K>{});
}

size_t g2_seg_partial_bytes() { return sizeof(G2SP); }

hipError_t launch_g2_seg_fold(hipStream_t st, int level, const SegRun* runs, uint32_t nruns, const uint32_t* items,
                              const int* ok, const uint8_t* include, const G2A* a, const G2SP* prev, G2SP* tmp,
                              G2SP* gsum) {
  if (!nruns) return hipSuccess;
  if (level == 0)
    hipLaunchKernelGGL(k_g2_seg_fold<true>, dim3(nblk(nruns, 64)), dim3(64), 0, st, runs, nruns, items, ok, include, a,
                       prev, tmp, gsum);
  else
    hipLaunchKernelGGL(k_g2_seg_fold<false>, dim3(nblk(nruns, 64)), dim3(64), 0, st, runs, nruns, items, ok, include,
                       a, prev, tmp, gsum);
  return hipGetLastError();
}

hipError_t launch_g2_seg_finish(hipStream_t st, size_t G, const G2SP* gsum, uint8_t* out96, uint8_t* out_ok) {
  if (!G) return hipSuccess;
  hipLaunchKernelGGL(k_g2_seg_finish, dim3(nblk(G, 64 * FIN_K)), dim3(64), 0, st, G, gsum, out96, out_ok);
  return hipGetLastError();
}

hipError_t launch_g1_seg_fold(hipStream_t st, int level, const SegRun* runs, uint32_t nruns, const uint32_t* items,
                              const int* status, const G1A* rP, const G1P* prev, G1P* tmp, G1P* gsum, int* ok) {
  if (!nruns) return hipSuccess;
  if (level == 0)
    hipLaunchKernelGGL(k_g1_seg_fold<true>, dim3(nblk(nruns, 64)), dim3(64), 0, st, runs, nruns, items, status, rP,
                       prev, tmp, gsum, ok);
  else
    hipLaunchKernelGGL(k_g1_seg_fold<false>, dim3(nblk(nruns, 64)), dim3(64), 0, st, runs, nruns, items, status, rP,
                       prev, tmp, gsum, ok);
  return hipGetLastError();
}

hipError_t launch_g2a_gather(hipStream_t st, size_t B, const G2A* H, const uint32_t* msg_id, G2A* out) {
  if (!B) return hipSuccess;
  hipLaunchKernelGGL(k_g2a_gather, dim3(nblk(B, 256)), dim3(256), 0, st, B, H, msg_id, out);
  return hipGetLastError();
}

}  // namespace bls
