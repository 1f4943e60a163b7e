// Kernels of the shared-message FAV batch (bls_capi.hip fav_prepare with a grouping):
//   k_g1_seg_fold   one level of the segmented G1 sum (bls_g1_segsum.h): one lane per run, complete additions in
//                   the redundant digit form in registers; no cross-lane operation, no LDS, no private segment
//   k_g2a_gather    the bisection's per-item H: H_item[i] = H[msg_id[i]]
// The M sums go to affine through launch_g1_affine (one inversion per 8) with the fold's ok as status.
#include "bls_kernels.h"
#include "bls_g1_segsum.h"

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
