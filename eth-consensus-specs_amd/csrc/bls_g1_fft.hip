// Kernels of the G1 transform and of the cell proofs' scalar rows (pieces, index maps and the derivation:
// bls_g1_fft.h; C ABI: bls_capi_kzg_cells.hip).
//
//   k_g1fft_load      decoded or MSM-made affine points -> the transform's buffer of canonical projective points,
//                     `have` given points per vector and the identity above them
//   k_g1fft_stage     one stage: one lane per butterfly over all B vectors, t = [z] b by a 128-step joint double-and-add
//                     through the endomorphism (no chain where z = 1 or b is the identity), then (a + t, a - t)
//   k_g1fft_scale     the inverse's 1 / n: one lane per point
//   k_g1fft_finish    the buffer in its output order (bit-reversed as it stands, or natural) with the live flags
//                     launch_g1_affine reads
//   k_g1fft_compress  affine points -> 48 bytes
//   k_cellproof_rows  S_KC_COEF's coefficient forms -> the 63 shifted, zero-filled scalar rows per blob
#include "bls_kernels.h"
#include "bls_g1_fft.h"

namespace bls {

namespace {
inline unsigned nblk(size_t n, unsigned t) { return (unsigned)((n + t - 1) / t); }
}  // namespace

__global__ void __launch_bounds__(256) k_g1fft_load(const G1A* src, const int* live, uint32_t have, uint32_t logn,
                                                    size_t total, G1P* buf) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= total) return;
  const size_t v = g >> logn;
  const uint32_t i = (uint32_t)(g & ((1u << logn) - 1u));
  const size_t j = i < have ? v * have + i : 0;  // entry 0 exists: B, have >= 1
  const G1A a = src[j];
  const bool pt = i < have && !a.inf && (!live || live[j]);
  // selects and field-wise stores, as k_g1t_first: no G1P temporary
  G1P* o = buf + g;
  o->x = fp_select(pt, a.x, fp_zero());
  o->y = fp_select(pt, a.y, FP_ONE);
  o->z = fp_select(pt, FP_ONE, fp_zero());
}

__global__ void __launch_bounds__(64) k_g1fft_stage(G1P* buf, uint32_t logn, uint32_t s, size_t B, const Fr* W,
                                                    uint32_t inv) {
  g1fft_stage(buf, logn, s, B, W, inv != 0, (size_t)blockIdx.x * 64 + threadIdx.x, (size_t)gridDim.x * 64);
}

__global__ void __launch_bounds__(64) k_g1fft_scale(G1P* buf, uint32_t logn, size_t B) {
  g1fft_scale(buf, logn, B, (size_t)blockIdx.x * 64 + threadIdx.x, (size_t)gridDim.x * 64);
}

__global__ void __launch_bounds__(256) k_g1fft_finish(const G1P* buf, uint32_t logn, size_t total, uint32_t natural,
                                                      G1P* out, int* live) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= total) return;
  const uint32_t i = (uint32_t)(g & ((1u << logn) - 1u));
  const size_t o = g - i + g1fft_out_index(logn, i, natural != 0);
  const G1P p = buf[g];
  out[o] = p;
  live[o] = fp_is_zero(p.z) ? 0 : 1;
}

__global__ void __launch_bounds__(64) k_g1fft_compress(const G1A* a, size_t n, uint8_t* out48) {
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i < n) g1_compress(out48 + 48 * i, a[i]);
}

// lane g: entry i of row m of blob b, g = (b 63 + m) 4,032 + i
__global__ void __launch_bounds__(256) k_cellproof_rows(const Fr* coef, size_t total, uint8_t* rows32) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= total) return;
  const size_t row = g / CELLPROOF_ROW_N;
  const uint32_t i = (uint32_t)(g % CELLPROOF_ROW_N), m = (uint32_t)(row % CELLPROOF_ROWS);
  fr_to_be32(cellproof_row_entry(coef + (row / CELLPROOF_ROWS) * NTT_BLOB, m, i), rows32 + 32 * g);
}

// ======================================================= host launchers ==
#define LAUNCH(k, g, b, st, ...)                                 \
  do {                                                           \
    hipLaunchKernelGGL(k, dim3(g), dim3(b), 0, st, __VA_ARGS__); \
    hipError_t e__ = hipGetLastError();                          \
    if (e__ != hipSuccess) return e__;                           \
  } while (0)

hipError_t launch_g1fft_load(hipStream_t st, const G1A* src, const int* live, uint32_t have, uint32_t logn, size_t B,
                             G1P* buf) {
  if (!B) return hipSuccess;
  if (logn < 1 || logn > G1FFT_LOG_MAX || !have || have > (1u << logn)) return hipErrorInvalidValue;
  const size_t total = B << logn;
  LAUNCH(k_g1fft_load, nblk(total, 256), 256, st, src, live, have, logn, total, buf);
  return hipSuccess;
}

hipError_t launch_g1fft(hipStream_t st, const Fr* W, uint32_t logn, bool inverse, size_t B, G1P* buf) {
  if (!B) return hipSuccess;
  if (logn < 1 || logn > G1FFT_LOG_MAX) return hipErrorInvalidValue;
  const unsigned blocks = nblk(B << (logn - 1), 64);
  for (uint32_t s = 0; s < logn; ++s) LAUNCH(k_g1fft_stage, blocks, 64, st, buf, logn, s, B, W, inverse ? 1u : 0u);
  if (inverse) LAUNCH(k_g1fft_scale, nblk(B << logn, 64), 64, st, buf, logn, B);
  return hipSuccess;
}

hipError_t launch_g1fft_finish(hipStream_t st, const G1P* buf, uint32_t logn, size_t B, bool natural, G1P* out,
                               int* live, G1A* aff, uint8_t* out48) {
  if (!B) return hipSuccess;
  if (logn < 1 || logn > G1FFT_LOG_MAX) return hipErrorInvalidValue;
  const size_t total = B << logn;
  LAUNCH(k_g1fft_finish, nblk(total, 256), 256, st, buf, logn, total, natural ? 1u : 0u, out, live);
  const hipError_t e = launch_g1_affine(st, total, live, out, aff);
  if (e != hipSuccess) return e;
  LAUNCH(k_g1fft_compress, nblk(total, 64), 64, st, aff, total, out48);
  return hipSuccess;
}

size_t cellproof_rows_per_blob() { return CELLPROOF_ROWS; }
size_t cellproof_row_entries() { return CELLPROOF_ROW_N; }

hipError_t launch_cellproof_rows(hipStream_t st, const Fr* coef, size_t B, uint8_t* rows32) {
  if (!B) return hipSuccess;
  const size_t total = B * CELLPROOF_ROWS * CELLPROOF_ROW_N;
  LAUNCH(k_cellproof_rows, nblk(total, 256), 256, st, coef, total, rows32);
  return hipSuccess;
}

}  // namespace bls
