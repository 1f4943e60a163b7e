// Deneb blob KZG kernels (specs/deneb/polynomial-commitments.md; the lane pieces and the mathematics are in
// bls_kzg_blob.h, the field in bls_fr.h; C ABI: bls_capi_kzg.hip).
//
//   k_fr_domain       the 4,096 domain entries omega^brp(i), once per context
//   k_blob_decode     blob bytes -> Montgomery limbs, ok[b] = every element < r
//   k_fr_decode       n 32-byte scalars -> Montgomery limbs and their < r verdicts (z, y)
//   k_blob_eval       y_b = p_b(z_b): one workgroup of 256 lanes per blob, 16 elements and one inversion per lane
//   k_blob_quotient   the quotient's evaluation form as the table MSM's scalar rows, the same partition
//   k_kzg_rlc         the random-linear-combination scalars of a verification batch and the points they multiply
//   k_kzg_pairs       the batch check's two Miller pairs from its two sums
//   k_kzg_item_pairs  every item's own two pairs (after a failed batch check)
//
// The evaluation and quotient kernels keep a lane's 16 prefix products in a scratch array in memory (`pre`, 4,096
// slots per blob), so their loops stay rolled and the private segment is empty (bls_kzg_blob.h).
#include "bls_kernels.h"
#include "bls_curve.h"
#include "bls_kzg_blob.h"
#include "bls_sha256.h"

namespace bls {

namespace {
inline unsigned nblk(size_t n, unsigned t) { return (unsigned)((n + t - 1) / t); }

// the sum of the workgroup's 256 values, returned to lane 0 (sh: 256 entries)
__device__ __forceinline__ Fr wg_sum(Fr v, Fr* sh) {
  const uint32_t t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
#pragma unroll 1
  for (uint32_t s = KZB_LANES / 2; s; s >>= 1) {
    if (t < s) sh[t] = fr_add(sh[t], sh[t + s]);
    __syncthreads();
  }
  return sh[0];
}
}  // namespace

__global__ void __launch_bounds__(256) k_fr_domain(Fr* dom) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < KZB_N) dom[i] = kzb_domain_entry(i);
}

// one workgroup per blob; lane t takes elements t, t + 256, ... (adjacent lanes read adjacent 32 bytes)
__global__ void __launch_bounds__(256) k_blob_decode(const uint8_t* blobs, Fr* f, int* ok) {
  const size_t b = blockIdx.x;
  int good = 1;
#pragma unroll 1
  for (uint32_t i = threadIdx.x; i < KZB_N; i += KZB_LANES) {
    Fr v;
    if (!fr_from_be32(v, blobs + (b * KZB_N + i) * 32)) good = 0;
    f[b * KZB_N + i] = v;
  }
  good = __syncthreads_and(good);
  if (threadIdx.x == 0) ok[b] = good;
}

__global__ void __launch_bounds__(64) k_fr_decode(const uint8_t* in32, size_t n, Fr* out, int* ok) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Fr v;
  ok[i] = fr_from_be32(v, in32 + 32 * i) ? 1 : 0;
  out[i] = v;
}

// ok (nullable): a blob with ok[b] = 0 gives y = 0 and no hit
__global__ void __launch_bounds__(256) k_blob_eval(const Fr* dom, const Fr* f, const Fr* z, const int* ok, Fr* pre,
                                                   Fr* y, uint8_t* y32, int* hit) {
  __shared__ Fr sh[KZB_LANES];
  __shared__ int sh_hit;
  const size_t b = blockIdx.x;
  const Fr* fb = f + b * KZB_N;
  if (threadIdx.x == 0) sh_hit = -1;
  __syncthreads();
  const Fr zb = z[b];
  const KzbLane r = kzb_eval_lane(dom, fb, zb, threadIdx.x, pre + b * KZB_N);
  if (r.hit >= 0) sh_hit = r.hit;  // at most one lane: the domain's entries are distinct
  const Fr total = wg_sum(r.sum, sh);
  if (threadIdx.x) return;
  const bool good = !ok || ok[b];
  const int h = good ? sh_hit : -1;
  const Fr v = good ? kzb_eval_finish(total, zb, fb, h) : fr_zero();
  y[b] = v;
  hit[b] = h;
  fr_to_be32(v, y32 + 32 * b);
}

__global__ void __launch_bounds__(256) k_blob_quotient(const Fr* dom, const Fr* f, const Fr* z, const Fr* y,
                                                       const int* hit, Fr* pre, uint8_t* q32) {
  __shared__ Fr sh[KZB_LANES];
  const size_t b = blockIdx.x;
  const int h = hit[b];
  const Fr zb = z[b];
  uint8_t* row = q32 + b * KZB_N * 32;
  const Fr s = kzb_quot_lane(dom, f + b * KZB_N, zb, y[b], h, threadIdx.x, row, pre + b * KZB_N);
  if (h < 0) return;  // uniform: the whole workgroup leaves
  const Fr total = wg_sum(s, sh);
  if (threadIdx.x == 0) kzb_quot_finish(total, zb, h, row);
}

// Item i's r_i: the first 16 bytes of SHA-256(seed32 || i as 8 big-endian bytes), a 128-bit integer.
// Points P (3 n + 1 of them; the caller decoded the commitments into P[0 .. n) and the proofs into P[n .. 2 n)) and
// their scalar rows k32:
//   [0, n)            C_i     r_i
//   [n, 2 n)          pi_i    r_i z_i
//   2 n               G1      -sum r_i y_i
//   [2 n + 1, 3 n + 1)  pi_i  r_i
// One workgroup; lanes stride over the items.
__global__ void __launch_bounds__(256) k_kzg_rlc(const uint8_t* seed32, size_t n, const Fr* z, const Fr* y, G1A* P,
                                                 uint8_t* k32) {
  __shared__ Fr sh[KZB_LANES];
  Fr acc = fr_zero();
#pragma unroll 1
  for (size_t i = threadIdx.x; i < n; i += KZB_LANES) {
    Sha256 s;
    sha256_init(s);
    sha256_update(s, seed32, 32);
    for (int k = 7; k >= 0; --k) sha256_byte(s, (uint8_t)((uint64_t)i >> (8 * k)));
    uint8_t h[32];
    sha256_final(s, h);
    uint8_t rb[32];
    for (int k = 0; k < 16; ++k) rb[k] = 0, rb[16 + k] = h[k];
    const Fr r = fr_to_mont(fr_raw_from_be32(rb));  // < 2^128 < r
    for (int k = 0; k < 32; ++k) k32[32 * i + k] = rb[k], k32[32 * (2 * n + 1 + i) + k] = rb[k];
    fr_to_be32(fr_mul(r, z[i]), k32 + 32 * (n + i));
    acc = fr_add(acc, fr_mul(r, y[i]));
    P[2 * n + 1 + i] = P[n + i];
  }
  const Fr total = wg_sum(acc, sh);
  if (threadIdx.x) return;
  fr_to_be32(fr_neg(total), k32 + 32 * (2 * n));
  P[2 * n] = g1_generator();
}

// sums[0] = sum r_i C_i + sum r_i z_i pi_i - (sum r_i y_i) G1, sums[1] = sum r_i pi_i:
// e(sums[1], -[tau] G2) e(sums[0], G2) is the batch's product
__global__ void __launch_bounds__(64) k_kzg_pairs(const G1J* sums, const G2A* negtau, G1A* P, G2A* Q) {
  const uint32_t t = threadIdx.x;
  if (t >= 2) return;
  P[t] = jac_to_aff(sums[1 - t]);
  Q[t] = t ? g2_generator() : *negtau;
}

// item i's pairs (pi_i, -[tau] G2) and (C_i + [z_i] pi_i - [y_i] G1, G2) at P / Q[2 i], [2 i + 1]; CP: the decoded
// commitments, then the proofs
__global__ void __launch_bounds__(64) k_kzg_item_pairs(size_t n, const G1A* CP, const Fr* z, const Fr* y,
                                                       const G2A* negtau, G1A* P, G2A* Q) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const G1A pi = CP[n + i];
  const Fr zk = fr_from_mont(z[i]), yk = fr_from_mont(fr_neg(y[i]));
  G1J x = jac_from_aff(CP[i]);
  x = jac_add(x, jac_mul_u256(jac_from_aff(pi), zk.l));
  x = jac_add(x, jac_mul_u256(jac_from_aff(g1_generator()), yk.l));
  P[2 * i] = pi;
  Q[2 * i] = *negtau;
  P[2 * i + 1] = jac_to_aff(x);
  Q[2 * i + 1] = g2_generator();
}

__global__ void k_kzg_g2_neg(G2A* q) {
  if (threadIdx.x || blockIdx.x) return;
  if (!q->inf) q->y = fp2_neg(q->y);
}

// ======================================================= host launchers ==
#define LAUNCH(k, g, b, st, ...)                                 \
  do {                                                           \
    hipLaunchKernelGGL(k, dim3(g), dim3(b), 0, st, __VA_ARGS__); \
    hipError_t e__ = hipGetLastError();                          \
    if (e__ != hipSuccess) return e__;                           \
  } while (0)

size_t kzg_domain_bytes() { return KZB_N * sizeof(Fr); }

hipError_t launch_fr_domain(hipStream_t st, Fr* dom) {
  LAUNCH(k_fr_domain, KZB_N / 256, 256, st, dom);
  return hipSuccess;
}
hipError_t launch_blob_decode(hipStream_t st, const uint8_t* blobs, size_t B, Fr* f, int* ok) {
  if (!B) return hipSuccess;
  LAUNCH(k_blob_decode, (unsigned)B, KZB_LANES, st, blobs, f, ok);
  return hipSuccess;
}
hipError_t launch_fr_decode(hipStream_t st, const uint8_t* in32, size_t n, Fr* out, int* ok) {
  if (!n) return hipSuccess;
  LAUNCH(k_fr_decode, nblk(n, 64), 64, st, in32, n, out, ok);
  return hipSuccess;
}
hipError_t launch_blob_eval(hipStream_t st, const Fr* dom, const Fr* f, const Fr* z, const int* ok, size_t B, Fr* pre,
                            Fr* y, uint8_t* y32, int* hit) {
  if (!B) return hipSuccess;
  LAUNCH(k_blob_eval, (unsigned)B, KZB_LANES, st, dom, f, z, ok, pre, y, y32, hit);
  return hipSuccess;
}
hipError_t launch_blob_quotient(hipStream_t st, const Fr* dom, const Fr* f, const Fr* z, const Fr* y, const int* hit,
                                size_t B, Fr* pre, uint8_t* q32) {
  if (!B) return hipSuccess;
  LAUNCH(k_blob_quotient, (unsigned)B, KZB_LANES, st, dom, f, z, y, hit, pre, q32);
  return hipSuccess;
}
hipError_t launch_kzg_rlc(hipStream_t st, const uint8_t* seed32, size_t n, const Fr* z, const Fr* y, G1A* P,
                          uint8_t* k32) {
  LAUNCH(k_kzg_rlc, 1, KZB_LANES, st, seed32, n, z, y, P, k32);
  return hipSuccess;
}
hipError_t launch_kzg_pairs(hipStream_t st, const G1J* sums, const G2A* negtau, G1A* P, G2A* Q) {
  LAUNCH(k_kzg_pairs, 1, 64, st, sums, negtau, P, Q);
  return hipSuccess;
}
hipError_t launch_kzg_item_pairs(hipStream_t st, size_t n, const G1A* CP, const Fr* z, const Fr* y,
                                 const G2A* negtau, G1A* P, G2A* Q) {
  if (!n) return hipSuccess;
  LAUNCH(k_kzg_item_pairs, nblk(n, 64), 64, st, n, CP, z, y, negtau, P, Q);
  return hipSuccess;
}
hipError_t launch_kzg_g2_neg(hipStream_t st, G2A* q) {
  LAUNCH(k_kzg_g2_neg, 1, 64, st, q);
  return hipSuccess;
}

}  // namespace bls
